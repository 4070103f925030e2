"""CPU-side checks of the trainable GATConv: the backward entry points (csrc/gat.hip) refuse bad arguments before any launch,
and the PPI training loop refuses an unknown mode."""
import ctypes

import pytest
import torch

import efficient_gnns_amd.models as PM
from efficient_gnns_amd import _lib

EINVAL = -1


def _buf(nbytes=4096):
    b = ctypes.create_string_buffer(nbytes)
    return ctypes.addressof(b), b


def test_gat_attention_bwd_argument_errors_without_a_gpu():
    lib = _lib.load()
    p, keep = _buf()
    #            rowptr col asrc adst att mult xl ld_xl go ld_go go_hs scale n nnz H C slope d_raw d_adst stream
    ok = dict(rowptr=p, col=p, asrc=p, adst=p, att=p, mult=None, xl=p, ld_xl=8, go=p, ld_go=8, go_hs=4, scale=1.0, n=2, nnz=3, H=2,
              C=4, slope=0.2, d_raw=p, d_adst=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.egnn_gat_attention_bwd_f32(*a.values())

    for bad in (dict(n=-1), dict(nnz=-1), dict(H=0), dict(H=65), dict(C=0), dict(ld_xl=7), dict(go_hs=-1), dict(ld_go=7),
                dict(rowptr=None), dict(d_adst=None), dict(col=None), dict(att=None), dict(xl=None), dict(go=None), dict(d_raw=None)):
        assert call(**bad) == EINVAL, bad
    assert call(n=0) == 0                                             # nothing to do, nothing launched
    del keep


def test_gat_aggregate_bwd_argument_errors_without_a_gpu():
    lib = _lib.load()
    p, keep = _buf()
    nws = lib.egnn_gat_aggregate_bwd_ws_floats(2, 2, 4)
    assert nws == 1 * 2 * 2 * 4                                       # one block for two rows, [2, H*C] partial per block
    assert lib.egnn_gat_aggregate_bwd_ws_floats(-1, 2, 4) == 0
    ok = dict(colptr=p, t_col=p, perm=p, att=p, mult=None, d_raw=p, go=p, ld_go=8, go_hs=4, scale=1.0, xl=p, ld_xl=8, att_l=p,
              att_r=p, d_adst=p, n=2, nnz=3, H=2, C=4, dxl=p, ld_dxl=8, d_att=p, ws=p, nws=nws, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.egnn_gat_aggregate_bwd_f32(*a.values())

    for bad in (dict(n=-1), dict(nnz=-1), dict(H=0), dict(H=65), dict(C=0), dict(ld_dxl=7), dict(ld_xl=7), dict(ld_go=7),
                dict(go_hs=-1), dict(att_r=None), dict(d_adst=None), dict(nws=nws - 1), dict(ws=None), dict(colptr=None),
                dict(att_l=None), dict(dxl=None), dict(perm=None), dict(t_col=None), dict(d_raw=None),
                dict(H=4, C=1024, ld_go=4096, go_hs=1024, ld_xl=4096, ld_dxl=4096, nws=1 << 20)):   # H*C > 2048 with d_att
        assert call(**bad) == EINVAL, bad
    assert call(n=0) == 0
    del keep


def test_ppi_train_epoch_rejects_unknown_mode():
    model = PM.StudentNet(8, 3)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    with pytest.raises(NotImplementedError):
        PM.ppi_train_epoch(model, None, [], opt, "crd", {})
    assert set(PM.PPI_MODES) == {"supervised", "kd", "fitnet", "at", "gpw", "lpw", "nce"}


def test_student_net_state_dict_keys_match_the_reference_layout():
    """ppi_pyg/gnn.py:50-83: conv1..5 (2 heads x 68, the last one averaging) and lin1..5."""
    sd = PM.StudentNet(50, 121).state_dict()
    for k in range(1, 6):
        assert f"conv{k}.att_l" in sd and f"conv{k}.lin_l.weight" in sd and f"lin{k}.weight" in sd
    assert sd["conv1.lin_l.weight"].shape == (136, 50)
    assert sd["conv5.att_l"].shape == (1, 2, 121) and sd["conv5.bias"].shape == (121,)
    assert sd["lin5.weight"].shape == (121, 136)
