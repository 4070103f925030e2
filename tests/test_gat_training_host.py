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


def _layer_bwd(lib, p, nws):
    """egnn_gat_layer_bwd_f32 on a GATConv's operands (H=2, C=4; keep / src_scale / dst_scale NULL) with single fields replaced."""
    desc = dict(rowptr=p, col=p, colptr=p, t_col=p, perm=p, n=2, nnz=3, H=2, C=4, xl=p, ld_xl=8, el=p, er=p, attn_l=p, attn_r=p,
                keep=None, mult=None, src_scale=None, dst_scale=None, negative_slope=0.2)
    args = dict(att=p, go=p, ld_go=8, mean_heads=0, d_raw=p, d_er=p, dxl=p, ld_dxl=8, d_attn=p, ws=p, nws=nws, stream=None)

    def call(**kw):
        d = dict(desc, **{k: v for k, v in kw.items() if k in desc})
        a = dict(args, **{k: v for k, v in kw.items() if k in args})
        assert set(kw) <= set(desc) | set(args)
        layer = _lib.GatLayer(*[d[name] for name, _ in _lib.GatLayer._fields_])
        return lib.egnn_gat_layer_bwd_f32(ctypes.byref(layer), *a.values())
    return call


def test_gat_attention_bwd_argument_errors_without_a_gpu():
    """The target-side operands of the one backward entry point (the former egnn_gat_attention_bwd_f32 cases)."""
    lib = _lib.load()
    p, keep = _buf()
    call = _layer_bwd(lib, p, lib.egnn_gat_layer_bwd_ws_floats(2, 2, 4))
    for bad in (dict(n=-1), dict(nnz=-1), dict(H=0), dict(H=65), dict(C=0), dict(ld_xl=7), dict(ld_go=7),
                dict(rowptr=None), dict(d_er=None), dict(col=None), dict(att=None), dict(xl=None), dict(go=None), dict(d_raw=None),
                dict(el=None)):
        assert call(**bad) == EINVAL, bad
    # go is [n, ld_go >= H*C], or [n, ld_go >= C] for the gradient of the head average; checked before the n == 0 return, and
    # n = 0 keeps a passing call from launching anything
    assert call(n=0, ld_go=7) == EINVAL and call(n=0, ld_go=8) == 0
    assert call(mean_heads=1, ld_go=3) == EINVAL and call(n=0, mean_heads=1, ld_go=3) == EINVAL
    assert call(n=0) == 0 and call(n=0, mean_heads=1, ld_go=4) == 0    # nothing to do, nothing launched
    del keep


def test_gat_aggregate_bwd_argument_errors_without_a_gpu():
    """The source-side operands of the one backward entry point (the former egnn_gat_aggregate_bwd_f32 cases)."""
    lib = _lib.load()
    p, keep = _buf()
    nws = lib.egnn_gat_layer_bwd_ws_floats(2, 2, 4)
    assert nws == 1 * 2 * 2 * 4                                       # one block for two rows, [2, H*C] partial per block
    assert lib.egnn_gat_layer_bwd_ws_floats(-1, 2, 4) == 0
    call = _layer_bwd(lib, p, nws)
    for bad in (dict(n=-1), dict(nnz=-1), dict(H=0), dict(H=65), dict(C=0), dict(ld_dxl=7), dict(ld_xl=7), dict(ld_go=7),
                dict(mean_heads=1, ld_go=3), dict(attn_r=None), dict(er=None), dict(d_er=None), dict(nws=nws - 1), dict(ws=None),
                dict(colptr=None), dict(attn_l=None), dict(dxl=None), dict(perm=None), dict(t_col=None), dict(d_raw=None),
                dict(H=4, C=1024, ld_go=4096, ld_xl=4096, ld_dxl=4096, nws=1 << 20)):   # H*C > 2048 with d_attn
        assert call(**bad) == EINVAL, bad
    assert call(attn_r=None, er=None, d_er=None, n=0) == 0            # a layer without a target-side vector: NULL together
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
