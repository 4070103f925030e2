"""CPU-side checks of the arxiv GAT teacher training path: the layer descriptor (egnn_gat_layer_t) against its ctypes mirror, the new
entry points declared / exported / bound and refusing bad arguments before any launch, and the host pieces of arxiv_dgl/gat.py
(loss :98-101, label split :121-125, warm-up :110-113) against known answers and the golden recorded from the reference."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import efficient_gnns_amd.models as PM
from conftest import GOLDEN, ROOT, as_t
from efficient_gnns_amd import _lib

EINVAL = -1
NEW_SYMBOLS = ("egnn_gat_layer_fwd_f32", "egnn_gat_layer_bwd_ws_floats", "egnn_gat_layer_bwd_f32")


def _header():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_gat_layer_descriptor_matches_the_header_field_by_field():
    src = _header()
    body = re.search(r"typedef\s+struct\s+egnn_gat_layer\s*\{([^}]*)\}\s*egnn_gat_layer_t\s*;", src).group(1)

    def kind(t):
        t = t.replace("const", "").strip()
        return "p" if t.endswith("*") else {"int64_t": "i64", "int": "i32", "float": "f32", "uint64_t": "u64"}[t]
    want = [(m.group(2), kind(m.group(1))) for m in (re.match(r"(.*?)(\w+)$", d.strip(), flags=re.S) for d in body.split(";") if d.strip())]
    assert len(want) == 20
    kinds = {C.c_void_p: "p", C.c_int64: "i64", C.c_int: "i32", C.c_float: "f32", C.c_uint64: "u64"}
    got = [(name, kinds[t]) for name, t in _lib.GatLayer._fields_]
    assert got == want, f"egnn_gat_layer_t: ctypes {got} vs header {want}"
    for ret, name, args in re.findall(r"\b(int64_t|size_t|int)\s+(egnn_\w+)\s*\(([^;{]*)\)\s*;", src):
        for i, a in enumerate(args.split(",")):
            if "egnn_gat_layer_t" in a:
                assert re.fullmatch(r"\s*const\s+egnn_gat_layer_t\s*\*\s*\w+\s*", a), f"{name}: {a}"
                assert _lib.SIGNATURES[name][1][i] is C.c_void_p, name


REMOVED_SYMBOLS = ("egnn_gat_attention_bwd_f32", "egnn_gat_aggregate_bwd_f32", "egnn_gat_aggregate_bwd_ws_floats")


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_is_9():
    src = _header()
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"{s} is not declared in include/egnn_hip.h"
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert lib.egnn_abi_version() == 9 and re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", src)
    # the coefficient forward keeps its signature; the positional backward pair is gone: one descriptor call for both layers
    assert len(_lib.SIGNATURES["egnn_gat_attention_fwd_f32"][1]) == 10
    assert len(_lib.SIGNATURES["egnn_gat_layer_bwd_f32"][1]) == 13
    whole = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    for s in REMOVED_SYMBOLS:
        assert s not in _lib.SIGNATURES and s not in whole and not hasattr(lib, s), s


def _desc(p, **kw):
    f = dict(rowptr=p, col=p, colptr=p, t_col=p, perm=p, n=2, nnz=3, H=2, C=5, xl=p, ld_xl=10, el=p, er=p, attn_l=p, attn_r=p,
             keep=None, mult=None, src_scale=None, dst_scale=None, negative_slope=0.2)
    f.update(kw)
    return _lib.GatLayer(*[f[name] for name, _ in _lib.GatLayer._fields_])


def test_gat_layer_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    assert lib.egnn_gat_layer_bwd_ws_floats(2, 2, 5) == 20
    assert lib.egnn_gat_layer_bwd_ws_floats(-1, 2, 5) == 0

    def fwd(att=p, out=p, ld_out=10, **kw):
        return lib.egnn_gat_layer_fwd_f32(C.byref(_desc(p, **kw)), att, out, ld_out, None)

    def bwd(att=p, go=p, ld_go=10, mean_heads=0, d_raw=p, d_er=p, dxl=p, ld_dxl=10, d_attn=p, ws=p, nws=20, **kw):
        return lib.egnn_gat_layer_bwd_f32(C.byref(_desc(p, **kw)), att, go, ld_go, mean_heads, d_raw, d_er, dxl, ld_dxl, d_attn, ws, nws,
                                          None)

    assert lib.egnn_gat_layer_fwd_f32(None, p, p, 10, None) == EINVAL
    assert lib.egnn_gat_layer_bwd_f32(None, p, p, 10, 0, p, p, p, 10, p, p, 20, None) == EINVAL
    for bad in (dict(n=-1), dict(nnz=-1), dict(H=0), dict(H=65), dict(C=0), dict(ld_xl=9), dict(rowptr=None), dict(col=None),
                dict(xl=None), dict(el=None)):
        assert fwd(**bad) == EINVAL, bad
        assert bwd(**bad) == EINVAL, bad
    for bad in (dict(ld_out=9), dict(out=None), dict(att=None)):
        assert fwd(**bad) == EINVAL, bad
    for bad in (dict(ld_go=9), dict(ld_dxl=9), dict(attn_r=None), dict(er=None), dict(d_er=None), dict(nws=19), dict(ws=None),
                dict(colptr=None), dict(attn_l=None), dict(dxl=None), dict(perm=None), dict(t_col=None), dict(d_raw=None),
                dict(go=None), dict(att=None), dict(H=4, C=1024, ld_xl=4096, ld_go=4096, ld_dxl=4096, nws=1 << 20),
                dict(mean_heads=1, ld_go=4)):
        assert bwd(**bad) == EINVAL, bad
    assert fwd(n=0) == 0 and bwd(n=0) == 0                            # nothing to do, nothing launched


def test_arxiv_gat_loss_known_answers():
    eps = 1 - math.log(2)
    assert PM.ARXIV_GAT_EPSILON == eps
    x = torch.tensor([[2.0, 0.0, -1.0], [0.0, 0.0, 0.0], [-3.0, 4.0, 0.5]], dtype=torch.float64)
    labels = torch.tensor([[0], [2], [0]])
    ce = [-math.log(math.exp(r[l]) / sum(math.exp(v) for v in r)) for r, l in zip(x.tolist(), [0, 2, 0])]
    want = sum(math.log(eps + c) - math.log(eps) for c in ce) / 3
    assert float(PM.arxiv_gat_loss(x, labels)) == pytest.approx(want, rel=1e-12)
    # a perfect prediction costs nothing; the loss grows like log(CE) for bad ones
    sure = torch.tensor([[50.0, 0.0]], dtype=torch.float64)
    assert float(PM.arxiv_gat_loss(sure, torch.tensor([[0]]))) == pytest.approx(0.0, abs=1e-12)
    assert float(PM.arxiv_gat_loss(sure, torch.tensor([[1]]))) == pytest.approx(math.log(eps + 50.0) - math.log(eps), rel=1e-9)


def test_arxiv_gat_loss_matches_the_reference_golden():
    G = np.load(os.path.join(GOLDEN, "arxiv_gat_train.npz"), allow_pickle=False)
    tr, mask, labels = as_t(G["in_train"]), as_t(G["in_mask"]), as_t(G["in_labels"])
    lab_idx, pred_idx = PM.arxiv_gat_label_split(tr, 0.5, mask)
    assert torch.equal(lab_idx, tr[mask]) and torch.equal(pred_idx, tr[~mask])
    loss = PM.arxiv_gat_loss(as_t(G["model__pred"])[pred_idx], labels[pred_idx])
    assert float(loss) == pytest.approx(float(G["model__loss"]), rel=1e-5)


def test_label_split_and_add_labels():
    tr = torch.arange(10, 110)
    torch.manual_seed(4)
    a, b = PM.arxiv_gat_label_split(tr, 0.5)
    torch.manual_seed(4)
    m = torch.rand(tr.shape) < 0.5                                    # gat.py:122: one draw per train node
    assert torch.equal(a, tr[m]) and torch.equal(b, tr[~m]) and a.numel() + b.numel() == 100
    assert PM.arxiv_gat_label_split(tr, 0.0)[0].numel() == 0 and PM.arxiv_gat_label_split(tr, 1.0)[1].numel() == 0
    labels = torch.randint(0, 4, (120, 1))
    feat = PM.add_labels(torch.zeros(120, 3), labels, a, 4)
    assert feat.shape == (120, 7) and float(feat[:, 3:].sum()) == a.numel()
    assert bool((feat[a, 3:].argmax(1) == labels[a, 0]).all()) and float(feat[b, 3:].abs().sum()) == 0


def test_warm_up_is_linear_over_the_first_50_epochs():
    opt = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(1))], lr=0.002)
    seen = []
    for epoch in (1, 25, 50, 51, 200):
        PM.arxiv_gat_adjust_learning_rate(opt, 0.002, epoch)
        seen.append(opt.param_groups[0]["lr"])
    assert seen == pytest.approx([0.002 / 50, 0.001, 0.002, 0.002, 0.002])


def test_dgl_gat_conv_refuses_cpu_tensors_in_training_mode():
    import efficient_gnns_amd as E
    conv = E.nn.DGLGATConv(4, 3, num_heads=2, residual=True).train()
    adj = E.SparseTensor(row=torch.tensor([0, 1]), col=torch.tensor([0, 1]), sparse_sizes=(2, 2))
    with pytest.raises(_lib.HipExtensionError):
        conv(adj, torch.randn(2, 4))
