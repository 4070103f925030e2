"""Training the arxiv GAT teacher on the gfx950 kernels (nn.DGLGATConv / models.ArxivGAT in training mode, csrc/gat.hip: the fused
all-heads forward and the backward with row scales): layer gradients against the oracle (fp32 and a float64 restatement) and against
the golden recorded from the reference's own arxiv_dgl/models.py in training mode, the edge-drop and attention-dropout semantics,
bit-equal repeated passes, one full training step (arxiv_dgl/gat.py:116-148) against the golden, and the inference side unchanged."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import efficient_gnns_amd as E
import efficient_gnns_amd.data as D
import efficient_gnns_amd.models as PM
import efficient_gnns_amd.nn as PN
import efficient_gnns_amd.ops_edge as OE
import oracle.nn as ON
import oracle.sparse as OS
from conftest import GOLDEN, as_t
from test_gpu_parity import close

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN + "/arxiv_gat_train.npz", allow_pickle=False)


def message_graph(n=420, avg_deg=5, seed=0, isolated=None):
    """(dst, src) of a bidirected graph with exactly one self loop per node, grouped by target (CSR order): target 3 is a hub with
    > 256 entries, target 5 has 65-256.  ``isolated``: a node without any entry (zero in-degree and out-degree)."""
    g = torch.Generator().manual_seed(seed)
    e = n * avg_deg // 2
    a, b = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    a = torch.cat([a, torch.full((300,), 3), torch.full((100,), 5)])
    b = torch.cat([b, torch.randperm(n, generator=g)[:300], torch.randperm(n, generator=g)[:100]])
    m = torch.zeros(n, n, dtype=torch.bool)
    m[a, b] = True
    m = m | m.t()
    m.fill_diagonal_(True)
    if isolated is not None:
        m[isolated, :] = False
        m[:, isolated] = False
    dst, src = torch.nonzero(m, as_tuple=True)
    return dst, src


def adj_pair(dst, src, n):
    return (OS.SparseTensor(row=dst, col=src, sparse_sizes=(n, n)),
            E.SparseTensor(row=dst.to(DEV), col=src.to(DEV), sparse_sizes=(n, n)))


def composite64(feat, P, dst, src, n, H, C, sym, slope=0.2, keep=None, mult=None):
    """The layer (arxiv_dgl/models.py:154-236) restated in float64 with torch autograd on the edge list: the float64 bar.  ``keep``
    bool [E]: the kept edges (softmax over those, 0 elsewhere); ``mult`` [H, E]: the attention-dropout multiplier."""
    feat_src = (feat @ P["fc.weight"].t()).view(n, H, C)
    feat_dst = feat_src
    if sym:
        out_deg = torch.bincount(src, minlength=n).double().clamp(min=1)
        feat_src = feat_src * out_deg.pow(-0.5).view(n, 1, 1)
    e = (feat_src * P["attn_l"]).sum(-1)[src]
    if "attn_r" in P:
        e = e + (feat_dst * P["attn_r"]).sum(-1)[dst]
    e = F.leaky_relu(e, slope)
    sel = torch.arange(src.numel()) if keep is None else torch.nonzero(keep).view(-1)
    d_s, e_s = dst[sel], e[sel]
    mx = torch.full((n, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, d_s[:, None].expand(-1, H), e_s, "amax")
    ex = torch.exp(e_s - mx[d_s])
    att_s = ex / torch.zeros(n, H, dtype=e.dtype).index_add(0, d_s, ex)[d_s]
    att = torch.zeros(src.numel(), H, dtype=e.dtype).index_add(0, sel, att_s)
    a = att if mult is None else att * mult.t()
    rst = torch.zeros(n, H, C, dtype=e.dtype).index_add(0, dst, feat_src[src] * a[..., None])
    if sym:
        rst = rst * torch.bincount(dst, minlength=n).double().clamp(min=1).pow(0.5).view(n, 1, 1)
    if "res_fc.weight" in P:
        rst = rst + (feat @ P["res_fc.weight"].t()).view(n, H, C)
    return rst, att


def run_layer(conv, adj, x, w):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    out = conv(adj, x)
    (out * w).sum().backward()
    return out.detach(), x.grad, {k: p.grad for k, p in conv.named_parameters()}


def run_composite(sd, x, w, dst, src, n, H, C, sym, **kw):
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items() if v is not None}
    xr = x.detach().cpu().double().requires_grad_(True)
    out, att = composite64(xr, P, dst, src, n, H, C, sym, **kw)
    (out * w.detach().cpu().double()).sum().backward()
    return out.detach(), xr.grad, {k: v.grad for k, v in P.items()}, att.detach()


def check_against(got, ref, tag, rtol=1e-4, atol_scale=1e-4):
    close(got[0], ref[0], rtol=rtol, atol_scale=atol_scale, msg=f"{tag}: out")
    close(got[1], ref[1], rtol=rtol, atol_scale=atol_scale, msg=f"{tag}: d feat")
    assert set(got[2]) == set(ref[2])
    for k in got[2]:
        close(got[2][k], ref[2][k], rtol=rtol, atol_scale=atol_scale, msg=f"{tag}: d {k}")


def layer_pair(F_in, H, C, attn_dst, sym, seed=1, **kw):
    torch.manual_seed(seed)
    oc = ON.DGLGATConv(F_in, C, num_heads=H, use_attn_dst=attn_dst, use_symmetric_norm=sym, residual=True, **kw)
    pc = PN.DGLGATConv(F_in, C, num_heads=H, use_attn_dst=attn_dst, use_symmetric_norm=sym, residual=True, **kw).to(DEV)
    pc.load_state_dict(oc.state_dict())
    return oc.train(), pc.train()


# ------------------------------------------------------------------------------------------------
# 1. layer gradients vs the oracle (fp32) and a float64 restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", [(3, 250), (1, 40)])
@pytest.mark.parametrize("attn_dst", [False, True], ids=["noattn", "attn"])
@pytest.mark.parametrize("sym", [False, True], ids=["plain", "norm"])
def test_layer_gradients_match_oracle(H, C, attn_dst, sym):
    n, F_in = 420, 24
    dst, src = message_graph(n)
    deg = torch.bincount(dst, minlength=n)
    assert deg.max() > 256 and ((deg > 64) & (deg <= 256)).any()
    oadj, padj = adj_pair(dst, src, n)
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(n, F_in, generator=g), torch.randn(n, H, C, generator=g)
    oc, pc = layer_pair(F_in, H, C, attn_dst, sym)
    got = run_layer(pc, padj, x.to(DEV), w.to(DEV))
    ref32 = run_layer(oc, oadj, x, w)
    ref64 = run_composite(dict(oc.named_parameters()), x, w, dst, src, n, H, C, sym)
    close(got[0], ref32[0], rtol=1e-4, atol_scale=1e-4, msg="out vs fp32 oracle")
    check_against(ref32, ref64[:3], "fp32 oracle vs float64 restatement")     # the restatement states the same layer
    check_against(got, ref64[:3], "vs float64")


def test_layer_gradients_with_an_isolated_node():
    n, F_in, H, C = 300, 16, 3, 250
    dst, src = message_graph(n, seed=4, isolated=11)
    assert int((dst == 11).sum()) == 0 and int((src == 11).sum()) == 0
    oadj, padj = adj_pair(dst, src, n)
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(n, F_in, generator=g), torch.randn(n, H, C, generator=g)
    oc, pc = layer_pair(F_in, H, C, True, True, allow_zero_in_degree=True)
    got = run_layer(pc, padj, x.to(DEV), w.to(DEV))
    ref32 = run_layer(oc, oadj, x, w)
    ref64 = run_composite(dict(oc.named_parameters()), x, w, dst, src, n, H, C, True)
    close(got[0], ref32[0], rtol=1e-4, atol_scale=1e-4, msg="out vs fp32 oracle")
    check_against(got, ref64[:3], "vs float64")
    _, strict = layer_pair(F_in, H, C, True, True)
    with pytest.raises(AssertionError):
        strict(padj, x.to(DEV))


# ------------------------------------------------------------------------------------------------
# 2. the reference's own training-mode layer and training step (tests/golden/arxiv_gat_train.npz)
# ------------------------------------------------------------------------------------------------
class _Injected(PN.DGLGATConv):
    """DGLGATConv whose edge_drop draws come from a recorded list of kept-entry masks (in call order)."""
    recorded = None

    def _draw_edge_keep(self, nnz, device):
        keep = self.recorded.pop(0)
        assert keep.numel() == nnz
        return keep.to(device)


def golden_graph(G):
    dst, src = as_t(G["in_dst"]), as_t(G["in_src"])
    n = G["in_x"].shape[0]
    adj = E.SparseTensor(row=dst.to(DEV), col=src.to(DEV), sparse_sizes=(n, n))
    rowptr, col, _ = adj.csr()
    rows = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).cpu())
    assert torch.equal(rows, dst) and torch.equal(col.cpu(), src)           # recorded in CSR order: an edge id is a CSR entry
    return adj, dst, src, n


@pytest.mark.parametrize("attn_dst", [False, True], ids=["noattn", "attn"])
@pytest.mark.parametrize("sym", [False, True], ids=["plain", "norm"])
def test_layer_matches_reference_golden_with_the_recorded_edge_subset(golden, attn_dst, sym):
    G = golden
    name = f"layer_{'attn' if attn_dst else 'noattn'}_{'norm' if sym else 'plain'}"
    adj, dst, src, n = golden_graph(G)
    x, w = as_t(G["in_x"], DEV), as_t(G["layer_w"], DEV)
    H, C = w.shape[1], w.shape[2]
    conv = _Injected(x.shape[1], C, num_heads=H, edge_drop=float(G["edge_drop"]), use_attn_dst=attn_dst, use_symmetric_norm=sym,
                     residual=True).to(DEV).train()
    pre = f"{name}__param__"
    conv.load_state_dict({k[len(pre):]: as_t(G[k], DEV) for k in G.files if k.startswith(pre)}, strict=True)
    keep = as_t(G[f"{name}__keep"])
    assert int(keep.sum()) == keep.numel() - int(keep.numel() * float(G["edge_drop"]))
    conv.recorded = [keep]
    out, gx, gp = run_layer(conv, adj, x, w)
    close(out, G[f"{name}__out"], rtol=1e-4, atol_scale=1e-4, msg="out")
    close(gx, G[f"{name}__d_x"], rtol=1e-4, atol_scale=1e-4, msg="d feat")
    pre = f"{name}__grad__"
    assert {k[len(pre):] for k in G.files if k.startswith(pre)} == set(gp)
    for k, v in gp.items():
        close(v, G[pre + k], rtol=1e-4, atol_scale=1e-4, msg=f"d {k}")


def test_training_step_matches_reference_golden(golden, monkeypatch):
    """One step of gat.py:116-148 (--use-norm --no-attn-dst --use-labels --n-label-iters=1, RMSprop lr 0.002) with the recorded
    label mask and kept-edge sets: loss, every parameter gradient, the state after the optimizer step."""
    G = golden
    adj, dst, src, n = golden_graph(G)
    x, labels = as_t(G["in_x"], DEV), as_t(G["in_labels"], DEV)
    tr, va, te = (as_t(G[k], DEV) for k in ("in_train", "in_val", "in_test"))
    C = 6
    monkeypatch.setattr(PM, "DGLGATConv", _Injected)
    model = PM.ArxivGAT(x.shape[1] + C, C, 5, 3, 3, F.relu, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=float(G["edge_drop"]),
                        use_attn_dst=False, use_symmetric_norm=True).to(DEV)
    pre = "model__init__"
    model.load_state_dict({k[len(pre):]: as_t(G[k], DEV) for k in G.files if k.startswith(pre)}, strict=True)
    keeps = [as_t(k) for k in G["model__keep"]]
    assert len(keeps) == 6
    shared = list(keeps)
    for conv in model.convs:
        conv.recorded = shared                                               # one list: the layers draw in call order
    opt = torch.optim.RMSprop(model.parameters(), lr=0.002, weight_decay=0)
    acc, loss = PM.arxiv_gat_train_step(model, adj, x, labels, tr, va, te, opt, C, use_labels=True, n_label_iters=1, mask_rate=0.5,
                                        mask=as_t(G["in_mask"]))
    assert not shared and 0.0 <= acc <= 1.0
    close(loss, float(G["model__loss"]), rtol=2e-4, atol_scale=0, msg="loss")
    for k, p in model.named_parameters():
        close(p.grad, G[f"model__grad__{k}"], rtol=2e-4, atol_scale=2e-4, msg=f"d {k}")
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(G[f"model__final__{k}"])
            continue
        close(v, G[f"model__final__{k}"], rtol=2e-4, atol_scale=2e-4, msg=f"after the step: {k}")


# ------------------------------------------------------------------------------------------------
# 3. edge-drop semantics
# ------------------------------------------------------------------------------------------------
def test_edge_drop_draw_and_attention_over_the_kept_entries():
    n, F_in, H, C, p = 420, 24, 3, 250, 0.3
    dst, src = message_graph(n, seed=6)
    _, padj = adj_pair(dst, src, n)
    nnz = padj.nnz()
    _, pc = layer_pair(F_in, H, C, False, True, edge_drop=p)
    torch.manual_seed(0)
    k1, k2 = pc._draw_edge_keep(nnz, DEV), pc._draw_edge_keep(nnz, DEV)
    assert k1.dtype == torch.bool and int(k1.sum()) == int(k2.sum()) == nnz - int(nnz * p) and not torch.equal(k1, k2)
    # the kernel's coefficients on a set that leaves one row (target 7) without any kept entry
    keep = k1.clone()
    rowptr, col, _ = padj.csr()
    keep[int(rowptr[7]):int(rowptr[8])] = False
    g = torch.Generator().manual_seed(7)
    xl = torch.randn(n, H * C, generator=g).to(DEV)
    in_sqrt, out_rsqrt, _ = pc._degrees(padj)
    out, att, _, _ = OE.dgl_gat_layer_forward(xl, pc.attn_l.detach(), None, padj, H, C, 0.2, keep.to(torch.uint8), None,
                                              out_rsqrt.reshape(n).contiguous(), in_sqrt.reshape(n).contiguous())
    assert att.shape == (H, nnz) and bool((att[:, ~keep] == 0).all()) and bool((att[:, keep] > 0).all())
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), rowptr[1:] - rowptr[:-1])
    tot = torch.zeros(H, n, dtype=torch.float64, device=DEV).index_add_(1, rows, att.double())
    has = torch.zeros(n, dtype=torch.bool, device=DEV)
    has[rows[keep]] = True
    assert not bool(has[7]) and int(has.sum()) >= n - 20
    assert float((tot[:, has] - 1).abs().max()) < 1e-5 and bool((tot[:, ~has] == 0).all())
    assert bool((out.view(n, H, C)[~has] == 0).all())


def test_a_row_whose_entries_are_all_dropped_yields_the_residual_alone():
    n, F_in, H, C = 300, 16, 3, 250
    dst, src = message_graph(n, seed=8)
    _, padj = adj_pair(dst, src, n)
    rowptr = padj.csr()[0]
    keep = torch.rand(padj.nnz(), generator=torch.Generator().manual_seed(9)) >= 0.3
    keep[int(rowptr[3]):int(rowptr[4])] = False                              # the hub row
    keep[int(rowptr[20]):int(rowptr[21])] = False
    torch.manual_seed(1)
    pc = _Injected(F_in, C, num_heads=H, edge_drop=0.3, use_attn_dst=True, use_symmetric_norm=True, residual=True).to(DEV).train()
    pc.recorded = [keep]
    g = torch.Generator().manual_seed(10)
    x, w = torch.randn(n, F_in, generator=g).to(DEV), torch.randn(n, H, C, generator=g).to(DEV)
    out, gx, gp = run_layer(pc, padj, x, w)
    res = (x @ pc.res_fc.weight.detach().t()).view(n, H, C)
    close(out[[3, 20]], res[[3, 20]], rtol=1e-4, atol_scale=1e-4, msg="residual alone")
    assert bool(torch.isfinite(gx).all()) and all(bool(torch.isfinite(v).all()) for v in gp.values())
    ref = run_composite(dict(pc.named_parameters()), x, w, dst, src, n, H, C, True, keep=keep)
    check_against((out, gx, gp), ref[:3], "vs float64")


# ------------------------------------------------------------------------------------------------
# 4. attention dropout with an injected multiplier (plus an edge subset), vs the float64 restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C,attn_dst,sym", [(3, 250, False, True), (2, 36, True, True), (3, 7, True, False)])
def test_attention_dropout_and_edge_drop_gradients_vs_float64(H, C, attn_dst, sym):
    n, F_in, p = 420, 24, 0.5
    dst, src = message_graph(n, seed=12)
    _, padj = adj_pair(dst, src, n)
    nnz = padj.nnz()
    g = torch.Generator().manual_seed(13)
    keep = torch.rand(nnz, generator=g) >= 0.3
    mult = (torch.rand(H, nnz, generator=g) >= p).float() / (1 - p)
    _, pc = layer_pair(F_in, H, C, attn_dst, sym)
    xl = torch.randn(n, H * C, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(n, H, C, generator=g)
    in_sqrt, out_rsqrt, _ = pc._degrees(padj)
    for q in pc.parameters():
        q.grad = None
    out = OE.dgl_gat_attention(xl, pc.attn_l, pc.attn_r, padj, H, 0.2, keep=keep.to(DEV), mult=mult.to(DEV),
                               src_scale=out_rsqrt if sym else None, dst_scale=in_sqrt if sym else None)
    (out * w.to(DEV)).sum().backward()
    # float64: the same layer with fc = identity and no residual
    P = {"fc.weight": torch.eye(H * C, dtype=torch.float64), "attn_l": pc.attn_l.detach().cpu().double().requires_grad_(True)}
    if attn_dst:
        P["attn_r"] = pc.attn_r.detach().cpu().double().requires_grad_(True)
    xr = xl.detach().cpu().double().requires_grad_(True)
    ref, _ = composite64(xr, P, dst, src, n, H, C, sym, keep=keep, mult=mult.double())
    (ref * w.double()).sum().backward()
    close(out, ref, rtol=1e-4, atol_scale=1e-4, msg="out")
    close(xl.grad, xr.grad, rtol=1e-4, atol_scale=1e-4, msg="d xl")
    close(pc.attn_l.grad, P["attn_l"].grad, rtol=1e-4, atol_scale=1e-4, msg="d attn_l")
    if attn_dst:
        close(pc.attn_r.grad, P["attn_r"].grad, rtol=1e-4, atol_scale=1e-4, msg="d attn_r")


def test_module_attention_dropout_draws_one_multiplier_per_call():
    n, F_in, H, C, p = 300, 16, 3, 250, 0.5
    dst, src = message_graph(n, seed=14)
    _, padj = adj_pair(dst, src, n)
    _, pc = layer_pair(F_in, H, C, False, True, attn_drop=p)
    g = torch.Generator().manual_seed(15)
    x, w = torch.randn(n, F_in, generator=g).to(DEV), torch.randn(n, H, C, generator=g).to(DEV)
    torch.manual_seed(123)
    got = run_layer(pc, padj, x, w)
    torch.manual_seed(123)                                                   # the layer's one [H, nnz] draw
    mult = ((torch.rand(H, padj.nnz(), device=DEV) >= p).double() / (1 - p)).cpu()
    ref = run_composite(dict(pc.named_parameters()), x, w, dst, src, n, H, C, True, mult=mult)
    check_against(got, ref[:3], "vs float64")


# ------------------------------------------------------------------------------------------------
# 5. determinism
# ------------------------------------------------------------------------------------------------
def test_forward_and_backward_are_bit_equal_across_passes():
    n, F_in, H, C = 420, 64, 3, 250
    dst, src = message_graph(n, seed=16)
    _, padj = adj_pair(dst, src, n)
    g = torch.Generator().manual_seed(17)
    keep = torch.rand(padj.nnz(), generator=g) >= 0.3
    torch.manual_seed(2)
    pc = _Injected(F_in, C, num_heads=H, edge_drop=0.3, use_attn_dst=True, use_symmetric_norm=True, residual=True).to(DEV).train()
    x, w = torch.randn(n, F_in, generator=g).to(DEV), torch.randn(n, H, C, generator=g).to(DEV)
    pc.recorded = [keep, keep]
    a = run_layer(pc, padj, x, w)
    b = run_layer(pc, padj, x, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


# ------------------------------------------------------------------------------------------------
# 6. the inference side is what it was; a short training run
# ------------------------------------------------------------------------------------------------
def test_eval_mode_with_gradients_still_raises():
    n = 420
    dst, src = message_graph(n, seed=18)
    _, padj = adj_pair(dst, src, n)
    _, pc = layer_pair(8, 2, 6, True, True)
    pc.eval()
    with pytest.raises(NotImplementedError):
        pc(padj, torch.randn(n, 8, device=DEV))
    with torch.no_grad():
        assert pc(padj, torch.randn(n, 8, device=DEV)).shape == (n, 2, 6)


def test_short_training_run_loss_decreases_and_artifacts(tmp_path):
    from efficient_gnns_amd.utils import dgl_bidirected_with_self_loops
    d = D.arxiv_like(scale=0.02, seed=9, with_teacher=False)
    n, C = d.num_nodes, d.num_classes
    adj = dgl_bidirected_with_self_loops(d.adj_t.to(DEV))
    x, y = d.x.to(DEV), d.y.to(DEV)
    tr, va, te = (d.split_idx[k].to(DEV) for k in ("train", "valid", "test"))
    torch.manual_seed(0)
    model = PM.ArxivGAT(d.num_features + C, C, 250, 3, 3, F.relu, dropout=0.75, input_drop=0.25, attn_drop=0.0, edge_drop=0.3,
                        use_attn_dst=False, use_symmetric_norm=True).to(DEV)
    before_sd = copy.deepcopy(model.state_dict())
    frozen = copy.deepcopy(model)
    pred0, feat0 = PM.teacher_evaluate(model, adj, x, y, tr, va, te, C, True, 1)
    lr = 0.002
    opt = torch.optim.RMSprop(model.parameters(), lr=lr, weight_decay=0)
    losses = []
    for epoch in range(1, 31):
        PM.arxiv_gat_adjust_learning_rate(opt, lr, epoch)
        assert opt.param_groups[0]["lr"] == pytest.approx(lr * epoch / 50)
        _, loss = PM.arxiv_gat_train_step(model, adj, x, y, tr, va, te, opt, C, use_labels=True, n_label_iters=1, mask_rate=0.5)
        assert np.isfinite(loss)
        losses.append(loss)
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    # the eval-mode forward is the inference forward it was: the trained weights in a fresh module give the same bits, and a
    # copy made before the training still gives the first prediction
    pred1, feat1 = PM.teacher_evaluate(model, adj, x, y, tr, va, te, C, True, 1)
    assert not model.training and pred1.shape == (n, C) and feat1.shape == (n, 750) and bool(torch.isfinite(pred1).all())
    assert any(not torch.equal(v, before_sd[k]) for k, v in model.state_dict().items())
    fresh = PM.ArxivGAT(d.num_features + C, C, 250, 3, 3, F.relu, dropout=0.75, input_drop=0.25, attn_drop=0.0, edge_drop=0.3,
                        use_attn_dst=False, use_symmetric_norm=True).to(DEV)
    fresh.load_state_dict(model.state_dict())
    pred2, feat2 = PM.teacher_evaluate(fresh, adj, x, y, tr, va, te, C, True, 1)
    assert torch.equal(pred1, pred2) and torch.equal(feat1, feat2)
    pred3, feat3 = PM.teacher_evaluate(frozen, adj, x, y, tr, va, te, C, True, 1)
    assert torch.equal(pred0, pred3) and torch.equal(feat0, feat3)
    D.save_teacher_artifacts(str(tmp_path), "gat-3L250x3h", 0, feat1, pred1)
    f2, l2 = D.load_teacher_artifacts(str(tmp_path), "gat-3L250x3h", 0, num_nodes=n, device=DEV)
    assert torch.equal(f2, feat1) and torch.equal(l2, pred1)
