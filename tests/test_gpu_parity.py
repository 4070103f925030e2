"""GPU parity tests (run with ``-m gpu`` on an MI355X): the HIP path, called through the C ABI via the
product package, against the CPU oracle and the golden vectors.

Bars: integer / index results bit-exact; fp32 layer outputs rtol 1e-5 with
atol = 1e-5 * max|ref|; scalar losses rtol 1e-5 (NCE 2e-5); gradients rtol 1e-4.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import efficient_gnns_amd as E
import efficient_gnns_amd.data as D
import efficient_gnns_amd.criterion as PC
import efficient_gnns_amd.models as PM
import efficient_gnns_amd.ops as ops
from efficient_gnns_amd import _lib
import oracle.criterion as OC
import oracle.models as OM
import oracle.nn as ON
import oracle.sparse as OS
import oracle.utils as OU
from conftest import ARXIV_GAT_CONFIGS, arxiv_gat_case, as_t, mag_rgcn_case, ppi_train_case
from test_oracle_golden import criterion_cases, run_training, noise_driven, parse_run

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(actual, ref, rtol=1e-5, atol_scale=1e-5, msg=""):
    a = actual.detach().cpu().double().numpy() if torch.is_tensor(actual) else np.asarray(actual, dtype=np.float64)
    r = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    atol = atol_scale * (np.abs(r).max() if r.size else 0.0) + 1e-30
    np.testing.assert_allclose(a, r, rtol=rtol, atol=atol, err_msg=msg)


def random_csr(n_rows, n_cols, avg_deg, seed, hubs=(), empty_frac=0.1, dup=False):
    """COO (row, col) with empty rows, optional hub rows (very long) and optional duplicate entries."""
    g = torch.Generator().manual_seed(seed)
    e = int(n_rows * avg_deg)
    row = torch.randint(0, n_rows, (e,), generator=g)
    col = torch.randint(0, n_cols, (e,), generator=g)
    for h, deg in hubs:
        row = torch.cat([row, torch.full((deg,), h)])
        col = torch.cat([col, torch.randint(0, n_cols, (deg,), generator=g)])
    keep = torch.rand(n_rows, generator=g) >= empty_frac
    for h, _ in hubs:
        keep[h] = True
    m = keep[row]
    row, col = row[m], col[m]
    if not dup:
        key = torch.unique(row * n_cols + col)
        row, col = key // n_cols, key % n_cols
    return row, col


def make_pair(row, col, val, sizes):
    o = OS.SparseTensor(row=row, col=col, value=val, sparse_sizes=sizes)
    p = E.SparseTensor(row=row.to(DEV), col=col.to(DEV), value=None if val is None else val.to(DEV), sparse_sizes=sizes)
    return o, p


# ------------------------------------------------------------------------------------------------
# structure (bit-exact)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,e,seed", [(1, 0, 0), (9, 0, 1), (40, 300, 2), (3000, 40000, 3)])
def test_structure_on_device_bit_exact(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
    o = OS.to_sparse_tensor(ei, n)
    p = E.to_sparse_tensor(ei.to(DEV), n)
    for a, b in zip(p.csr()[:2], o.csr()[:2]):
        assert torch.equal(a.cpu(), b)
    so, sp = o.to_symmetric(), p.to_symmetric()
    for a, b in zip(sp.csr()[:2], so.csr()[:2]):
        assert torch.equal(a.cpu(), b)
    assert torch.equal(sp.storage.colptr().cpu(), so._colptr())
    assert torch.equal(sp.storage.csr2csc().cpu(), so._csr2csc())
    # host-built tensor moved to the GPU gives the same arrays
    moved = E.to_sparse_tensor(ei, n).to_symmetric().to(DEV)
    assert torch.equal(moved.csr()[1], sp.csr()[1]) and torch.equal(moved.csr()[0], sp.csr()[0])
    # gcn_norm: structure bit-exact (diagonal inserted in sorted position), values fp32-close
    go, gp = OS.gcn_norm_sparse(so), E.gcn_norm(sp)
    assert torch.equal(gp.csr()[0].cpu(), go.csr()[0]) and torch.equal(gp.csr()[1].cpu(), go.csr()[1])
    close(gp.csr()[2], go.csr()[2], rtol=2e-6, atol_scale=0)
    # int32 narrowing round-trips
    rp32, c32, bits = sp._index_arrays()
    assert bits == 32 and torch.equal(rp32.long(), sp.csr()[0]) and torch.equal(c32.long(), sp.csr()[1])


def test_gcn_norm_replaces_existing_diagonal_and_duplicates():
    row = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 3])
    col = torch.tensor([0, 0, 2, 0, 1, 1, 2, 3, 0])  # duplicate diagonal in row 0
    o, p = make_pair(row, col, None, (4, 4))
    go, gp = OS.gcn_norm_sparse(o), E.gcn_norm(p)
    assert torch.equal(gp.csr()[0].cpu(), go.csr()[0]) and torch.equal(gp.csr()[1].cpu(), go.csr()[1])
    close(gp.csr()[2], go.csr()[2], rtol=2e-6, atol_scale=0)


def test_subgraph_and_edge_index_norm_on_device():
    n = 500
    g = torch.Generator().manual_seed(0)
    ei = torch.stack([torch.randint(0, n, (4000,), generator=g), torch.randint(0, n, (4000,), generator=g)])
    subset = torch.randperm(n, generator=g)[:200]
    a = E.subgraph(subset.to(DEV), ei.to(DEV), relabel_nodes=True, num_nodes=n)[0]
    b = OU.subgraph(subset, ei, relabel_nodes=True, num_nodes=n)[0]
    assert torch.equal(a.cpu(), b)


# ------------------------------------------------------------------------------------------------
# SpMM
# ------------------------------------------------------------------------------------------------
SPMM_K = [1, 3, 4, 40, 50, 64, 121, 128, 256, 300]


@pytest.mark.parametrize("K", SPMM_K)
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_forward_backward_vs_oracle(K, reduce):
    n_rows, n_cols = 700, 650
    row, col = random_csr(n_rows, n_cols, 9, seed=K, hubs=((5, 1400), (699, 600)), dup=(K % 2 == 0))
    g = torch.Generator().manual_seed(K + 1)
    val = torch.rand(row.numel(), generator=g) + 0.1 if reduce != "mean" and K % 3 != 0 else None
    o, p = make_pair(row, col, val, (n_rows, n_cols))
    x = torch.randn(n_cols, K, generator=g)
    gy = torch.randn(n_rows, K, generator=g)
    xo = x.clone().requires_grad_(True)
    xp = x.to(DEV).requires_grad_(True)
    yo = o.matmul(xo, reduce)
    yp = p.matmul(xp, reduce)
    close(yp, yo, msg=f"fwd K={K} {reduce}")
    yo.backward(gy)
    yp.backward(gy.to(DEV))
    close(xp.grad, xo.grad, rtol=1e-4, msg=f"bwd K={K} {reduce}")


@pytest.mark.parametrize("K", [4, 33, 128])
def test_spmm_max_argmax_bit_exact_with_ties(K):
    n_rows, n_cols = 300, 280
    row, col = random_csr(n_rows, n_cols, 12, seed=11, hubs=((7, 900),), dup=True)
    o, p = make_pair(row, col, None, (n_rows, n_cols))
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (n_cols, K), generator=g).float()  # small integers => many exact ties
    yo, ao = OS.matmul_max_with_arg(o, x)
    yp, ap = ops.spmm_raw(p, x.to(DEV), "max")
    assert torch.equal(yp.cpu(), yo)
    assert torch.equal(ap.cpu(), ao), "argmax must be the first maximal stored entry"


def test_spmm_int64_path_and_no_long_row_list_agree():
    n = 400
    row, col = random_csr(n, n, 10, seed=5, hubs=((3, 1500),))
    o, p = make_pair(row, col, None, (n, n))
    x = torch.randn(n, 96)
    ref = o.matmul(x, "sum")
    p._struct["idx"] = (p._rowptr, p._col, 64)  # force the int64 kernels
    y64, _ = ops.spmm_raw(p, x.to(DEV), "sum")
    close(y64, ref)
    y_nolong, _ = ops.spmm_raw(p, x.to(DEV), "sum", use_plan=False)
    close(y_nolong, ref)


def test_spmm_deterministic_and_strided_input():
    n = 2000
    row, col = random_csr(n, n, 14, seed=8, hubs=((0, 3000),))
    o, p = make_pair(row, col, torch.rand(row.numel()), (n, n))
    big = torch.randn(n, 320, device=DEV)
    x = big[:, 32:288]  # ld = 320, 16-byte aligned view
    y1, _ = ops.spmm_raw(p, x, "sum")
    y2, _ = ops.spmm_raw(p, x, "sum")
    assert torch.equal(y1, y2), "fixed summation order => run-to-run bit-stable"
    close(y1, o.matmul(x.cpu().contiguous(), "sum"))
    x_odd = big[:, 1:257]  # misaligned view must take the scalar path and still be right
    y3, _ = ops.spmm_raw(p, x_odd, "sum")
    close(y3, o.matmul(x_odd.cpu().contiguous(), "sum"))


def test_spmm_rectangular_mag_style_mean():
    n_dst, n_src = 900, 400
    row, col = random_csr(n_dst, n_src, 6, seed=21)
    o, p = make_pair(row, col, None, (n_dst, n_src))
    x = torch.randn(n_src, 128)
    close(p.matmul(x.to(DEV), reduce="mean"), o.matmul(x, reduce="mean"))


@pytest.mark.parametrize("schedule", ["blocks", "segments", "classes"])
@pytest.mark.parametrize("K", [64, 100, 128, 256])
def test_spmm_schedules_agree_with_oracle(schedule, K, monkeypatch):
    """The three schedules of the aggregation (row blocks + hub segments in one launch = the default; round-1 segments;
    row classes) on a graph with empty rows, duplicates and hubs, values / src-scale / bias / mean."""
    monkeypatch.setattr(ops, "_SPMM_SCHEDULE", schedule)
    n = 1500
    row, col = random_csr(n, n, 11, seed=K, hubs=((2, 2100), (1499, 700), (640, 65)), dup=True)
    g = torch.Generator().manual_seed(K)
    val = torch.rand(row.numel(), generator=g) + 0.1
    o, p = make_pair(row, col, val, (n, n))
    x = torch.randn(n, K, generator=g)
    bias = torch.randn(K, generator=g)
    for reduce in ("sum", "mean"):
        y, _ = ops.spmm_raw(p, x.to(DEV), reduce, bias=bias.to(DEV))
        close(y, o.matmul(x, reduce) + bias, msg=f"{schedule} K={K} {reduce}")
    scale = torch.rand(n, generator=g) + 0.5
    y, _ = ops.spmm_raw(p, x.to(DEV), "sum", src_scale=scale.to(DEV))
    close(y, o.matmul(x * scale[:, None], "sum"), msg=f"{schedule} src_scale")
    y1, _ = ops.spmm_raw(p, x.to(DEV), "sum")
    y2, _ = ops.spmm_raw(p, x.to(DEV), "sum")
    assert torch.equal(y1, y2), "fixed summation order => run-to-run bit-stable"
    add = torch.randn(n, K, generator=g)
    ya, _ = ops.spmm_raw(p, x.to(DEV), "mean", bias=bias.to(DEV), addend=add.to(DEV))     # Y = A X + bias + addend (hub rows included)
    close(ya, o.matmul(x, "mean") + bias + add, msg=f"{schedule} addend")


@pytest.mark.parametrize("K,reduce", [(256, "sum"), (64, "mean"), (128, "sum")])
def test_spmm_epilogue_statistics_match_a_pass_over_the_result(K, reduce):
    """BatchNorm statistics formed in the aggregation's epilogue (arxiv_pyg/gnn.py:47-48): column mean / biased variance of
    ALL rows of Y (block rows + hub rows) against torch on the result, for few and for many (> 128) row blocks."""
    for n in (900, 40000):   # 40000 rows: 5000 wave partials, the two-launch fold of egnn_bn_stats_merge_f32
        row, col = random_csr(n, n, 9, seed=n + K, hubs=((1, 1300), (n - 1, 300)))
        g = torch.Generator().manual_seed(K)
        val = torch.rand(row.numel(), generator=g) + 0.1 if reduce == "sum" else None
        o, p = make_pair(row, col, val, (n, n))
        x = torch.randn(n, K, generator=g) + 0.7
        bias = torch.randn(K, generator=g)
        shift = (torch.randn(K, generator=g) * 0.1).to(DEV)
        y, _, (mean, var) = ops.spmm_raw(p, x.to(DEV), reduce, bias=bias.to(DEV), stat_shift=shift, want_stats=True)
        y_plain, _ = ops.spmm_raw(p, x.to(DEV), reduce, bias=bias.to(DEV))
        assert torch.equal(y, y_plain), "the statistics epilogue must not change the result"
        close(mean, y.double().mean(0), rtol=1e-5)
        close(var, y.double().var(0, unbiased=False), rtol=2e-5)
        y2, _, (mean2, var2) = ops.spmm_raw(p, x.to(DEV), reduce, bias=bias.to(DEV), stat_shift=None, want_stats=True)
        close(mean2, y.double().mean(0), rtol=1e-5)
        close(var2, y.double().var(0, unbiased=False), rtol=1e-4)
        assert torch.equal(ops.spmm_raw(p, x.to(DEV), reduce, bias=bias.to(DEV), want_stats=True)[2][0], mean2), "deterministic"


def test_gcn_layer_with_epilogue_statistics_trains_like_the_separate_pass(monkeypatch):
    """GCN.forward hands BatchNorm the statistics of the aggregation epilogue: same losses / gradients as with the
    separate egnn_bn_stats_f32 pass (within fp32 rounding of the two summation orders)."""
    d = D.arxiv_like(scale=0.02, seed=4)
    dev_args = (d.x.to(DEV), d.adj_t.to(DEV))
    torch.manual_seed(0)
    m1 = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.0).to(DEV)
    m2 = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.0).to(DEV)
    m2.load_state_dict(m1.state_dict())
    m1.train(), m2.train()
    out1 = m1(*dev_args)
    monkeypatch.setattr(ops, "_SPMM_SCHEDULE", "segments")   # no statistics epilogue there: bn_act runs its own pass
    out2 = m2(*dev_args)
    close(out1, out2, rtol=1e-5)
    close(m1.bns[1].running_var, m2.bns[1].running_var, rtol=1e-5)
    out1.square().mean().backward()
    out2.square().mean().backward()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        if k in ("convs.0.bias", "convs.1.bias"):
            continue   # a bias in front of BatchNorm has a mathematically zero gradient: what is left is rounding noise
        close(a.grad, b.grad, rtol=1e-4, atol_scale=1e-5, msg=k)


@pytest.mark.parametrize("rows_per_blk", [128, 256, 512])
def test_spmm_lds_staged_diagonal_blocks_opt_in(rows_per_blk):
    """SparseTensor.stage_diagonal_blocks (LDS-DMA staging of a block's own source rows; opt-in) on the community graph in
    community order: same result as the oracle, with hub rows, and the in-block ranges are exactly the entries whose column
    lies in the row's block."""
    d = D.arxiv_like(scale=0.05, seed=3, with_teacher=False, graph="local-sorted")
    rowptr, col, _ = d.adj_t.csr()
    n = d.num_nodes
    o = OS.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n))
    p = d.adj_t.to(DEV).stage_diagonal_blocks(rows_per_blk)
    R, win = p._struct["locality"]
    rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    inblk = (col // R) == (rows // R)
    cnt_in = torch.zeros(n, dtype=torch.int64).index_add_(0, rows, inblk.long())
    w = win.cpu().long()
    assert torch.equal(w[:, 1] - w[:, 0], cnt_in), "window ranges = the intra-block entries, bit-exact"
    x = torch.randn(n, 96 if rows_per_blk == 128 else 256)
    for reduce in ("sum", "mean"):
        close(p.matmul(x.to(DEV), reduce), o.matmul(x, reduce), msg=reduce)
    p.stage_diagonal_blocks(None)
    close(p.matmul(x.to(DEV), "sum"), o.matmul(x, "sum"))


def test_spmm_full_size_properties():
    """BASELINE.json size (N=169 343, ~2.3 M nnz): size-independent properties instead of the oracle."""
    d = D.arxiv_like(1.0, seed=0, with_teacher=False)
    adj = d.adj_t.to(DEV)
    n = d.num_nodes
    cnt = (adj.csr()[0][1:] - adj.csr()[0][:-1]).float()
    ones = torch.ones(n, 8, device=DEV)
    deg, _ = ops.spmm_raw(adj, ones, "sum")
    assert torch.equal(deg[:, 0], cnt), "A * 1 = row counts, exactly (integers < 2^24)"
    x = torch.randn(n, 256, device=DEV)
    y, _ = ops.spmm_raw(adj, x, "sum")
    ym, _ = ops.spmm_raw(adj, x, "mean")
    close(ym * cnt.clamp(min=1).unsqueeze(1), y, rtol=1e-5)
    # linearity and symmetry: <A x, z> == <x, A^T z> with A symmetric
    z = torch.randn(n, 256, device=DEV)
    yz, _ = ops.spmm_raw(adj.t(), z, "sum")
    lhs, rhs = (y.double() * z.double()).sum(), (x.double() * yz.double()).sum()
    # the inner product cancels heavily (|<y,z>| << ||y|| ||z||): bound the fp32 rounding by the norms, not by the value
    assert abs(lhs - rhs) <= 1e-6 * float(y.double().norm() * z.double().norm())
    # spot rows against a gather-sum done with torch on the device (incl. the hub row)
    rowptr, col, _ = adj.csr()
    hub = int(torch.argmax(cnt))
    for r in [0, 1, hub, n - 1]:
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        ref = x[col[s:e]].double().sum(0)
        close(y[r], ref, rtol=1e-5)
    gn = E.gcn_norm(adj)
    rs, _ = ops.spmm_raw(gn, torch.ones(n, 4, device=DEV), "sum")
    dinv = (cnt + 1).pow(-0.5)
    rs_ref, _ = ops.spmm_raw(adj, dinv.unsqueeze(1).expand(n, 4).contiguous(), "sum")
    close(rs[:, 0], dinv * (rs_ref[:, 0] + dinv), rtol=1e-5)


def test_spmm_full_size_vs_oracle_k256():
    """BASELINE.json size against the CPU oracle itself (not only properties): the K = 256 GCN aggregation of the headline
    workload -- forward and the backward through the transposed CSR -- on the synthetic ogbn-arxiv graph, N = 169 343,
    nnz_hat = 2.5 M (reference call sites arxiv_pyg/gnn.py:47,52).  Layer-output bar rtol 1e-5 / atol 1e-5 max|ref|,
    gradient bar rtol 1e-4."""
    d = D.arxiv_like(1.0, seed=0, with_teacher=False)
    rowptr, col, _ = d.adj_t.csr()
    oadj = OS.gcn_norm_sparse(OS.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=d.adj_t.sparse_sizes()))
    padj = E.gcn_norm(d.adj_t.to(DEV))
    assert torch.equal(padj.csr()[0].cpu(), oadj.csr()[0]) and torch.equal(padj.csr()[1].cpu(), oadj.csr()[1])
    close(padj.csr()[2], oadj.csr()[2], rtol=2e-6)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(d.num_nodes, 256, generator=g)
    gy = torch.randn(d.num_nodes, 256, generator=g)
    xo = x.clone().requires_grad_(True)
    yo = OS.matmul(oadj, xo, "sum")
    yo.backward(gy)
    xp = x.to(DEV).requires_grad_(True)
    yp = ops.spmm(padj, xp, "sum")
    yp.backward(gy.to(DEV))
    close(yp, yo, rtol=1e-5)
    close(xp.grad, xo.grad, rtol=1e-4, atol_scale=1e-5)
    # SAGE's valueless mean aggregation at the same size (gnn.py:79,84)
    ym = ops.spmm(d.adj_t.to(DEV), x.to(DEV), "mean")
    close(ym, OS.matmul(OS.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=d.adj_t.sparse_sizes()), x, "mean"), rtol=1e-5)


# ------------------------------------------------------------------------------------------------
# dense GEMM
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (130, 70, 33), (256, 256, 256), (1000, 40, 256), (515, 256, 750), (64, 300, 17)])
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_all_layouts(M, N, K, ta, tb):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn((K, M) if ta else (M, K), generator=g)
    b = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g)
    ref = (a.t() if ta else a).double() @ (b.t() if tb else b).double() * 0.5 + bias.double()
    out = ops.gemm_raw(a.to(DEV), b.to(DEV), ta, tb, bias.to(DEV), alpha=0.5)
    close(out, ref, rtol=1e-5, atol_scale=2e-6, msg=f"{M}x{N}x{K} ta={ta} tb={tb}")


@pytest.mark.parametrize("M,N,K", [(5000, 256, 256), (4097, 128, 64), (169343, 256, 128), (8192, 384, 96)])
@pytest.mark.parametrize("tb", [False, True])
def test_gemm_dma_form_tall_a_small_b(M, N, K, tb):
    """The DMA form of egnn_gemm_f32 (csrc/gemm3.h: A by LDS-DMA as fp32 and cut on the fragment side, B cut once into
    tile-packed bf16 planes): tall A with a ragged last row tile, both weight layouts, bias and the fused ReLU, against a float64
    product; and bit-equal to itself across launches."""
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 6, (M, K), generator=g).float())).to(DEV)
    w = (torch.randn(N, K, generator=g) if tb else torch.randn(K, N, generator=g)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    ref = a.double() @ (w.double().t() if tb else w.double()) + bias.double()
    scale = (a.double().abs() @ (w.double().abs().t() if tb else w.double().abs())) + bias.double().abs()
    for relu in (False, True):
        y = ops.gemm_raw(a, w, False, tb, bias=bias, relu=relu)
        if not os.environ.get("EGNN_GEMM_PIPE", "").startswith("f"):
            assert ops.gemm_last_route() & 255 == 6, "not the DMA form"
        r = torch.relu(ref) if relu else ref
        assert float(((y.double() - r).abs() / scale).max()) < 1e-6
        assert torch.equal(y, ops.gemm_raw(a, w, False, tb, bias=bias, relu=relu))
    # autograd through linear / matmul at a DMA-form size
    m2 = min(M, 6000)
    x = a[:m2].clone().requires_grad_(True)
    wp = w.clone().requires_grad_(True)
    out = ops.linear(x, wp, bias) if tb else ops.matmul(x, wp, bias)
    gy = torch.randn(m2, N, generator=g).to(DEV)
    out.backward(gy)
    xd, wd = a[:m2].double().requires_grad_(True), w.double().requires_grad_(True)
    (xd @ (wd.t() if tb else wd) + bias.double()).backward(gy.double())
    close(x.grad, xd.grad, rtol=1e-4, atol_scale=2e-5)
    close(wp.grad, wd.grad, rtol=1e-4, atol_scale=2e-5)


@pytest.mark.parametrize("M,N,K", [(5000, 40, 256), (4099, 64, 128), (9001, 7, 64), (6000, 48, 16)])
@pytest.mark.parametrize("tb", [False, True])
def test_gemm_skinny_output_layer_forms(M, N, K, tb):
    """Class-count-wide shapes on the dedicated 16x16x4-MFMA kernels (csrc/gemm_skinny.hip): x W3 (+ bias), dX = dOut W3^T and
    dW3 = X^T dOut (both weight layouts: GCNConv [in,out], nn.Linear [out,in]) against fp64 torch."""
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(*((N, K) if tb else (K, N)), generator=g)
    bias = torch.randn(N, generator=g)
    ref = x.double() @ (w.double().t() if tb else w.double()) + bias.double()
    y = ops.gemm_raw(x.to(DEV), w.to(DEV), False, tb, bias.to(DEV))
    assert ops.gemm_last_route() == (1 if K == 256 else 2)        # the LDS-tile form takes 256-wide rows, skinny_fwd the others
    close(y, ref, rtol=1e-5, atol_scale=1e-6)
    y2 = ops.gemm_raw(x.to(DEV), w.to(DEV), False, tb, None, alpha=0.5)
    close(y2, 0.5 * (ref - bias.double()), rtol=1e-5, atol_scale=1e-6)
    # dX = dY op(W)': [M,N] x [N,K] -> [M,K] (needs K % 64 == 0 for the skinny form, else the general kernel: both must be right)
    gy = torch.randn(M, N, generator=g)
    dx = ops.gemm_raw(gy.to(DEV), w.to(DEV), False, not tb)
    close(dx, gy.double() @ (w.double() if tb else w.double().t()), rtol=1e-5, atol_scale=1e-6)
    # dW: both orientations of a^T b with the node count as the reduction
    dw_a = ops.gemm_raw(x.to(DEV), gy.to(DEV), True, False)      # [K, N]  (GCNConv weight gradient)
    assert ops.gemm_last_route() & 255 == (5 if K % 64 == 0 else 7)   # the wide matrix needs whole 64-column slices
    close(dw_a, x.double().t() @ gy.double(), rtol=2e-5, atol_scale=2e-6)
    dw_b = ops.gemm_raw(gy.to(DEV), x.to(DEV), True, False)      # [N, K]  (nn.Linear weight gradient)
    assert ops.gemm_last_route() & 255 == (4 if K % 64 == 0 else 7)
    close(dw_b, gy.double().t() @ x.double(), rtol=2e-5, atol_scale=2e-6)
    assert torch.equal(dw_a, ops.gemm_raw(x.to(DEV), gy.to(DEV), True, False)), "fixed reduction order => bit-stable"


def test_gemm_split_k_and_asymmetric_operand():
    # A = I with an asymmetric B catches row/column transposes of the MFMA fragment layout
    n = 160
    b = torch.arange(n * n, dtype=torch.float32).reshape(n, n) / 7.0
    out = ops.gemm_raw(torch.eye(n, device=DEV), b.to(DEV))
    assert torch.equal(out.cpu(), b)
    g = torch.Generator().manual_seed(0)
    x, gy = torch.randn(20000, 96, generator=g), torch.randn(20000, 72, generator=g)
    ref = x.double().t() @ gy.double()
    for sk in (1, 7, 32):
        close(ops.gemm_raw(x.to(DEV), gy.to(DEV), True, False, split_k=sk), ref, rtol=1e-5, atol_scale=2e-6, msg=f"split_k={sk}")
    o1 = ops.gemm_raw(x.to(DEV), gy.to(DEV), True, False, split_k=32)
    o2 = ops.gemm_raw(x.to(DEV), gy.to(DEV), True, False, split_k=32)
    assert torch.equal(o1, o2)


_PIPE_SNIPPET = r"""
import sys, torch
sys.path.insert(0, %r)
import efficient_gnns_amd.ops as ops
g = torch.Generator().manual_seed(5)
out = []
for (M, N, K, ta, tb) in [(4096, 256, 256, False, True), (3000, 384, 1000, False, False), (512, 256, 20000, True, False), (1500, 200, 750, True, True)]:
    # twelve binades of dynamic range inside every dot product: the low planes of the split carry real weight
    a = torch.randn((K, M) if ta else (M, K), generator=g) * torch.exp2(torch.randint(-6, 6, ((K, M) if ta else (M, K)), generator=g).float())
    b = torch.randn((N, K) if tb else (K, N), generator=g) * torch.exp2(torch.randint(-6, 6, ((N, K) if tb else (K, N)), generator=g).float())
    c = ops.gemm_raw(a.cuda(), b.cuda(), ta, tb).cpu().double()
    A, B = (a.t() if ta else a).double(), (b.t() if tb else b).double()
    err = ((c - A @ B).abs() / (A.abs() @ B.abs())).flatten()
    out.append((float(err.mean()), float(err.max())))
print("RESULT", out)
"""


def test_split_pipeline_error_is_not_above_the_f32_mfma_pipeline():
    """csrc/gemm_split.h claims fp32 results from the bf16 matrix pipe (three bf16 terms per operand, six exact partial
    products, dropped terms <= 2^-26 |a b|).  Both pipelines (EGNN_GEMM_PIPE selects one per process) are compared with a
    float64 product on operands with a wide dynamic range; error unit = sum_k |a_k b_k|.  The split pipeline must not be
    less accurate than the f32-input MFMA (it is slightly MORE accurate: its partial products are exact, only the
    accumulation rounds)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    # (the round-2 opt-in lab forms "planes" / "tile256" lost their measurements -- profiles/r02_gemm_split_lab.md -- and were removed
    # with their switches in round 5; the shapes below take the register-staged split pipeline and the DMA form of gemm3.h)
    variants = {"f32": dict(EGNN_GEMM_PIPE="f32"), "split": {}}
    for name, extra in variants.items():
        env = {k: v for k, v in os.environ.items() if k != "EGNN_GEMM_PIPE"}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PIPE_SNIPPET % root], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1]
        res[name] = eval(line[len("RESULT"):])
    for name in ("split",):
        for (mean_s, max_s), (mean_f, max_f) in zip(res[name], res["f32"]):
            assert mean_s <= 1.10 * mean_f, (name, res)          # the same fp32 accumulation rounding, no extra term
            assert max_s <= 1.5 * max_f and max_s < 2e-6, (name, res)
            assert mean_f < 2e-7, res                            # sanity: the unit is fp32 rounding (6e-8), not bf16 (4e-3)


def test_split_accuracy_one_pass_matches_evaluator_arithmetic():
    """egnn_split_accuracy_f32 = argmax (first maximal column) + per-split hit count / split size in double, the ogb
    Evaluator's arithmetic (gnn.py:198-218), incl. ties, an all-equal row, nodes in no split and an odd class count."""
    g = torch.Generator().manual_seed(3)
    for n, C in ((1000, 40), (777, 7), (5000, 349), (33, 1)):
        logits = torch.randn(n, C, generator=g).round(decimals=1)          # one decimal: many exact ties
        logits[5 % n] = 0.25                                                 # all columns equal -> column 0
        y = torch.randint(0, C, (n, 1), generator=g)
        perm = torch.randperm(n, generator=g)
        a, b = n // 2, n // 2 + n // 5
        split = {"train": perm[:a].clone(), "valid": perm[a:b].clone(), "test": perm[b:b + n // 10].clone()}   # the rest: unlabelled
        acc = ops.split_accuracy(logits.to(DEV), y.to(DEV), {k: v.to(DEV) for k, v in split.items()}).cpu()
        pred = logits.argmax(dim=-1)
        for i, k in enumerate(("train", "valid", "test")):
            idx = split[k]
            want = float((pred[idx] == y[idx, 0]).sum()) / max(idx.numel(), 1) if idx.numel() else float("nan")
            assert (acc[i] != acc[i] and want != want) or float(acc[i]) == want, (n, C, k, float(acc[i]), want)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_bn_state_update_kernel_matches_nn_batchnorm(momentum):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3000, 64, generator=g) * 2 + 0.5
    ref = torch.nn.BatchNorm1d(64, momentum=momentum)
    got = torch.nn.BatchNorm1d(64, momentum=momentum).to(DEV)
    ref.train(); got.train()
    for step in range(3):
        xs = x * (1 + step)
        ref(xs)
        ops.bn_act(xs.to(DEV), got, relu=False, p=0.0, training=True)
    close(got.running_mean, ref.running_mean, rtol=1e-5, atol_scale=1e-6)
    close(got.running_var, ref.running_var, rtol=1e-5, atol_scale=1e-6)
    assert int(got.num_batches_tracked) == int(ref.num_batches_tracked) == 3


def test_bias_gradient_formed_in_the_bn_backward_and_row_compact_tap():
    """(1) The fused BatchNorm backward tags dx with its column sums (the gradient of a bias in front of the BatchNorm):
    the tag equals dx.sum(0) to rounding and ops.colsum returns it.  (2) linear_rows on a grad_tap tensor hands its
    input gradient over row-compact: the tapped tensor's gradient equals the plain dense accumulation."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(5000, 256, generator=g).to(DEV).requires_grad_()
    bn = torch.nn.BatchNorm1d(256).to(DEV)
    seen = []
    x.register_hook(lambda gr: seen.append(gr))
    y = ops.bn_act(x, bn, relu=True, p=0.0, training=True)
    (y * torch.randn(5000, 256, generator=g).to(DEV)).sum().backward()
    gr = seen[0]
    tag = getattr(gr, "_egnn_colsum", None)
    assert tag is not None and tag[1] == gr._version
    scale = gr.abs().sum(0)
    assert float(((tag[0] - gr.double().sum(0).float()).abs() / scale).max()) < 1e-6
    assert ops.colsum(gr) is tag[0]
    gr.add_(1.0)                                  # an in-place change voids the tag
    assert ops.colsum(gr) is not tag[0]

    def run(tap):
        torch.manual_seed(0)
        h0 = torch.randn(4000, 64, generator=torch.Generator().manual_seed(7)).to(DEV).requires_grad_()
        w1 = torch.randn(32, 64, generator=torch.Generator().manual_seed(8)).to(DEV).requires_grad_()
        w2 = torch.randn(16, 64, generator=torch.Generator().manual_seed(9)).to(DEV).requires_grad_()
        idx = torch.randperm(4000, generator=torch.Generator().manual_seed(10))[:1500].to(DEV)
        h = h0 * 2.0
        h = ops.grad_tap(h) if tap else h
        out = ops.linear(h, w1).square().sum() + ops.linear_rows(h, idx, w2).square().sum()
        out.backward()
        return h0.grad, w1.grad, w2.grad
    a, b = run(True), run(False)
    for u, v in zip(a, b):
        close(u, v, rtol=1e-6, atol_scale=1e-6)


def test_grad_tap_never_edits_a_gradient_it_does_not_own_and_stale_tags_are_ignored():
    """Hygiene of the tensor-tag shortcuts (round-2 review): (1) ``_GradTap`` adds the row-compact pieces in place only into a
    gradient this package has just allocated; a pass-through consumer (``h + 0``: AddBackward hands its grad_output on) must see
    its caller's gradient untouched and the result must still be the dense accumulation.  (2) The BatchNorm statistics tag of
    ``ops.spmm`` is version-checked: an in-place edit of the aggregated tensor makes ``bn_act`` recompute them.  (3) The
    "ReLU already applied" state of ``spmm_raw`` is a return value, not a tag on a (caller-owned, reusable) ``out`` buffer."""
    gen = torch.Generator().manual_seed(3)
    h0 = torch.randn(3000, 64, generator=gen).to(DEV).requires_grad_()
    w2 = torch.randn(16, 64, generator=gen).to(DEV)
    idx = torch.randperm(3000, generator=gen)[:1000].to(DEV)
    gy = torch.randn(3000, 64, generator=gen).to(DEV)
    gy_copy = gy.clone()
    h = ops.grad_tap(h0 * 1.0)
    z = ops.linear_rows(h, idx, w2)
    torch.autograd.backward([h + 0, z], [gy, torch.ones_like(z)])
    assert torch.equal(gy, gy_copy), "the caller's grad_output was modified in place"
    ref = gy_copy.clone()
    ref[idx] += torch.ones(1000, 16, device=DEV) @ w2
    close(h0.grad, ref, rtol=1e-5, atol_scale=1e-6)
    # (2)
    row, col = random_csr(2000, 2000, 6.0, seed=5)
    _, adj = make_pair(row, col, None, (2000, 2000))
    x = torch.randn(2000, 128, generator=gen).to(DEV)
    bn = torch.nn.BatchNorm1d(128).to(DEV)
    y = ops.spmm(adj, x, "sum", want_bn_stats=True, bn_stats_shift=bn.running_mean)
    assert getattr(y, "_egnn_bn_stats", None) is not None
    y.mul_(3.0).add_(1.0)
    out = ops.bn_act(y, bn, relu=False, p=0.0, training=True)
    close(out, torch.nn.functional.batch_norm(y, None, None, bn.weight, bn.bias, True, 0.0, bn.eps), rtol=1e-4, atol_scale=1e-5)
    # (3) one output buffer, first through the block kernel with the fused ReLU, then through a schedule without it
    buf = torch.empty(2000, 128, device=DEV)
    ops.spmm_raw(adj, x, "sum", out=buf, relu=True)
    assert not hasattr(buf, "_egnn_relu_done")
    x40 = torch.randn(2000, 40, generator=gen).to(DEV)
    buf40 = torch.empty(2000, 40, device=DEV)
    for _ in range(2):
        got, _ = ops.spmm_raw(adj, x40, "sum", out=buf40, relu=True)      # K < 64: segment schedule, the clamp follows
        plain, _ = ops.spmm_raw(adj, x40, "sum")
        assert torch.equal(got, plain.clamp(min=0))


def test_split_pipeline_non_finite_and_tiny_operands():
    """Documented edge semantics of the three-way bf16 split (csrc/gemm_split.h): an infinite operand gives NaN in every
    output it touches (inf - inf while cutting; the f32-input MFMA would give inf or NaN) and leaves all other outputs
    exact; NaN propagates; operands whose low terms fall below the bf16 subnormal range (|x| < 2^-110) lose only those
    terms -- the product keeps at least the leading 8 bits and anything >= 2^-100 keeps fp32 accuracy."""
    gen = torch.Generator().manual_seed(1)
    M, N, K = 256, 256, 64
    a = torch.randn(M, K, generator=gen)
    b = torch.randn(K, N, generator=gen)
    ref = (a.double() @ b.double())
    a_inf = a.clone()
    a_inf[3, 5] = float("inf")
    a_inf[7, 9] = float("nan")
    y = ops.matmul(a_inf.to(DEV), b.to(DEV)).cpu()
    assert torch.isnan(y[3]).all() and torch.isnan(y[7]).all()
    keep = torch.ones(M, dtype=torch.bool)
    keep[[3, 7]] = False
    close(y[keep], ref[keep], rtol=1e-5, atol_scale=1e-6)
    # tiny operands: 2^-100 scale stays fp32-accurate (the third term of 2^-100 x is ~2^-116 >= the bf16 subnormal floor 2^-133)
    s = 2.0 ** -100
    y_small = ops.matmul((a * s).to(DEV), b.to(DEV)).cpu().double() / s
    close(y_small, ref, rtol=1e-5, atol_scale=2e-6)
    # 2^-120: the low terms are flushed / subnormal; what is left is at least the 8 leading bits of every element
    s = 2.0 ** -120
    y_tiny = ops.matmul((a * s).to(DEV), b.to(DEV)).cpu().double() / s
    assert torch.isfinite(y_tiny).all()
    err = (y_tiny - ref).abs().max() / ref.abs().max()
    assert float(err) < 2.0 ** -6, float(err)


def test_eval_mode_batchnorm_fold_and_relu_epilogues():
    """test() (gnn.py:198-218): the eval-mode BatchNorm folded into the conv's weights (egnn_bn_fold_f32) + ReLU in the last
    kernel's store (GEMM / aggregation / hub-row combine) equals the unfused chain conv -> bn_act; plus the two relu
    epilogues on their own, incl. the K < 64 aggregation (clamp after the segment kernel)."""
    d = D.arxiv_like(scale=0.05, seed=5)
    adj = d.adj_t.to(DEV)
    torch.manual_seed(3)
    model = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.5).to(DEV)
    with torch.no_grad():
        for bn in model.bns:                      # running statistics / affine parameters away from their initial values
            bn.running_mean.copy_(torch.randn(64, device=DEV) * 0.3)
            bn.running_var.copy_(torch.rand(64, device=DEV) + 0.5)
            bn.weight.copy_(torch.rand(64, device=DEV) + 0.5)
            bn.bias.copy_(torch.randn(64, device=DEV) * 0.2)
        for conv in model.convs:
            conv.bias.copy_(torch.randn_like(conv.bias) * 0.1)
    model.eval()
    x = d.x.to(DEV)
    outs = {}
    for fold in (True, False):
        PM._EVAL_BN_FOLD = fold
        try:
            with torch.no_grad():
                outs[fold] = model(x, adj).clone()
                feat = model.out_feat.clone()
            outs[(fold, "feat")] = feat
        finally:
            PM._EVAL_BN_FOLD = True
    close(outs[True], outs[False], rtol=1e-5, atol_scale=2e-6)
    close(outs[(True, "feat")], outs[(False, "feat")], rtol=1e-5, atol_scale=2e-6)
    assert float(outs[(True, "feat")].min()) >= 0.0
    g = torch.Generator().manual_seed(1)
    a, b, bias = torch.randn(3000, 96, generator=g), torch.randn(96, 200, generator=g), torch.randn(200, generator=g)
    close(ops.gemm_raw(a.to(DEV), b.to(DEV), False, False, bias.to(DEV), relu=True), torch.relu(a.double() @ b.double() + bias.double()),
          rtol=1e-5, atol_scale=2e-6)
    for K in (256, 40):
        xx = torch.randn(d.num_nodes, K, generator=g)
        bb = torch.randn(K, generator=g)
        y = ops.spmm_raw(adj, xx.to(DEV), "sum", bias=bb.to(DEV), relu=True)[0]
        ref = torch.relu(ops.spmm_raw(adj, xx.to(DEV), "sum", bias=bb.to(DEV))[0])
        assert torch.equal(y, ref), K


def test_linear_and_matmul_autograd():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(777, 128, generator=g)
    w = torch.randn(128, 40, generator=g)
    wl = torch.randn(256, 128, generator=g)
    bl = torch.randn(256, generator=g)
    for kind in ("matmul", "linear"):
        xr = x.clone().requires_grad_(True)
        xg = x.to(DEV).requires_grad_(True)
        if kind == "matmul":
            wr, wg = w.clone().requires_grad_(True), w.to(DEV).requires_grad_(True)
            yr, yg = xr @ wr, ops.matmul(xg, wg)
            params = [(wr, wg)]
        else:
            wr, wg = wl.clone().requires_grad_(True), wl.to(DEV).requires_grad_(True)
            br, bg = bl.clone().requires_grad_(True), bl.to(DEV).requires_grad_(True)
            yr, yg = torch.nn.functional.linear(xr, wr, br), ops.linear(xg, wg, bg)
            params = [(wr, wg), (br, bg)]
        close(yg, yr, rtol=1e-5, atol_scale=2e-6)
        gy = torch.randn(yr.shape, generator=g)
        yr.backward(gy)
        yg.backward(gy.to(DEV))
        close(xg.grad, xr.grad, rtol=1e-4, atol_scale=1e-5)
        for r, q in params:
            close(q.grad, r.grad, rtol=1e-4, atol_scale=1e-5)


# ------------------------------------------------------------------------------------------------
# convs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gcn", "sage_mean", "sage_max", "sage_sum"])
def test_conv_layers_vs_oracle(kind):
    n, fin, fout = 600, 50, 121
    row, col = random_csr(n, n, 8, seed=2, hubs=((1, 700),))
    o, p = make_pair(row, col, None, (n, n))
    o, p = o.to_symmetric(), p.to_symmetric()
    torch.manual_seed(0)
    if kind == "gcn":
        co, cp = ON.GCNConv(fin, fout, cached=True), E.GCNConv(fin, fout, cached=True).to(DEV)
    else:
        aggr = kind.split("_")[1]
        co, cp = ON.SAGEConv(fin, fout, aggr=aggr), E.SAGEConv(fin, fout, aggr=aggr).to(DEV)
    cp.load_state_dict(co.state_dict())
    x = torch.randn(n, fin)
    xo, xp = x.clone().requires_grad_(True), x.to(DEV).requires_grad_(True)
    yo, yp = co(xo, o), cp(xp, p)
    close(yp, yo, msg=kind)
    gy = torch.randn(n, fout)
    yo.backward(gy)
    yp.backward(gy.to(DEV))
    close(xp.grad, xo.grad, rtol=1e-4, msg=kind)
    for (k, a), (_, b) in zip(cp.named_parameters(), co.named_parameters()):
        close(a.grad, b.grad, rtol=1e-4, msg=f"{kind}:{k}")


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_sageconv_output_layer_transforms_before_aggregating(aggr):
    """SAGEConv with out < in (the 256 -> 40 output layer, gnn.py:84) aggregates lin_l(x) instead of x: same result as the oracle's
    aggregate-first order, rows without neighbours included (they get the bias), forward and backward."""
    n, fin, fout = 5000, 256, 40
    row, col = random_csr(n, n, 6, seed=7, hubs=((3, 900),), empty_frac=0.2)
    o, p = make_pair(row, col, None, (n, n))
    torch.manual_seed(1)
    co, cp = ON.SAGEConv(fin, fout, aggr=aggr), E.SAGEConv(fin, fout, aggr=aggr).to(DEV)
    cp.load_state_dict(co.state_dict())
    x = torch.randn(n, fin)
    xo, xp = x.clone().requires_grad_(True), x.to(DEV).requires_grad_(True)
    yo, yp = co(xo, o), cp(xp, p)
    close(yp, yo, rtol=2e-5, msg=aggr)
    gy = torch.randn(n, fout)
    yo.backward(gy)
    yp.backward(gy.to(DEV))
    close(xp.grad, xo.grad, rtol=1e-4, msg=aggr)
    for (k, a), (_, b) in zip(cp.named_parameters(), co.named_parameters()):
        close(a.grad, b.grad, rtol=1e-4, msg=f"{aggr}:{k}")


def test_gcnconv_edge_index_input_ppi_path():
    n = 300
    g = torch.Generator().manual_seed(4)
    ei = torch.stack([torch.randint(0, n, (2500,), generator=g), torch.randint(0, n, (2500,), generator=g)])
    ei = torch.cat([ei, ei.flip(0)], dim=1)  # symmetric like PPI, with a few self loops and duplicates
    torch.manual_seed(0)
    co, cp = ON.GCNConv(50, 64, cached=False), E.GCNConv(50, 64, cached=False).to(DEV)
    cp.load_state_dict(co.state_dict())
    x = torch.randn(n, 50)
    close(cp(x.to(DEV), ei.to(DEV)), co(x, ei))
    so, sp = ON.SAGEConv(50, 64), E.SAGEConv(50, 64).to(DEV)
    sp.load_state_dict(so.state_dict())
    close(sp(x.to(DEV), ei.to(DEV)), so(x, ei))


# ------------------------------------------------------------------------------------------------
# criteria: golden vectors produced by the reference's own criterion.py
# ------------------------------------------------------------------------------------------------
def _run_case(fn, leaves, seed):
    L = {k: v.clone().requires_grad_(True) for k, v in leaves.items()}
    if seed is not None:
        np.random.seed(seed)
    loss, loss_cls, loss_aux = fn(L)
    g = torch.autograd.grad(loss, list(L.values()), allow_unused=True, retain_graph=True)
    ga = torch.autograd.grad(loss_aux, list(L.values()), allow_unused=True)
    rec = {"loss": loss, "loss_cls": loss_cls, "loss_aux": loss_aux}
    for (k, _), a, b in zip(L.items(), g, ga):
        rec["grad_" + k] = a
        rec["auxgrad_" + k] = b
    return rec


def test_criteria_match_reference_goldens(golden_criterion):
    G = golden_criterion
    cases, _ = criterion_cases(G, PC, DEV)
    failures = []
    for name, fn, leaves, seed in cases:
        try:
            rec = _run_case(fn, leaves, seed)
            for k, v in rec.items():
                ref = G[f"{name}__{k}"]
                if v is None:
                    assert ref.size == 0 or np.abs(ref).max() == 0, f"{name}:{k} missing grad"
                    continue
                rtol = 2e-5 if k.startswith("loss") else 1e-4
                close(v, ref, rtol=rtol, atol_scale=1e-5 if not k.startswith("loss") else 0, msg=f"{name}:{k}")
        except NotImplementedError as ex:  # pragma: no cover
            failures.append(f"{name}: not implemented {ex}")
        except AssertionError as ex:
            failures.append(f"{name}: {str(ex)[:300]}")
    assert not failures, "\n".join(failures)


def test_ppi_auxiliary_criteria_match_reference_goldens(golden_criterion, golden_criterion_ppi):
    """The PPI drop-in's fitnet / at / gpw / lpw / nce (multi-label BCE classification term) on the kernels against the goldens
    produced by the reference's own ppi_pyg/criterion.py:21-146 -- through the module ``dropin/launch.py`` puts in front of the
    ppi_pyg scripts, i.e. under the reference's names."""
    import importlib.util
    import types
    from test_oracle_golden import ppi_aux_cases
    path = os.path.join(os.path.dirname(os.path.abspath(PC.__file__)), "dropin", "ppi_pyg", "criterion.py")
    spec = importlib.util.spec_from_file_location("_ppi_dropin_criterion", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    shim = types.SimpleNamespace(ppi_fitnet_criterion=mod.fitnet_criterion, ppi_at_criterion=mod.at_criterion, ppi_gpw_criterion=mod.gpw_criterion,
                                 ppi_lpw_criterion=mod.lpw_criterion, ppi_nce_criterion=mod.nce_criterion)
    Gp = golden_criterion_ppi
    failures = []
    for name, fn, leaves, seed in ppi_aux_cases(golden_criterion, Gp, shim, DEV):
        try:
            rec = _run_case(fn, leaves, seed)
            for k, v in rec.items():
                ref = Gp[f"{name}__{k}"]
                if v is None:
                    assert ref.size == 0 or np.abs(ref).max() == 0, f"{name}:{k} missing grad"
                    continue
                close(v, ref, rtol=2e-5 if k.startswith("loss") else 1e-4, atol_scale=1e-5 if not k.startswith("loss") else 0, msg=f"{name}:{k}")
        except AssertionError as ex:
            failures.append(f"{name}: {str(ex)[:300]}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n,Ds,Dt", [(1, 8, 8), (777, 256, 256), (5000, 128, 128), (3001, 64, 750)])
def test_fitnet_and_at_kernels_vs_oracle(n, Ds, Dt):
    """egnn_fitnet_* / egnn_at_* (criterion.py:24-54) against the oracle at sizes beyond the goldens, with all-zero rows (the
    eps clamp of F.normalize: constant denominator, no projection term in the gradient)."""
    g = torch.Generator().manual_seed(n)
    logits, labels = torch.randn(n, 5, generator=g), torch.randint(0, 5, (n,), generator=g)
    f = torch.relu(torch.randn(n, Ds, generator=g))
    t = torch.relu(torch.randn(n, Dt, generator=g)) * 0.7
    if n > 10:
        f[3] = 0.0
        t[5] = 0.0
    for name in ("fitnet", "at"):
        if name == "fitnet" and Ds != Dt:
            with pytest.raises(ValueError):
                E.fitnet_criterion(logits.to(DEV), labels.to(DEV), f.to(DEV), t.to(DEV))
            continue
        fo, to_ = f.clone().requires_grad_(True), t.clone().requires_grad_(True)
        fp, tp = f.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
        ref = getattr(OC, f"{name}_criterion")(logits, labels, fo, to_, 1000)
        out = getattr(E, f"{name}_criterion")(logits.to(DEV), labels.to(DEV), fp, tp, 1000)
        close(out[2], ref[2], rtol=2e-5, atol_scale=0, msg=f"{name} loss_aux")
        close(out[0], ref[0], rtol=2e-5, atol_scale=0, msg=f"{name} loss")
        ref[0].backward()
        out[0].backward()
        close(fp.grad, fo.grad, rtol=1e-4, atol_scale=2e-5, msg=f"{name} d feat")
        close(tp.grad, to_.grad, rtol=1e-4, atol_scale=2e-5, msg=f"{name} d teacher_feat")


def test_ppi_kd_matches_reference_golden(golden_criterion):
    G = golden_criterion
    pl, py, pt = (as_t(G["in_ppi_" + k], DEV) for k in ("logits", "labels", "teacher"))
    rec = _run_case(lambda L: E.ppi_kd_criterion(L["logits"], py, pt, 0.5, 1.0), {"logits": pl}, None)
    for k, v in rec.items():
        close(v, G[f"ppi_kd__{k}"], rtol=2e-5 if k.startswith("loss") else 1e-4, atol_scale=1e-5)


@pytest.mark.parametrize("n,C,T", [(1, 2, 1.0), (257, 40, 4.0), (1000, 121, 2.0), (5000, 7, 4.0)])
def test_ce_kd_kernel_vs_oracle(n, C, T):
    g = torch.Generator().manual_seed(n)
    logits = (torch.randn(n, C, generator=g) * 3).requires_grad_(True)
    labels = torch.randint(0, C, (n,), generator=g)
    teacher = torch.randn(n, C, generator=g) * 4
    ref = OC.kd_criterion(logits, labels, teacher, 0.9, T)
    lg = logits.detach().to(DEV).requires_grad_(True)
    out = E.kd_criterion(lg, labels.to(DEV), teacher.to(DEV), 0.9, T)
    for a, b in zip(out, ref):
        close(a, b, rtol=1e-5, atol_scale=0)
    ref[0].backward()
    out[0].backward()
    close(lg.grad, logits.grad, rtol=1e-4)


def test_criteria_rows_twins_equal_the_compact_call():
    """The ``rows_*`` twins of the criteria (full logits / labels / teacher logits + the row ids, picked inside the CE / KD
    kernels) gives the losses of the reference-style call on ``logits[rows]`` bit for bit and the same logits gradient, scattered."""
    g = torch.Generator().manual_seed(4)
    N, C = 3000, 40
    logits = torch.randn(N, C, generator=g).to(DEV)
    labels = torch.randint(0, C, (N,), generator=g).to(DEV)
    teacher = (torch.randn(N, C, generator=g) * 3).to(DEV)
    rows = torch.randperm(N, generator=g)[:1700].to(DEV)
    f = torch.relu(torch.randn(1700, 64, generator=g)).to(DEV)
    t = torch.relu(torch.randn(1700, 64, generator=g)).to(DEV)
    for name, full, compact in (
            ("kd", lambda L: PC.rows_kd_criterion(L, labels, teacher, 0.9, 4, rows=rows), lambda L: E.kd_criterion(L[rows], labels[rows], teacher[rows], 0.9, 4)),
            ("nce", lambda L: PC.rows_nce_criterion(L, labels, f, t, 0.1, 0.075, 4096, rows=rows), lambda L: E.nce_criterion(L[rows], labels[rows], f, t, 0.1, 0.075, 4096)),
            ("gpw", lambda L: PC.rows_gpw_criterion(L, labels, f, t, "cosine", 1.0, 4096, rows=rows), lambda L: E.gpw_criterion(L[rows], labels[rows], f, t, "cosine", 1.0, 4096))):
        a = logits.clone().requires_grad_(True)
        b = logits.clone().requires_grad_(True)
        la, lb = full(a), compact(b)
        for x, y in zip(la, lb):
            assert float(x) == float(y), name
        la[0].backward()
        lb[0].backward()
        assert torch.equal(a.grad, b.grad), name
        assert float(a.grad[rows].abs().sum()) > 0 and float(a.grad.abs().sum()) == float(a.grad[rows].abs().sum()), "rows outside the list get exact zeros"


@pytest.mark.parametrize("S,P,n,tau", [(64, 16, 64, 0.075), (300, 72, 500, 0.075), (1000, 256, 1000, 0.05), (2048, 256, 3000, 0.075)])
def test_nce_vs_oracle(S, P, n, tau):
    g = torch.Generator().manual_seed(S)
    logits = torch.randn(n, 5, generator=g)
    labels = torch.randint(0, 5, (n,), generator=g)
    f = torch.relu(torch.randn(n, P, generator=g))
    t = torch.relu(torch.randn(n, P, generator=g) + 0.3 * f)
    fo, to_ = f.clone().requires_grad_(True), t.clone().requires_grad_(True)
    fp, tp = f.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    np.random.seed(S)
    ref = OC.nce_criterion(logits, labels, fo, to_, 0.1, tau, S)
    np.random.seed(S)
    out = E.nce_criterion(logits.to(DEV), labels.to(DEV), fp, tp, 0.1, tau, S)
    close(out[2], ref[2], rtol=2e-5, atol_scale=0, msg="loss_nce")
    close(out[0], ref[0], rtol=2e-5, atol_scale=0)
    ref[0].backward()
    out[0].backward()
    close(fp.grad, fo.grad, rtol=1e-4, atol_scale=2e-5)
    close(tp.grad, to_.grad, rtol=1e-4, atol_scale=2e-5)


def test_nce_full_size_vs_oracle_s16384():
    """G-CRD at the script-of-record size S = 16 384, P = 256, tau = 0.075 (run_gcn.sh:140-145) against the CPU oracle's
    nce_criterion (criterion.py:129-149) on the same rows: loss rtol 2e-5, gradients rtol 1e-4 (atol 2e-5 max|ref|)."""
    S, P, tau = 16384, 256, 0.075
    g = torch.Generator().manual_seed(11)
    f = torch.randn(S, P, generator=g)
    t = torch.relu(torch.randn(S, P, generator=g)) + 0.05 * torch.randn(S, P, generator=g)
    logits = torch.randn(S, 40, generator=g)
    labels = torch.randint(0, 40, (S,), generator=g)

    def run(mod, dev):
        fl, tl, ll = (v.to(dev).clone().requires_grad_(True) for v in (f, t, logits))
        loss, loss_cls, loss_aux = mod.nce_criterion(ll, labels.to(dev), fl, tl, 0.1, tau, S)   # max_samples == n: no draw
        loss.backward()
        return (loss, loss_cls, loss_aux), (fl.grad, tl.grad, ll.grad)
    (lo, go), (lp, gp) = run(OC, "cpu"), run(PC, DEV)
    for a, b in zip(lp, lo):
        assert abs(float(a) - float(b)) <= 2e-5 * abs(float(b)), (lp, lo)
    for a, b in zip(gp, go):
        close(a, b, rtol=1e-4, atol_scale=2e-5)


def test_nce_full_size_properties():
    """S = 16384, P = 256 (run_gcn.sh:140-145): properties that need no S x S oracle."""
    S, P = 16384, 256
    g = torch.Generator(device=DEV).manual_seed(0)
    f = torch.nn.functional.normalize(torch.randn(S, P, device=DEV, generator=g), dim=-1)
    # identical student and teacher with tiny tau: the positive dominates, loss -> ~0
    l0 = ops.nce_unit(f, f.clone(), 0.01)
    assert float(l0) < 1e-3
    # orthogonal-ish random teacher: loss ~ log(S) + small; and invariance to a row permutation applied to both
    t = torch.nn.functional.normalize(torch.randn(S, P, device=DEV, generator=g), dim=-1)
    l1 = ops.nce_unit(f, t, 0.075)
    perm = torch.randperm(S, device=DEV)
    l2 = ops.nce_unit(f[perm].contiguous(), t[perm].contiguous(), 0.075)
    assert abs(float(l1) - float(l2)) <= 2e-5 * abs(float(l1))
    assert abs(float(l1) - np.log(S)) < 1.0
    # gradient rows are orthogonal to nothing in particular, but sum_i dL/df_i . f_i relation: check against
    # a row-block evaluated with torch on the device
    fr = f.clone().requires_grad_(True)
    tr = t.clone().requires_grad_(True)
    ops.nce_unit(fr, tr, 0.075).backward()
    rows = torch.arange(0, S, 997, device=DEV)
    z = (f[rows] @ t.t()) / 0.075
    p = torch.softmax(z.double(), dim=1)
    p[torch.arange(rows.numel(), device=DEV), rows] -= 1.0
    ref = (p @ t.double()) / (S * 0.075)
    close(fr.grad[rows], ref, rtol=1e-4, atol_scale=2e-5)


# ------------------------------------------------------------------------------------------------
# whole train / eval step vs goldens produced by the reference's own gnn.py
# ------------------------------------------------------------------------------------------------
def _build_adj_dev(G):
    n = G["in_x"].shape[0]
    return E.to_sparse_tensor(as_t(G["in_edge_index"], DEV), n).to_symmetric()


def test_train_and_eval_match_reference_goldens(golden_train):
    G = golden_train
    failures = []
    for name in G["run_names"]:
        name = str(name)
        tag = name.split(":")[0]
        try:
            model, losses, logits0, accs0 = run_training(G, name, PM, _build_adj_dev, DEV)
            mode = parse_run(name)[2]
            # SINGLE-step bars: eval logits of the initial state rtol 1e-5 (+ 1e-5 max|ref|), the three losses of
            # the first step rtol 1e-5 (G-CRD / GSP 2e-5)
            close(logits0, G[f"{tag}__eval0_logits"], rtol=1e-5, atol_scale=1e-5, msg=name)
            close(losses[0], G[f"{tag}__losses"][0], rtol=2e-5 if mode in ("nce", "gpw") else 1e-5, atol_scale=0, msg=f"{name}: step 1")
            # TRAJECTORY bars (steps 2-3, final weights): Adam's update is lr * m / (sqrt(v) + eps) -- for an entry whose
            # gradient is rounding-sized both m and sqrt(v) are, and the quotient is an O(1) number of either sign, so the
            # first update already moves such weights by +-lr in an implementation-dependent direction (the reference's own
            # CUDA and CPU paths differ the same way); what is comparable after that is the loss to ~1e-4 and the weights to
            # a fraction of lr = 0.01
            close(losses, G[f"{tag}__losses"], rtol=2e-4, atol_scale=0, msg=name)
            for k, v in model.state_dict().items():
                if noise_driven(k, int(G["hp"][2])):
                    continue
                close(v, G[f"{tag}__final__model.{k}"], rtol=2e-3, atol_scale=2e-3, msg=f"{name}:{k}")
        except NotImplementedError as ex:  # pragma: no cover
            failures.append(f"{name}: not implemented {ex}")
        except AssertionError as ex:
            failures.append(f"{name}: {str(ex)[:400]}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------
# LSP / GSP building blocks at larger sizes than the goldens
# ------------------------------------------------------------------------------------------------
def test_segment_softmax_unsorted_index_vs_oracle():
    g = torch.Generator().manual_seed(0)
    E_, n = 5000, 300
    src = (torch.randn(E_, generator=g) * 3).requires_grad_(True)
    index = torch.randint(0, n, (E_,), generator=g)
    index[:900] = 7  # one long segment (> 64 entries), some empty segments exist too
    ref = OU.softmax(src, index, n)
    sp = src.detach().to(DEV).requires_grad_(True)
    out = E.softmax(sp, index.to(DEV), num_nodes=n)
    close(out, ref, rtol=1e-5, atol_scale=1e-6)
    w = torch.randn(E_, generator=g)
    (ref * w).sum().backward()
    (out * w.to(DEV)).sum().backward()
    close(sp.grad, src.grad, rtol=1e-4, atol_scale=1e-5)


@pytest.mark.parametrize("kernel", ["cosine", "poly", "l2", "rbf"])
@pytest.mark.parametrize("crit", ["kld", "mse"])
def test_lsp_vs_oracle_on_train_subgraph(kernel, crit):
    d = D.arxiv_like(scale=0.02, seed=5)
    tr = d.split_idx["train"]
    ei = OU.subgraph(tr, torch.stack(d.adj_t.coo()[:2]), relabel_nodes=True, num_nodes=d.num_nodes)[0]
    g = torch.Generator().manual_seed(1)
    n_tr = tr.numel()
    scale = 0.15 if kernel in ("l2", "rbf") else 1.0   # keep rbf similarities away from exp underflow
    f = (torch.relu(torch.randn(n_tr, 256, generator=g)) * scale)
    t = (torch.relu(torch.randn(n_tr, 750, generator=g)) * scale * 0.6)
    logits, labels = torch.randn(n_tr, 40, generator=g), torch.randint(0, 40, (n_tr,), generator=g)
    fo, to_ = f.clone().requires_grad_(True), t.clone().requires_grad_(True)
    fp, tp = f.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    ref = OC.lpw_criterion(logits, labels, fo, to_, ei, kernel, 100, crit)
    out = E.lpw_criterion(logits.to(DEV), labels.to(DEV), fp, tp, ei.to(DEV), kernel, 100, crit)
    close(out[2], ref[2], rtol=1e-5, atol_scale=0, msg="loss_lpw")
    ref[2].backward()
    out[2].backward()
    close(fp.grad, fo.grad, rtol=1e-4, atol_scale=2e-5)
    close(tp.grad, to_.grad, rtol=1e-4, atol_scale=2e-5)


@pytest.mark.parametrize("kernel,S,P", [("cosine", 1000, 128), ("poly", 777, 128), ("l2", 600, 64), ("rbf", 900, 128), ("cosine", 4096, 128)])
def test_gsp_vs_oracle(kernel, S, P):
    g = torch.Generator().manual_seed(S)
    n = S + 500
    scale = 0.12 if kernel in ("l2", "rbf") else 1.0
    f = torch.relu(torch.randn(n, P, generator=g)) * scale
    t = torch.relu(torch.randn(n, P, generator=g) + 0.2 * f) * scale
    logits, labels = torch.randn(n, 5, generator=g), torch.randint(0, 5, (n,), generator=g)
    fo, to_ = f.clone().requires_grad_(True), t.clone().requires_grad_(True)
    fp, tp = f.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    np.random.seed(S)
    ref = OC.gpw_criterion(logits, labels, fo, to_, kernel, 1.0, S)
    np.random.seed(S)
    out = E.gpw_criterion(logits.to(DEV), labels.to(DEV), fp, tp, kernel, 1.0, S)
    close(out[2], ref[2], rtol=2e-5, atol_scale=0, msg="loss_gpw")
    ref[2].backward()
    out[2].backward()
    close(fp.grad, fo.grad, rtol=1e-4, atol_scale=2e-5)
    close(tp.grad, to_.grad, rtol=1e-4, atol_scale=2e-5)


def test_gsp_stress_all_pairs_beyond_reference_capacity():
    """S = 16384 with the rbf kernel: the reference would need a [S,S,P] fp32 tensor (137 GB at P=128)."""
    S, P = 16384, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    f = torch.randn(S, P, device=DEV, generator=g) * 0.1
    from efficient_gnns_amd.ops_pairwise import gsp_loss
    same = gsp_loss(f, f.clone(), None, "rbf")
    assert float(same) == 0.0, "identical student and teacher => exactly zero loss"
    t = f + 0.01 * torch.randn(S, P, device=DEV, generator=g)
    rows = torch.arange(0, S, 1237, device=DEV)
    l = gsp_loss(f, t, None, "rbf")

    def k(x):
        d2 = (x[rows].double().unsqueeze(1) - x.double().unsqueeze(0)).pow(2).sum(-1)
        return torch.exp(-0.5 * d2)
    est = (k(f) - k(t)).pow(2).mean()
    assert abs(float(l) - float(est)) < 0.2 * float(est) + 1e-12  # row-sample estimate of the same mean


# ------------------------------------------------------------------------------------------------
# fused BatchNorm + ReLU + dropout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,relu", [(1000, 256, True), (777, 128, False), (5001, 40, True), (300, 1024, True)])
def test_fused_bn_act_matches_torch_batchnorm(n, C, relu):
    g = torch.Generator().manual_seed(n + C)
    x = torch.randn(n, C, generator=g) * 2 + torch.randn(C, generator=g) * 3  # non-zero column means
    gy = torch.randn(n, C, generator=g)
    bn_ref = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn_ref.weight.uniform_(0.5, 1.5)
        bn_ref.bias.uniform_(-0.5, 0.5)
    bn_dev = torch.nn.BatchNorm1d(C).to(DEV)
    bn_dev.load_state_dict(bn_ref.state_dict())
    for training in (True, False):
        bn_ref.train(training)
        bn_dev.train(training)
        xr = x.clone().requires_grad_(True)
        xd = x.to(DEV).requires_grad_(True)
        yr = bn_ref(xr)
        yr = torch.relu(yr) if relu else yr
        yd = ops.bn_act(xd, bn_dev, relu=relu, p=0.0)
        close(yd, yr, rtol=1e-4, atol_scale=1e-5, msg=f"fwd training={training}")
        bn_ref.zero_grad()
        bn_dev.zero_grad()
        yr.backward(gy)
        yd.backward(gy.to(DEV))
        close(xd.grad, xr.grad, rtol=1e-3, atol_scale=1e-4, msg=f"dx training={training}")
        close(bn_dev.weight.grad, bn_ref.weight.grad, rtol=1e-3, atol_scale=1e-4)
        close(bn_dev.bias.grad, bn_ref.bias.grad, rtol=1e-3, atol_scale=1e-4)
        close(bn_dev.running_mean, bn_ref.running_mean, rtol=1e-5, atol_scale=1e-6)
        close(bn_dev.running_var, bn_ref.running_var, rtol=1e-4, atol_scale=1e-6)
        assert int(bn_dev.num_batches_tracked) == int(bn_ref.num_batches_tracked)


@pytest.mark.parametrize("n,C,S,relu,p", [(5000, 256, 1200, True, 0.0), (777, 128, 777, True, 0.0), (9000, 256, 64, False, 0.0),
                                         (6000, 256, 2000, True, 0.4)])
def test_fused_bn_act_on_picked_rows_equals_the_full_call_indexed(n, C, S, relu, p):
    """ops.bn_act(..., pick=idx) == ops.bn_act(...)[idx] in value, in dx / dgamma / dbeta, in the bias-gradient tag and in the module
    state (what the projection heads of the sampled criteria use, gnn.py:296-306 -> criterion.py:62-65,134-137)."""
    g = torch.Generator().manual_seed(n + S)
    x = (torch.randn(n, C, generator=g) * 2 + torch.randn(C, generator=g) * 3).to(DEV)
    idx = torch.randperm(n, generator=g)[:S].to(DEV)
    gy = torch.randn(S, C, generator=g).to(DEV)
    bns = []
    for _ in range(2):
        bn = torch.nn.BatchNorm1d(C).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.5, 0.5, C))
        bns.append(bn)
    for training in (True, False):
        outs = []
        for k, bn in enumerate(bns):
            bn.train(training)
            bn.zero_grad()
            xk = x.clone().requires_grad_(True)
            torch.manual_seed(99)                       # same dropout seed for both calls
            if k == 0:
                y = ops.bn_act(xk, bn, relu=relu, p=p, training=True if p > 0 else None)[idx]
            else:
                y = ops.bn_act(xk, bn, relu=relu, p=p, training=True if p > 0 else None, pick=idx)
            assert y.shape == (S, C)
            y.backward(gy)
            outs.append((y.detach(), xk.grad, bn.weight.grad.clone(), bn.bias.grad.clone(), bn.running_mean.clone(), bn.running_var.clone()))
        (y0, dx0, dg0, db0, rm0, rv0), (y1, dx1, dg1, db1, rm1, rv1) = outs
        assert torch.equal(y0, y1), f"forward rows differ (training={training})"
        close(dx1, dx0, rtol=2e-5, atol_scale=2e-6, msg=f"dx training={training}")
        close(dg1, dg0, rtol=2e-5, atol_scale=2e-6, msg="dgamma")
        close(db1, db0, rtol=2e-5, atol_scale=2e-6, msg="dbeta")
        assert torch.equal(rm0, rm1) and torch.equal(rv0, rv1)
    # the column sums of dx (gradient of a bias in front of the BatchNorm) carried by the tag: mathematically 0 with batch statistics
    bn = bns[1]
    bn.train(True)
    lin = torch.nn.Linear(C, C).to(DEV)
    xin = torch.randn(n, C, generator=g).to(DEV)
    y = ops.bn_act(ops.linear(xin, lin.weight, lin.bias), bn, relu=relu, p=0.0, pick=idx)
    y.backward(gy)
    ref_scale = float(gy.abs().sum(0).max())
    assert float(lin.bias.grad.abs().max()) <= 1e-4 * ref_scale


@pytest.mark.parametrize("n,C,Ks,p,dense_consumer,tap", [(9000, 256, 40, 0.5, False, True), (5000, 128, 40, 0.0, True, True),
                                                         (4100, 256, 47, 0.3, False, False), (700, 64, 7, 0.0, True, False)])
def test_bn_act_linear_equals_the_three_separate_ops(n, C, Ks, p, dense_consumer, tap):
    """ops.bn_act_linear == bn_act -> grad_tap -> matmul: values, and every gradient when h also feeds linear_rows (tap rows) and / or a
    dense consumer (the last hidden layer of the GCN student, gnn.py:47-52,150)."""
    g = torch.Generator().manual_seed(n + Ks)
    x0 = (torch.randn(n, C, generator=g) * 2 + torch.randn(C, generator=g)).to(DEV)
    w0 = (torch.randn(C, Ks, generator=g) * 0.1).to(DEV)
    wp0 = (torch.randn(32, C, generator=g) * 0.1).to(DEV)
    idx = torch.randperm(n, generator=g)[: n // 2].to(DEV)
    g_xw = torch.randn(n, Ks, generator=g).to(DEV)
    g_rows = torch.randn(idx.numel(), 32, generator=g).to(DEV)
    res = []
    for fused in (False, True):
        bn = torch.nn.BatchNorm1d(C).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.5, 0.5, C))
        x = x0.clone().requires_grad_(True)
        w = w0.clone().requires_grad_(True)
        wp = wp0.clone().requires_grad_(True)
        torch.manual_seed(7)
        if fused:
            both = ops.bn_act_linear(x, bn, w, relu=True, p=p, training=True)
            assert both is not None
            h, xw = both
        else:
            h = ops.grad_tap(ops.bn_act(x, bn, relu=True, p=p, training=True))
            xw = ops.matmul(h, w)
        loss = (xw * g_xw).sum()
        if tap:
            loss = loss + (ops.linear_rows(h, idx, wp) * g_rows).sum()
        if dense_consumer:
            loss = loss + (h * h).sum() * 0.01
        loss.backward()
        res.append((h.detach(), xw.detach(), x.grad, w.grad, wp.grad if tap else None, bn.weight.grad, bn.bias.grad))
    a, b = res
    assert torch.equal(a[0], b[0])                          # h: the same per-element arithmetic
    close(b[1], a[1], rtol=2e-5, atol_scale=2e-6, msg="xw")    # the fused forward adds the k-ranges in another order
    for name, u, v in zip(("dx", "dW", "dWp", "dgamma", "dbeta"), a[2:], b[2:]):
        if u is not None:
            close(v, u, rtol=2e-5, atol_scale=2e-6, msg=name)


def test_gcn_train_step_with_the_fused_tail_equals_the_separate_ops():
    """models.GCN.forward with ops.bn_act_linear for the last hidden layer vs the composed path: same logits, same parameter gradients."""
    d = D.arxiv_like(scale=0.04, seed=5, with_teacher=False)
    x, adj, y, tr = d.x.to(DEV), d.adj_t.to(DEV), d.y.to(DEV), d.split_idx["train"].to(DEV)
    grads = []
    for fused in (False, True):
        prev = PM._FUSED_TAIL
        PM._FUSED_TAIL = fused
        try:
            torch.manual_seed(3)
            model = PM.GCN(d.num_features, 256, d.num_classes, 3, 0.5).to(DEV)
            proj = PM.make_projection(256, 64).to(DEV)
            model.train(), proj.train()
            torch.manual_seed(11)
            out = model(x, adj)
            f = proj.forward_rows(model.out_feat, tr)
            loss = ops.cross_entropy(out, y.view(-1), tr) + (f * f).mean()
            loss.backward()
            named = list(model.named_parameters()) + list(proj.named_parameters())
            grads.append((out.detach(), [(k, q.grad.clone()) for k, q in named]))
        finally:
            PM._FUSED_TAIL = prev
    close(grads[1][0], grads[0][0], rtol=2e-5, atol_scale=2e-6, msg="logits")
    for (k, u), (_, v) in zip(grads[0][1], grads[1][1]):
        if k in ("convs.0.bias", "convs.1.bias", "0.bias"):
            continue   # a bias in front of a BatchNorm: its gradient is rounding noise around 0
        close(v, u, rtol=5e-5, atol_scale=5e-6, msg=k)


def test_fused_bn_dropout_mask_is_consistent_and_unbiased():
    n, C, p = 20000, 256, 0.5
    torch.manual_seed(0)
    x = torch.randn(n, C, device=DEV, requires_grad=True)
    bn = torch.nn.BatchNorm1d(C).to(DEV)
    torch.manual_seed(123)
    y = ops.bn_act(x, bn, relu=True, p=p, training=True)
    torch.manual_seed(123)
    bn2 = torch.nn.BatchNorm1d(C).to(DEV)
    y2 = ops.bn_act(x.detach(), bn2, relu=True, p=p, training=True)
    assert torch.equal(y, y2), "same host seed => same mask"
    ref = torch.relu(torch.nn.functional.batch_norm(x.detach(), None, None, bn.weight, bn.bias, True, 0.0, bn.eps))
    kept = y != 0
    pos = ref > 0
    frac = kept.sum().item() / pos.sum().item()
    assert abs(frac - (1 - p)) < 0.01, frac
    close(y[kept], ref[kept] / (1 - p), rtol=1e-4, atol_scale=1e-5)
    # E[y] = relu(bn(x)) : column means agree to sampling error
    assert abs(float(y.mean()) - float(ref.mean())) < 5e-3
    # backward: zero exactly where the output was dropped / clipped ... through the BN statistics, so test via a probe
    y.sum().backward()
    assert torch.isfinite(x.grad).all()
    # eval mode: no dropout, running statistics
    bn.eval()
    ye = ops.bn_act(x.detach(), bn, relu=True, p=p)
    close(ye, torch.relu(bn(x.detach())), rtol=1e-4, atol_scale=1e-5)


# ------------------------------------------------------------------------------------------------
# BASELINE.json configs[0]: PPI 2-layer GCN student, logit-KD, mini-batch = one graph (ppi_pyg/gnn.py:185-274)
# ------------------------------------------------------------------------------------------------
def test_ppi_gcn_kd_steps_vs_oracle():
    train, _, _ = D.ppi_like(seed=1, n_train=3, total_train_nodes=2400)
    torch.manual_seed(0)
    om = OM.GCN(50, 64, 121, 2, 0.0, cached=False)
    pm = PM.GCN(50, 64, 121, 2, 0.0, cached=False).to(DEV)
    pm.load_state_dict(om.state_dict())
    oo, po = torch.optim.Adam(om.parameters(), lr=0.005), torch.optim.Adam(pm.parameters(), lr=0.005)
    for g in train:  # one optimisation step per graph, edge_index LongTensor input, BCE-with-logits KD
        om.train(); pm.train()
        ref = OC.ppi_kd_criterion(om(g.x, g.edge_index), g.y, g.teacher_logits, 0.5, 1.0)
        oo.zero_grad(); ref[0].backward(); oo.step()
        out = E.ppi_kd_criterion(pm(g.x.to(DEV), g.edge_index.to(DEV)), g.y.to(DEV), g.teacher_logits.to(DEV), 0.5, 1.0)
        po.zero_grad(); out[0].backward(); po.step()
        for a, b in zip(out, ref):
            close(a, b, rtol=2e-4, atol_scale=0)
    om.eval(); pm.eval()
    g = train[0]
    with torch.no_grad():
        lo, lp = om(g.x, g.edge_index), pm(g.x.to(DEV), g.edge_index.to(DEV))
    # micro-F1 inputs (ppi_pyg/gnn.py:285-288): predictions (out > 0) agree except on numerically-zero logits
    agree = ((lo > 0) == (lp.cpu() > 0)).float().mean()
    assert agree > 0.999


def test_mag_shaped_mean_aggregation_properties():
    """BASELINE.json configs[4] kernel: SAGE-mean aggregation on a MAG-shaped graph (mag_pyg/gnn.py:162), scaled."""
    d = D.mag_like(scale=0.05, seed=0)
    adj = d.adj_t.to(DEV)
    x = d.x.to(DEV)
    y, _ = ops.spmm_raw(adj, x, "mean")
    rowptr, col, _ = adj.csr()
    cnt = (rowptr[1:] - rowptr[:-1]).float()
    ysum, _ = ops.spmm_raw(adj, x, "sum")
    close(y * cnt.clamp(min=1).unsqueeze(1), ysum, rtol=1e-5)
    for r in (0, int(torch.argmax(cnt)), d.num_nodes - 1):
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        ref = x[col[s:e]].double().mean(0) if e > s else torch.zeros(x.shape[1], dtype=torch.float64, device=DEV)
        close(y[r], ref, rtol=1e-5)


@pytest.mark.parametrize("unit_rows", [True, False])
@pytest.mark.parametrize("Sr,Sc,off,P", [(100, 300, 37, 48), (256, 2048, 1024, 256), (77, 77, 0, 20), (513, 1100, 587, 128)])
def test_nce_row_block_kernels_vs_torch(Sr, Sc, off, P, unit_rows):
    """The sharded G-CRD pieces (egnn_nce_block_*): a rank's Sr rows against all Sc teacher rows, positives at i+off.
    Both forms of the saved score matrix: logits (general) and exp(logit - 1.0001/tau) (unit rows)."""
    g = torch.Generator().manual_seed(Sr + Sc)
    f = torch.nn.functional.normalize(torch.randn(Sr, P, generator=g), dim=-1)
    t = torch.nn.functional.normalize(torch.randn(Sc, P, generator=g) + 0.1, dim=-1)
    tau, S_total = 0.075, 4096
    fd, td = f.double().requires_grad_(True), t.double().requires_grad_(True)
    z = fd @ td.t() / tau
    lse = torch.logsumexp(z, dim=1)
    loss_ref = (lse - z[torch.arange(Sr), torch.arange(Sr) + off]).sum() / S_total
    loss_ref.backward()
    Z, lse_k, loss = ops.nce_block_fwd(f.to(DEV), t.to(DEV), off, tau, 1.0 / S_total, unit_rows=unit_rows)
    close(loss[0], loss_ref, rtol=2e-5, atol_scale=0)
    close(lse_k, lse, rtol=1e-5, atol_scale=1e-6)
    saves_exp = bool(_lib.load().egnn_nce_saves_exp(tau, int(unit_rows)))
    assert saves_exp == unit_rows
    if saves_exp:
        shift = float(np.float32(np.float32(1.0) / np.float32(tau)) * np.float32(1.0001))
        close(Z, torch.exp(z - shift), rtol=1e-4, atol_scale=1e-6)
    else:
        close(Z, z, rtol=1e-5, atol_scale=1e-6)
    gscale = torch.tensor([0.7], device=DEV)
    df, dt = ops.nce_block_bwd(f.to(DEV), t.to(DEV), off, 1.0 / (S_total * tau), Z, lse_k, gscale, tau, unit_rows=unit_rows)
    close(df, 0.7 * fd.grad, rtol=1e-4, atol_scale=2e-5)
    close(dt, 0.7 * td.grad, rtol=1e-4, atol_scale=2e-5)
    # the same backward without a workspace (no split-K; smaller row tiles) must agree
    df2, dt2 = torch.empty_like(df), torch.empty_like(dt)
    fg, tg = f.to(DEV), t.to(DEV)
    rc = _lib.load().egnn_nce_block_bwd_f32(_lib.ptr(fg), P, _lib.ptr(tg), P, Sr, Sc, off, P, tau, 1.0 / (S_total * tau), int(unit_rows),
                                            _lib.ptr(Z), _lib.ptr(lse_k), _lib.ptr(gscale), _lib.ptr(df2), P, _lib.ptr(dt2), P,
                                            None, 0, _lib.stream())
    assert rc == 0
    close(df2, df, rtol=1e-5, atol_scale=2e-6)
    close(dt2, dt, rtol=1e-5, atol_scale=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("gnn,mode", [("gcn", "nce"), ("sage", "kd"), ("gcn", "gpw"), ("sage", "lpw")])
def test_sharded_path_with_one_rank_over_rccl_matches_single_gpu_path(gnn, mode):
    """The node-range sharded code (dist.py: halo plan, SyncBN, row-block G-CRD, gathered-sample GSP, train-subgraph LSP,
    flat gradient all-reduce) on the real RCCL backend with world_size 1 must reproduce the single-GPU step; the
    N = 2 / 3 / 4 logic is covered on gloo."""
    import torch.distributed as dist
    import efficient_gnns_amd.dist as DD
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29577", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        hp = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=256, kernel="rbf")
        if mode in ("gpw", "lpw"):
            hp.update(kernel="cosine", beta=100.0)
        d = D.arxiv_like(scale=0.02, seed=5)
        edge_index = None
        if mode == "lpw":   # gnn.py:246-250
            from efficient_gnns_amd.utils import subgraph
            edge_index = subgraph(d.split_idx["train"].to(DEV), torch.stack(d.adj_t.to(DEV).coo()[:2]), relabel_nodes=True,
                                  num_nodes=d.num_nodes)[0]

        def build():
            torch.manual_seed(0)
            np.random.seed(0)
            model = (PM.GCN if gnn == "gcn" else PM.SAGE)(d.num_features, 64, d.num_classes, 3, 0.0).to(DEV)
            sp = tp = None
            groups = [{"params": model.parameters(), "lr": 0.01}]
            if mode in ("nce", "gpw"):
                sp, tp = PM.make_projection(64, 32).to(DEV), PM.make_projection(750, 32).to(DEV)
                groups += [{"params": sp.parameters(), "lr": 0.01}, {"params": tp.parameters(), "lr": 0.01}]
            return model, sp, tp, groups

        model, sp, tp, groups = build()
        opt = torch.optim.Adam(groups)
        adj = d.adj_t.to(DEV)
        x, y = d.x.to(DEV), d.y.to(DEV)
        split = {k: v.to(DEV) for k, v in d.split_idx.items()}
        ref_logits, ref_accs = PM.evaluate(model, x, adj, y, split)
        ref = [PM.train_step(model, x, adj, y, split["train"], opt, mode, hp, d.teacher_out_feat.to(DEV), d.teacher_logits.to(DEV),
                             sp, tp, edge_index) for _ in range(3)]

        model, sp, tp, groups = build()
        for m in (model, sp, tp):
            if m is not None:
                DD.swap_batchnorm(m)
        opt = torch.optim.Adam(groups)
        prob = DD.ShardedProblem(d, 1, 0, DEV, None, need_gcn=(gnn == "gcn"))
        out, accs = DD.sharded_evaluate(model, prob)
        got = [DD.sharded_train_step(model, prob, opt, mode, hp, sp, tp) for _ in range(3)]
        close(out, ref_logits, rtol=1e-4, atol_scale=1e-5)
        np.testing.assert_allclose(accs, ref_accs, atol=1e-9)
        np.testing.assert_allclose(np.array(got), np.array(ref), rtol=2e-4, atol=1e-6)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("gnn,mode", [("gcn", "nce"), ("sage", "kd"), ("sage", "lpw"), ("gcn", "nce+static"), ("gcn", "gpw+static")])
def test_sharded_epoch_captured_as_a_graph_replays_the_eager_steps(gnn, mode):
    """dist.ShardedGraphedEpoch (one rank over RCCL): the captured epoch -- collectives included -- reproduces the eager sharded
    steps (same host draw, dropout 0).  Runs in its own interpreter (tools/checks/sharded_graph_check.py), as bench.py does: a
    process that has captured RCCL work into a graph keeps communicator threads alive that must not sit next to later,
    unrelated captures of the same test process."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # "+static": the fixed-capacity sample layout the multi-rank runs capture (dist.StaticSample), exercised on this one rank
    extra = ["--static"] if mode.endswith("+static") else []
    mode = mode.split("+")[0]
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "checks", "sharded_graph_check.py"), "--gnn", gnn, "--mode", mode] + extra,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    assert "SHARDED-GRAPH-OK" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("n,N,M,K", [(40000, 750, 256, 20011), (30000, 256, 512, 16384), (25000, 100, 256, 17000)])
def test_weight_gradient_against_constant_rows_cut_once_into_planes(n, N, M, K):
    """egnn_gemm_tn_planes_{pack,}_f32 (ops._dw_const_rows): dW = dY^T x[idx] for a constant x whose gathered rows were cut once
    into bf16 planes -- against a float64 product (error unit sum_k |a_k b_k|, the bar of the split-pipeline accuracy test) and
    against the generic gather-fused GEMM; ragged K (zero planes past the end, clamped dY rows), padded columns dropped, a second
    call reuses the cached planes, an in-place change of x rebuilds them."""
    g = torch.Generator().manual_seed(n + N)
    x = ops.pad_pitch((torch.randn(n, N, generator=g) * torch.exp2(torch.randint(-4, 4, (n, N), generator=g).float())).to(DEV))
    idx = torch.randperm(n, generator=g)[:K].to(DEV)
    gy = (torch.randn(K, M, generator=g) * torch.exp2(torch.randint(-4, 4, (K, M), generator=g).float())).to(DEV)
    got = ops._dw_const_rows(gy, x, idx)
    assert got is not None and got.shape == (M, N)
    A, B = gy.double().t().cpu(), x[idx].double().cpu()
    ref = A @ B
    unit = A.abs() @ B.abs()
    err = ((got.double().cpu() - ref).abs() / unit)
    assert float(err.mean()) < 1.2e-7 and float(err.max()) < 2e-6, (float(err.mean()), float(err.max()))
    generic = ops.gemm_raw(gy, x, True, False, b_rows=idx)
    close(got, generic, rtol=1e-5, atol_scale=1e-6)
    n_cached = len(ops._CONST_PLANES)
    again = ops._dw_const_rows(gy, x, idx)
    assert torch.equal(again, got) and len(ops._CONST_PLANES) == n_cached, "planes reused, fixed summation order"
    x.mul_(2.0)                                  # a new version of x: the planes are rebuilt
    close(ops._dw_const_rows(gy, x, idx), got * 2.0, rtol=1e-6, atol_scale=1e-7)
    # through autograd: the teacher head's Linear over constant features -- forward on the planes x planes form, backward as above
    w = (torch.randn(M, N, generator=g) * 0.05).to(DEV).requires_grad_(True)
    b = torch.randn(M, generator=g).to(DEV).requires_grad_(True)
    y = ops.linear_rows(x, idx, w, b)
    Y64 = x[idx].double().cpu() @ w.detach().double().cpu().t()
    uy = x[idx].double().cpu().abs() @ w.detach().double().cpu().abs().t()
    ey = (y.detach().double().cpu() - b.detach().double().cpu() - Y64).abs() / uy
    assert float(ey.mean()) < 1.2e-7 and float(ey.max()) < 2e-6, (float(ey.mean()), float(ey.max()))
    close(y, ops.gemm_raw(x, ops.pad_pitch(w.detach()), False, True, b.detach(), a_rows=idx), rtol=1e-5, atol_scale=1e-6)
    y.backward(gy)
    close(w.grad, ops.gemm_raw(gy, x, True, False, b_rows=idx), rtol=1e-5, atol_scale=1e-6)
    close(b.grad, gy.sum(0), rtol=1e-5, atol_scale=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,P,m,padded", [(1000, 750, 256, 400, True), (1000, 750, 256, 400, False), (513, 64, 40, 513, True),
                                           (3000, 256, 128, 1, True), (700, 130, 72, 300, False)])
def test_linear_rows_fused_gather_gemm_vs_torch(n, C, P, m, padded):
    """egnn_gemm_rows_f32: F.linear(x[idx], W, b) and its gradients with the gather fused into the operand loads, for
    16-byte-aligned row pitches (float4 path) and for odd pitches (scalar path)."""
    g = torch.Generator().manual_seed(n + C)
    x = torch.randn(n, C, generator=g)
    w = torch.randn(P, C, generator=g) * 0.1
    b = torch.randn(P, generator=g)
    idx = torch.randperm(n, generator=g)[:m]
    gy = torch.randn(m, P, generator=g)
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = torch.nn.functional.linear(xd[idx], wd, bd)
    ref.backward(gy.double())
    xg = x.to(DEV)
    if padded:
        xg = ops.pad_pitch(xg)
        assert xg.stride(0) % 4 == 0 and xg.shape == (n, C)
    xg.requires_grad_(True)
    wg, bg = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.linear_rows(xg, idx.to(DEV), wg, bg)
    y.backward(gy.to(DEV))
    close(y, ref, rtol=1e-5, atol_scale=1e-6)
    close(wg.grad, wd.grad, rtol=1e-5, atol_scale=1e-6)
    close(bg.grad, bd.grad, rtol=1e-5, atol_scale=1e-6)
    close(xg.grad, xd.grad, rtol=1e-5, atol_scale=1e-6)


@pytest.mark.gpu
def test_constant_operand_planes_are_an_explicit_opt_in():
    """``linear_rows`` builds the 6-bytes-per-element plane image of ``x[idx]`` only when the caller SAYS the input
    is constant (``const_input=True``: the teacher head).  A large activation under ``no_grad`` (requires_grad False as well) or with
    autograd off must leave both plane caches untouched; with the flag the two routes agree and the image is reused."""
    g = torch.Generator().manual_seed(11)
    n, C, P, m = 20000, 264, 128, 16640
    x = torch.randn(n, C, generator=g).to(DEV)
    w = (torch.randn(P, C, generator=g) * 0.1).to(DEV).requires_grad_(True)
    b = torch.randn(P, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randperm(n, generator=g)[:m].to(DEV)
    before = (len(ops._CONST_PLANES), len(ops._CONST_ROW_PLANES))
    with torch.no_grad():
        y0 = ops.linear_rows(x, idx, w, b)
    y1 = ops.linear_rows(x, idx, w, b)
    y1.sum().backward()
    gw1 = w.grad.clone()
    assert (len(ops._CONST_PLANES), len(ops._CONST_ROW_PLANES)) == before, "no plane image without the flag"
    w.grad = None
    y2 = ops.linear_rows(x, idx, w, b, const_input=True)
    y2.sum().backward()
    assert len(ops._CONST_ROW_PLANES) == before[1] + 1
    close(y2, y1, rtol=1e-5, atol_scale=1e-6)
    close(w.grad, gw1, rtol=1e-5, atol_scale=1e-6)
    assert torch.equal(y0, y1)
    n_now = (len(ops._CONST_PLANES), len(ops._CONST_ROW_PLANES))
    ops.linear_rows(x, idx, w, b, const_input=True)
    assert (len(ops._CONST_PLANES), len(ops._CONST_ROW_PLANES)) == n_now, "image reused"
    # a tensor that takes part in autograd is never treated as constant, whatever the flag says
    xr = x.clone().requires_grad_(True)
    ops.linear_rows(xr, idx, w, b, const_input=True).sum().backward()
    assert (len(ops._CONST_PLANES), len(ops._CONST_ROW_PLANES)) == n_now and xr.grad is not None


@pytest.mark.gpu
def test_native_graph_construction_edge_cases_bit_exact():
    """egnn_csr_from_coo_i64 / egnn_csr_transpose_i64 against the oracle: duplicates kept (ToSparseTensor) or merged
    (to_symmetric), self loops, isolated nodes, a single edge, an empty edge list, a rectangular transpose with values."""
    n = 37
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, n - 5, (400,), generator=g)          # nodes n-5 .. n-1 stay isolated
    dst = torch.randint(0, n - 5, (400,), generator=g)
    src[:20], dst[:20] = dst[20:40].clone(), src[20:40].clone()  # reverse duplicates
    src[40:60] = dst[40:60]                                      # self loops
    src[60:80], dst[60:80] = src[80:100].clone(), dst[80:100].clone()   # exact duplicates
    for ei in (torch.stack([src, dst]), torch.tensor([[3], [7]]), torch.zeros(2, 0, dtype=torch.int64)):
        o = OS.to_sparse_tensor(ei, n)
        p = E.to_sparse_tensor(ei.to(DEV), n)
        assert p.nnz() == ei.shape[1]
        for a, b in zip(p.csr()[:2], o.csr()[:2]):
            assert torch.equal(a.cpu(), b)
        so, sp = o.to_symmetric(), p.to_symmetric()
        for a, b in zip(sp.csr()[:2], so.csr()[:2]):
            assert torch.equal(a.cpu(), b)
        assert torch.equal(sp.storage.colptr().cpu(), so._colptr()) and torch.equal(sp.storage.csr2csc().cpu(), so._csr2csc())
    # rectangular, valued: the transposed tensor carries value[csr2csc]
    rows = torch.sort(torch.randint(0, 11, (90,), generator=g)).values
    cols = torch.randint(0, 23, (90,), generator=g)
    val = torch.randn(90, generator=g)
    o, p = make_pair(rows, cols, val, (11, 23))
    ot, pt = o.t(), p.t()
    for a, b in zip(pt.csr(), ot.csr()):
        assert torch.equal(a.cpu(), b)


# ------------------------------------------------------------------------------------------------
# the frozen GAT teacher the PPI train loop runs inside every student step (ppi_pyg/gnn.py:208-209)
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("heads,concat,C,sparse_input", [(4, True, 32, False), (6, False, 121, False), (1, True, 8, True), (3, True, 20, True)])
def test_gatconv_inference_vs_oracle(heads, concat, C, sparse_input):
    g = torch.Generator().manual_seed(heads * 7 + C)
    n, F_in = 700, 50
    src = torch.randint(0, n - 4, (9000,), generator=g)           # isolated tail nodes keep only their self loop
    dst = torch.cat([torch.randint(0, n - 4, (8000,), generator=g), torch.full((1000,), 11)])   # one hub target
    src[:50] = dst[:50]                                           # self loops in the input are replaced, not doubled
    ei = torch.stack([src, dst])
    x = torch.randn(n, F_in, generator=g)
    torch.manual_seed(1)
    oc = ON.GATConv(F_in, C, heads=heads, concat=concat)
    with torch.no_grad():
        oc.bias.uniform_(-0.1, 0.1)
    pc = E.GATConv(F_in, C, heads=heads, concat=concat).to(DEV)
    pc.load_state_dict(oc.state_dict())
    oc.eval(); pc.eval()
    adj_o = OS.to_sparse_tensor(ei, n) if sparse_input else ei
    adj_p = E.to_sparse_tensor(ei.to(DEV), n) if sparse_input else ei.to(DEV)
    with torch.no_grad():
        ref, out = oc(x, adj_o), pc(x.to(DEV), adj_p)
    close(out, ref, rtol=1e-5, atol_scale=1e-5)
    with pytest.raises(NotImplementedError):                      # teacher training is out of scope: no silent wrong gradients
        pc(x.to(DEV), adj_p)


@pytest.mark.gpu
def test_ppi_teacher_models_match_reference_golden_and_oracle(golden_ppi_teacher):
    G = golden_ppi_teacher
    x, ei = as_t(G["in_x"], DEV), as_t(G["in_edge_index"], DEV)
    m = PM.GAT(x.shape[1], 6, G["gat_logits"].shape[1], 3, 0.5, heads=2).to(DEV)
    m.load_state_dict({k[len("gat_param__"):]: as_t(G[k], DEV) for k in G.files if k.startswith("gat_param__")})
    m.eval()
    with torch.no_grad():
        y = m(x, ei)
    close(y, G["gat_logits"], rtol=1e-5, atol_scale=1e-5)
    close(m.out_feat, G["gat_out_feat"], rtol=1e-5, atol_scale=1e-5)
    # TeacherNet (4 x 256, 6-head output layer) on a PPI-shaped graph against the oracle with the same weights
    train, _, _ = D.ppi_like(seed=2, n_train=1, total_train_nodes=1500)
    gph = train[0]
    torch.manual_seed(0)
    ot = OM.TeacherNet(50, 121)
    pt = PM.TeacherNet(50, 121).to(DEV)
    pt.load_state_dict(ot.state_dict())
    ot.eval(); pt.eval()
    with torch.no_grad():
        ref, out = ot(gph.x, gph.edge_index), pt(gph.x.to(DEV), gph.edge_index.to(DEV))
    close(out, ref, rtol=1e-5, atol_scale=1e-5)
    close(pt.out_feat, ot.out_feat, rtol=1e-5, atol_scale=1e-5)


@pytest.mark.gpu
def test_ppi_student_step_with_teacher_forward_inside_vs_oracle():
    """ppi_pyg/gnn.py:205-212: every student step first runs the frozen GAT teacher on the batch graph, then the KD loss."""
    train, _, _ = D.ppi_like(seed=3, n_train=2, total_train_nodes=1800)
    torch.manual_seed(0)
    ot, om = OM.TeacherNet(50, 121), OM.GCN(50, 64, 121, 2, 0.0, cached=False)
    pt, pm = PM.TeacherNet(50, 121).to(DEV), PM.GCN(50, 64, 121, 2, 0.0, cached=False).to(DEV)
    pt.load_state_dict(ot.state_dict()); pm.load_state_dict(om.state_dict())
    ot.eval(); pt.eval()
    oo, po = torch.optim.Adam(om.parameters(), lr=0.005), torch.optim.Adam(pm.parameters(), lr=0.005)
    for gph in train:
        om.train(); pm.train()
        with torch.no_grad():
            t_ref = ot(gph.x, gph.edge_index)
            t_out = pt(gph.x.to(DEV), gph.edge_index.to(DEV))
        ref = OC.ppi_kd_criterion(om(gph.x, gph.edge_index), gph.y, t_ref, 0.5, 1.0)
        oo.zero_grad(); ref[0].backward(); oo.step()
        out = E.ppi_kd_criterion(pm(gph.x.to(DEV), gph.edge_index.to(DEV)), gph.y.to(DEV), t_out, 0.5, 1.0)
        po.zero_grad(); out[0].backward(); po.step()
        for a, b in zip(out, ref):
            close(a, b, rtol=2e-4, atol_scale=0)


# ------------------------------------------------------------------------------------------------
# R-GCN per-relation mean aggregation (mag_pyg/gnn.py:25-68,140-168)
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rgcn_matches_reference_golden(golden_mag_rgcn):
    G = golden_mag_rgcn
    sizes, edge_index_dict, key2int, params, args = mag_rgcn_case(G, DEV)
    m = PM.RGCN(8, 12, 5, 2, 0.5, sizes, [0], 4).to(DEV)
    m.load_state_dict(params)
    m.eval()
    with torch.no_grad():
        y = m(*args)
    inf = m.inference(args[0], edge_index_dict, key2int)
    close(y, G["forward_logits"], rtol=1e-5, atol_scale=1e-5)
    close(m.out_feat, G["forward_out_feat"], rtol=1e-5, atol_scale=1e-5)
    for j, v in inf.items():
        close(v, G[f"inference__{j}"], rtol=1e-5, atol_scale=1e-5)


@pytest.mark.gpu
def test_rgcnconv_forward_backward_vs_oracle():
    """A larger grouped graph: 4 node types, 7 relations (one of them empty), hub targets; values and all gradients."""
    g = torch.Generator().manual_seed(17)
    n, F_in, F_out, NT, ET = 3000, 64, 48, 4, 7
    node_type = torch.randint(0, NT, (n,), generator=g)
    E_ = 40000
    ei = torch.stack([torch.randint(0, n, (E_,), generator=g),
                      torch.cat([torch.randint(0, n, (E_ - 3000,), generator=g), torch.full((3000,), 5)])])
    et = torch.randint(0, ET - 1, (E_,), generator=g)             # relation ET-1 has no edges
    x = torch.randn(n, F_in, generator=g)
    gy = torch.randn(n, F_out, generator=g)
    torch.manual_seed(2)
    oc = ON.RGCNConv(F_in, F_out, NT, ET)
    pc = E.RGCNConv(F_in, F_out, NT, ET).to(DEV)
    pc.load_state_dict(oc.state_dict())
    xo = x.clone().requires_grad_(True)
    xp = x.to(DEV).requires_grad_(True)
    ref = oc(xo, ei, et, node_type)
    out = pc(xp, ei.to(DEV), et.to(DEV), node_type.to(DEV))
    close(out, ref, rtol=1e-5, atol_scale=1e-5)
    ref.backward(gy)
    out.backward(gy.to(DEV))
    close(xp.grad, xo.grad, rtol=1e-4, atol_scale=1e-5)
    for (k, a), (_, b) in zip(pc.named_parameters(), oc.named_parameters()):
        ga = torch.zeros_like(a) if a.grad is None else a.grad      # an unused relation: no gradient == zero gradient
        gb = torch.zeros_like(b) if b.grad is None else b.grad
        close(ga, gb, rtol=1e-4, atol_scale=1e-5, msg=k)


@pytest.mark.gpu
def test_sign_neighbor_averaged_features_vs_oracle():
    """arxiv_dgl/sign.py:175-186: R rounds of mean aggregation over the in-neighbours."""
    d = D.arxiv_like(scale=0.03, seed=4, with_teacher=False)
    import efficient_gnns_amd.transforms as T
    rowptr, col, _ = d.adj_t.csr()
    oadj = OS.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=d.adj_t.sparse_sizes())
    ref = OS.neighbor_average_features(oadj, d.x, 3)
    out = T.neighbor_average_features(d.adj_t.to(DEV), d.x.to(DEV), 3)
    assert len(out) == 4 and torch.equal(out[0].cpu(), d.x)
    for a, b in zip(out[1:], ref[1:]):
        close(a, b, rtol=1e-5, atol_scale=1e-5)


@pytest.mark.gpu
def test_structure_memo_is_not_fooled_by_allocator_address_reuse():
    """GCNConv / GATConv memoise A^ / the attention CSR on the identity of the edge_index tensor.  A different graph of the
    same shape created right after the first one was dropped (the caching allocator would hand out the same address) must
    not hit the old entry: the entries keep their key tensors alive."""
    n = 300
    torch.manual_seed(0)
    og, pg = ON.GCNConv(16, 8, cached=False), E.GCNConv(16, 8, cached=False).to(DEV)
    pg.load_state_dict(og.state_dict())
    oa, pa = ON.GATConv(16, 8, heads=2).eval(), E.GATConv(16, 8, heads=2).to(DEV).eval()
    pa.load_state_dict(oa.state_dict())
    x = torch.randn(n, 16)
    xg = x.to(DEV)
    for seed in range(4):
        g = torch.Generator().manual_seed(seed)
        ei = torch.randint(0, n, (2, 2000), generator=g)
        ei_dev = ei.to(DEV)
        with torch.no_grad():
            close(pg(xg, ei_dev), og(x, ei), rtol=1e-5, atol_scale=1e-5, msg=f"gcn seed {seed}")
            close(pa(xg, ei_dev), oa(x, ei), rtol=1e-5, atol_scale=1e-5, msg=f"gat seed {seed}")
        del ei_dev
    # in-place edits bump the version counter: a new entry, not the stale one
    ei_dev = ei.to(DEV)
    with torch.no_grad():
        pg(xg, ei_dev)
        ei_dev[0, :50] = 0
        ei2 = ei.clone(); ei2[0, :50] = 0
        close(pg(xg, ei_dev), og(x, ei2), rtol=1e-5, atol_scale=1e-5, msg="in-place edit")


# ------------------------------------------------------------------------------------------------
# property-based: SpMM on arbitrary CSR structures (empty rows, self loops, duplicates, hub rows)
# ------------------------------------------------------------------------------------------------
from hypothesis import given, settings, strategies as st  # noqa: E402


@st.composite
def _spmm_cases(draw):
    n_rows = draw(st.integers(1, 60))
    n_cols = draw(st.integers(1, 60))
    e = draw(st.integers(0, 400))
    seed = draw(st.integers(0, 2 ** 16))
    hub = draw(st.booleans())
    K = draw(st.sampled_from([1, 3, 4, 8, 12, 32, 40, 64, 68]))
    reduce = draw(st.sampled_from(["sum", "mean", "max"]))
    valued = draw(st.booleans())
    return n_rows, n_cols, e, seed, hub, K, reduce, valued


@pytest.mark.gpu
@settings(max_examples=60, deadline=None, derandomize=True)
@given(_spmm_cases())
def test_spmm_property_random_structures(case):
    n_rows, n_cols, e, seed, hub, K, reduce, valued = case
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, n_rows, (e,), generator=g)
    cols = torch.randint(0, n_cols, (e,), generator=g)
    if hub and e:
        rows[: (3 * e) // 4] = rows[0]                 # one row holds 3/4 of the entries (> 64 of them when e is large)
    rows, perm = torch.sort(rows, stable=True)
    cols = cols[perm]
    val = torch.randn(e, generator=g) if valued else None
    x = torch.randn(n_cols, K, generator=g)
    gy = torch.randn(n_rows, K, generator=g)
    o, p = make_pair(rows, cols, val, (n_rows, n_cols))
    xo, xp = x.clone().requires_grad_(True), x.to(DEV).requires_grad_(True)
    yo, yp = OS.matmul(o, xo, reduce), p.matmul(xp, reduce)
    close(yp, yo, rtol=1e-5, atol_scale=1e-5, msg=f"fwd {case}")
    yo.backward(gy)
    yp.backward(gy.to(DEV))
    close(xp.grad, xo.grad, rtol=1e-4, atol_scale=1e-5, msg=f"bwd {case}")


@pytest.mark.gpu
def test_plain_c_host_program_drives_the_c_abi(tmp_path):
    """examples/c_abi_spmm.c: a C99 program (gcc, no Python / torch) that allocates with the HIP runtime C API, calls
    egnn_spmm_csr_f32 / egnn_gcn_norm_count_i64 through include/egnn_hip.h and checks them against host loops."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "efficient-gnns_amd", "lib")
    exe = str(tmp_path / "c_abi_spmm")
    cmd = ["gcc", "-std=c99", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(root, "include"),
           os.path.join(root, "examples", "c_abi_spmm.c"), "-L", lib, "-legnn_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "max rel err" in run.stdout and run.stdout.strip().endswith("ok")


@pytest.mark.gpu
def test_sharded_batchnorm_descriptor_pieces_on_simulated_shards():
    """The N > 1 BatchNorm math without N GPUs: rows split into 3 uneven shards (one of them empty), per-shard
    egnn_bn_stats_f32 -> egnn_bn_merge_shards_f32 must equal the full-batch statistics, and per-shard
    egnn_bn_act_bwd_reduce_f32 summed over shards (what the all-reduce does) -> egnn_bn_act_bwd_apply_f32 with 1/N_total
    must equal the single-GPU backward (egnn_bn_act_bwd_f32) on the whole batch."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    n, C = 5000, 64
    x = (torch.randn(n, C, generator=g) * 2.0 + 0.7).to(DEV)
    dy = torch.randn(n, C, generator=g).to(DEV)
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV)
    cuts = [0, 1234, 1234, 5000]                                    # shard 1 is empty
    world = 3
    nws = lib.egnn_bn_ws_floats(C)
    ws = torch.empty(nws, device=DEV)
    stats = torch.zeros(world, 2 * C + 1, device=DEV)
    for w in range(world):
        xs = x[cuts[w]:cuts[w + 1]]
        if xs.shape[0]:
            _lib.check(lib.egnn_bn_stats_f32(_lib.ptr(xs), C, xs.shape[0], C, _lib.ptr(stats[w]), _lib.ptr(stats[w, C:]), _lib.ptr(ws), nws,
                                             _lib.stream()), "stats")
            stats[w, 2 * C] = float(xs.shape[0])
    merged = torch.empty(2 * C + 1, device=DEV)
    _lib.check(lib.egnn_bn_merge_shards_f32(_lib.ptr(stats), world, C, _lib.ptr(merged), _lib.ptr(merged[C:]), _lib.ptr(merged[2 * C:]),
                                            _lib.stream()), "merge")
    mean, var = merged[:C].clone(), merged[C:2 * C].clone()
    assert float(merged[2 * C]) == n
    close(mean, x.double().mean(0), rtol=1e-5, atol_scale=1e-6)
    close(var, x.double().var(0, unbiased=False), rtol=1e-5, atol_scale=1e-6)
    # backward: reference = the single-GPU entry point on the whole batch with the same statistics
    eps, relu, p, seed = 1e-5, 1, 0.0, 0

    def desc(rows):   # egnn_bn_act_t over the rows `rows` of x, every row an output row
        return ctypes.byref(_lib.BnAct(_lib.ptr(rows), C, rows.shape[0], C, _lib.ptr(mean), _lib.ptr(var), eps, _lib.ptr(gamma), _lib.ptr(beta),
                                       relu, p, seed, None, None, 0))
    dg_ref, db_ref, dx_ref = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty_like(x)
    _lib.check(lib.egnn_bn_act_bwd_f32(desc(x), _lib.ptr(dy), C, 1, _lib.ptr(dg_ref), _lib.ptr(db_ref), _lib.ptr(dx_ref), C, None, _lib.ptr(ws), nws,
                                       _lib.stream()), "bwd")
    total = torch.zeros(2 * C, device=DEV)                           # [dbeta | dgamma] summed over the shards
    for w in range(world):
        xs, ds = x[cuts[w]:cuts[w + 1]], dy[cuts[w]:cuts[w + 1]]
        if xs.shape[0]:
            part = torch.empty(2 * C, device=DEV)
            _lib.check(lib.egnn_bn_act_bwd_reduce_f32(desc(xs), _lib.ptr(ds), C, _lib.ptr(part[C:]), _lib.ptr(part), _lib.ptr(ws), nws,
                                                      _lib.stream()), "reduce")
            total += part
    close(total[:C], db_ref, rtol=1e-4, atol_scale=1e-5)
    close(total[C:], dg_ref, rtol=1e-4, atol_scale=1e-5)
    dx = torch.empty_like(x)
    for w in range(world):
        xs, ds = x[cuts[w]:cuts[w + 1]], dy[cuts[w]:cuts[w + 1]]
        if xs.shape[0]:
            _lib.check(lib.egnn_bn_act_bwd_apply_f32(desc(xs), _lib.ptr(ds), C, _lib.ptr(total), _lib.ptr(total[C:]), 1.0 / n, None,
                                                     _lib.ptr(dx[cuts[w]:cuts[w + 1]]), C, None, None, 0, _lib.stream()), "apply")
    close(dx, dx_ref, rtol=1e-4, atol_scale=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["kd", "supervised"])
def test_ppi_epochs_match_reference_train_loop_golden(golden_ppi_train, mode):
    """models.ppi_train_epoch / ppi_test on the GPU against the records of the reference's own ppi_pyg train() / test()."""
    G = golden_ppi_train
    graphs, teacher_sd, init = ppi_train_case(G, DEV)
    F_in, Cn = graphs[0].x.shape[1], graphs[0].y.shape[1]
    teacher = PM.GAT(F_in, 6, Cn, 3, 0.0, heads=2).to(DEV)
    teacher.load_state_dict(teacher_sd)
    teacher.requires_grad_(False)
    model = PM.GCN(F_in, 16, Cn, 2, 0.0, cached=False).to(DEV)
    model.load_state_dict(init[mode])
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    hp = dict(alpha=0.5, kd_T=1.0)
    recs = [PM.ppi_train_epoch(model, teacher if mode == "kd" else None, graphs, opt, mode, hp) for _ in range(3)]
    np.testing.assert_allclose(np.array(recs), G[f"{mode}_epoch_losses"], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(PM.ppi_test(model, graphs), float(G[f"{mode}_f1"]), atol=5e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("gnn,mode", [("gcn", "nce"), ("sage", "kd"), ("gcn", "gpw"), ("sage", "lpw")])
def test_graphed_epoch_replays_equal_eager_steps(gnn, mode):
    """models.GraphedEpoch (train step + eval captured once as a hipGraph) against the eager train_step / evaluate from the same
    state and the same NumPy draws: with dropout 0 every replay must reproduce the eager losses and accuracies."""
    d = D.arxiv_like(scale=0.02, seed=6)
    dev = torch.device(DEV)
    x, adj, y = d.x.to(dev), d.adj_t.to(dev), d.y.to(dev)
    split = {k: v.to(dev) for k, v in d.split_idx.items()}
    tf, tl = ops.pad_pitch(d.teacher_out_feat.to(dev)), d.teacher_logits.to(dev)
    hp = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=256, kernel="cosine", proj_dim=32)
    ei = None
    if mode == "lpw":   # gnn.py:246-250: the train-node subgraph; beta of record
        from efficient_gnns_amd.utils import subgraph
        ei = subgraph(split["train"], torch.stack(adj.coo()[:2]), relabel_nodes=True, num_nodes=d.num_nodes)[0]
        hp["beta"] = 100.0

    def build():
        torch.manual_seed(0)
        m = (PM.GCN if gnn == "gcn" else PM.SAGE)(d.num_features, 64, d.num_classes, 3, 0.0).to(dev)
        sp, tp = PM.make_projection(64, 32).to(dev), PM.make_projection(750, 32).to(dev)
        opt = torch.optim.Adam([{"params": m.parameters()}, {"params": sp.parameters()}, {"params": tp.parameters()}], lr=0.01,
                               fused=True, capturable=True)
        return m, sp, tp, opt
    warm, steps = 2, 4
    m1, sp1, tp1, o1 = build()
    np.random.seed(1)
    for _ in range(warm):
        PM.train_step(m1, x, adj, y, split["train"], o1, mode, hp, tf, tl, sp1, tp1, ei)
    np.random.seed(2)
    ref = []
    for _ in range(steps):
        l = PM.train_step(m1, x, adj, y, split["train"], o1, mode, hp, tf, tl, sp1, tp1, ei)
        _, a = PM.evaluate(m1, x, adj, y, split)
        ref.append(l + a)
    m2, sp2, tp2, o2 = build()
    np.random.seed(1)
    ge = PM.GraphedEpoch(m2, x, adj, y, split["train"], o2, mode, hp, tf, tl, sp2, tp2, edge_index=ei, split_idx=split, warmup=warm)
    np.random.seed(2)
    ge.redraw()    # the randomness of a replay is drawn one step ahead: re-draw it under the new seed
    got = []
    for _ in range(steps):
        l, a = ge.step()
        got.append(l + a)
    got, ref = np.array(got), np.array(ref)
    np.testing.assert_allclose(got[:, :3], ref[:, :3], rtol=2e-5, atol=1e-7)
    # accuracies: eval-mode logits after Adam steps are rounding-noise sensitive (biases in front of BatchNorm, see
    # tests/golden/make_golden.py); allow a couple of argmax flips, report how far the parameters really are
    worst = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))
                for (k, a), (_, b) in zip(m2.named_parameters(), m1.named_parameters()) if not noise_driven(k, 3))
    n_small = min(v.numel() for v in split.values())
    np.testing.assert_allclose(got[:, 3:], ref[:, 3:], atol=3.0 / n_small, err_msg=f"max relative parameter distance {worst:.2e}")
    assert worst < 1e-3, worst
    assert PC._ROW_SAMPLER is None and ops._DROPOUT_SEED_DEV is None, "the capture hooks must not leak into eager code"


@pytest.mark.gpu
def test_graphed_epoch_draws_fresh_dropout_masks_and_samples():
    """Replays are not frozen: the device-side dropout seed and the sampled-row buffer change before every replay."""
    d = D.arxiv_like(scale=0.02, seed=7)
    dev = torch.device(DEV)
    x, adj, y = d.x.to(dev), d.adj_t.to(dev), d.y.to(dev)
    split = {k: v.to(dev) for k, v in d.split_idx.items()}
    tf, tl = ops.pad_pitch(d.teacher_out_feat.to(dev)), d.teacher_logits.to(dev)
    hp = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=128, kernel="cosine", proj_dim=32)
    torch.manual_seed(0)
    m = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.5).to(dev)
    sp, tp = PM.make_projection(64, 32).to(dev), PM.make_projection(750, 32).to(dev)
    opt = torch.optim.Adam([{"params": m.parameters(), "lr": 0.0}, {"params": sp.parameters(), "lr": 0.0},
                            {"params": tp.parameters(), "lr": 0.0}], fused=True, capturable=True)   # lr 0: only the randomness moves
    ge = PM.GraphedEpoch(m, x, adj, y, split["train"], opt, "nce", hp, tf, tl, sp, tp, split_idx=None, warmup=2)
    seen = {ge.step()[0] for _ in range(4)}
    assert len(seen) == 4 and all(np.isfinite(v).all() for v in map(np.array, seen)), seen
    picks = []
    for _ in range(3):
        ge.step()
        picks.append(ge._pick_dev.clone())
    assert not torch.equal(picks[0], picks[1]) and not torch.equal(picks[1], picks[2])


@pytest.mark.gpu
@pytest.mark.parametrize("with_eval", [True, False])
def test_graphed_epoch_step_async_hands_out_the_same_values_one_call_later(with_eval):
    """``GraphedEpoch.step_async`` (replay k is launched before the values of epoch k - 1 are read: no idle GPU between epochs) is the
    same program as ``step``: same replays, same host draws in the same order, dropout 0.5 -- every loss and accuracy BIT-equal, handed
    out one call later; ``drain`` delivers the last epoch; ``step`` refuses to run while an epoch's values are in flight."""
    d = D.arxiv_like(scale=0.02, seed=8)
    dev = torch.device(DEV)
    x, adj, y = d.x.to(dev), d.adj_t.to(dev), d.y.to(dev)
    split = {k: v.to(dev) for k, v in d.split_idx.items()}
    tf, tl = ops.pad_pitch(d.teacher_out_feat.to(dev)), d.teacher_logits.to(dev)
    hp = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=256, kernel="cosine", proj_dim=32)

    def run(async_):
        torch.manual_seed(0)
        np.random.seed(3)
        m = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.5).to(dev)
        sp, tp = PM.make_projection(64, 32).to(dev), PM.make_projection(750, 32).to(dev)
        opt = torch.optim.Adam([{"params": list(m.parameters()) + list(sp.parameters()) + list(tp.parameters())}], lr=0.01, fused=True, capturable=True)
        ge = PM.GraphedEpoch(m, x, adj, y, split["train"], opt, "nce", hp, tf, tl, sp, tp, split_idx=split if with_eval else None, warmup=2)
        vals = []
        if not async_:
            return [ge.step() for _ in range(6)]
        assert ge.step_async() is None
        for _ in range(5):
            vals.append(ge.step_async())
        with pytest.raises(RuntimeError, match="drain"):
            ge.step()
        vals.append(ge.drain())
        assert ge.drain() is None
        vals.append(ge.step())          # and the synchronous form continues the same trajectory
        return vals
    ref, got = run(False), run(True)
    assert got[:6] == ref, (got, ref)
    assert np.isfinite(np.array([v[0] for v in got])).all() and len({v[0] for v in got}) == 7


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ARXIV_GAT_CONFIGS))
def test_arxiv_gat_teacher_matches_reference_golden(golden_arxiv_gat, name):
    """The arxiv GAT teacher on the kernels (models.ArxivGAT / nn.DGLGATConv / teacher_evaluate) against the golden recorded
    from the reference's own arxiv_dgl/models.py (three gat.py configurations incl. label reuse)."""
    G = golden_arxiv_gat
    model, adj, x, labels, (tr, va, te), C, iters = arxiv_gat_case(G, PM, E.SparseTensor, name, DEV)
    pred, feat = PM.teacher_evaluate(model, adj, x, labels, tr, va, te, C, use_labels=True, n_label_iters=iters)
    close(pred, G[f"{name}__pred"], rtol=2e-5, atol_scale=2e-6)
    close(feat, G[f"{name}__feat"], rtol=2e-5, atol_scale=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("use_attn_dst,sym", [(False, True), (True, False)])
def test_arxiv_gat_teacher_vs_oracle_and_artifact_files(use_attn_dst, sym, tmp_path):
    """Teacher pipeline at a larger size with the script-of-record width (3 heads x 250: head blocks that are not float4
    aligned): message graph (gat.py:56-71), forward + one label-reuse round, artefact files in the reference's layout read back
    the way arxiv_pyg/gnn.py:278-279 does."""
    import torch.nn.functional as F
    from efficient_gnns_amd.utils import dgl_bidirected_with_self_loops
    d = D.arxiv_like(scale=0.02, seed=9, with_teacher=False)
    n, C = d.num_nodes, d.num_classes
    padj = dgl_bidirected_with_self_loops(d.adj_t.to(DEV))
    rowptr, col, _ = padj.csr()
    rows = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).cpu())
    assert int(((rows == col.cpu()).long()).sum()) == n, "exactly one self loop per node"
    oadj = OS.SparseTensor(rowptr=rowptr.cpu(), col=col.cpu(), sparse_sizes=(n, n))
    torch.manual_seed(3)
    om = OM.ArxivGAT(d.num_features + C, C, 250, 3, 3, F.relu, dropout=0.75, input_drop=0.25, edge_drop=0.3,
                     use_attn_dst=use_attn_dst, use_symmetric_norm=sym)
    pm = PM.ArxivGAT(d.num_features + C, C, 250, 3, 3, F.relu, dropout=0.75, input_drop=0.25, edge_drop=0.3,
                     use_attn_dst=use_attn_dst, use_symmetric_norm=sym).to(DEV)
    pm.load_state_dict(om.state_dict())
    tr, va, te = (d.split_idx[k] for k in ("train", "valid", "test"))
    po, fo = OM.teacher_evaluate(om, oadj, d.x.clone(), d.y, tr, va, te, C, True, 1)
    pp, fp = PM.teacher_evaluate(pm, padj, d.x.to(DEV), d.y.to(DEV), tr.to(DEV), va.to(DEV), te.to(DEV), C, True, 1)
    close(pp, po, rtol=1e-4, atol_scale=2e-5)
    close(fp, fo, rtol=1e-4, atol_scale=2e-5)
    assert fp.shape == (n, 750) and float(fp.min()) >= 0.0          # post-ReLU features, the [N,750] the student reads
    D.save_teacher_artifacts(str(tmp_path), "gat-3L250x3h", 0, fp, pp)
    f2, l2 = D.load_teacher_artifacts(str(tmp_path), "gat-3L250x3h", 0, num_nodes=n, device=DEV)
    assert torch.equal(f2, fp) and torch.equal(l2, pp)


@pytest.mark.gpu
def test_bench_mag_workload_runs_on_one_rank_over_rccl():
    """BASELINE.json configs[4] through bench.py on ONE rank over the real RCCL backend (the sharded code path with an empty
    halo): MAG-shaped graph at 1 % size, SAGE-mean + logit KD; the JSON line carries the roofline of rank 0's aggregation."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "mag", "--scale", "0.01", "--steps", "2", "--warmup", "1",
                          "--gpus", "1"], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert "mag" in line["config"]["workload"] and line["n_gpus"] == 1 and line["value"] > 0
    assert line["roofline"] and line["roofline"]["achieved"] > 0 and all(np.isfinite(line["last_losses"]))


@pytest.mark.gpu
def test_reordered_graph_aggregates_to_the_permuted_result():
    """ToSparseTensor(reorder='community') on the device: the reordered problem is the same problem -- aggregating x[perm] over
    the permuted adjacency equals the permuted aggregation (oracle on the original graph), for GCN values and for SAGE mean."""
    import types
    from efficient_gnns_amd.transforms import ToSparseTensor
    src = D.arxiv_like(scale=0.05, seed=8, with_teacher=False, graph="local")
    rowptr, col, _ = src.adj_t.csr()
    n = src.num_nodes
    rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    data = types.SimpleNamespace(edge_index=torch.stack([col, rows]).to(DEV), x=src.x.to(DEV), y=src.y.to(DEV), num_nodes=n,
                                 split_idx={k: v.to(DEV) for k, v in src.split_idx.items()})
    data = ToSparseTensor(reorder="community")(data)
    perm = data.perm.cpu()
    o = OS.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n))          # the graph is symmetric already
    x = src.x
    close(data.adj_t.matmul(data.x, "mean"), o.matmul(x, "mean")[perm], rtol=1e-5)
    close(E.gcn_norm(data.adj_t).matmul(data.x, "sum"), OS.gcn_norm_sparse(o).matmul(x, "sum")[perm], rtol=1e-5)
    assert torch.equal(data.y.cpu(), src.y[perm])
