"""Weighted adjacency on the GPU (run with ``-m gpu`` on an MI355X): the SDDMM value gradient (egnn_sddmm_csr_f32) through the C ABI,
value gradients through ``ops.spmm``, the valued ``gcn_norm`` and ``GCNConv`` with weights for both input kinds.  References are
float64 on the CPU (dense torch ops and the oracle's helpers).

Bars: the value gradient against the derived bound of a length-K fp32 dot product in any summation order plus the scale's rounding,
|got - ref| <= gamma_(K+2) * sum_k |G[r,k] X[c,k]| * |scale|, gamma_n = n u / (1 - n u), u = 2^-24; layer outputs rtol 1e-5 with
atol = 1e-5 * max|ref| and gradients rtol 1e-4 (the bars of tests/test_gpu_parity.py); normalised values relative error
(d_max + 8) * 2^-23 (a positive sum of d_max terms, one rsqrt, two products)."""
import functools

import numpy as np
import pytest
import torch

import efficient_gnns_amd as E
import efficient_gnns_amd.nn as PN
import efficient_gnns_amd.ops as ops
from efficient_gnns_amd import _lib
from efficient_gnns_amd.sparse import gcn_norm
import oracle.sparse as OS

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def close(actual, ref, rtol=1e-5, atol_scale=1e-5, msg=""):
    """The project's bar (tests/test_gpu_parity.py): rtol plus atol = atol_scale * max|ref|."""
    a, r = actual.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    atol = atol_scale * (np.abs(r).max() if r.size else 0.0) + 1e-30
    np.testing.assert_allclose(a, r, rtol=rtol, atol=atol, err_msg=msg)


def leaf(t):
    """A fresh float32 leaf on the device."""
    return t.detach().to(DEV).clone().requires_grad_(True)


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------
# graphs (built once on the CPU; the tests move them to the device)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rect_graph():
    """37 x 53: rows 0, 9 and 36 empty, 20 duplicate entries, row 17 a hub of 1 500 entries (several 256-entry chunks, ragged tail)."""
    g = torch.Generator().manual_seed(7)
    row = torch.randint(1, 36, (150,), generator=g)
    row = row[(row != 9) & (row != 17)]
    col = torch.randint(0, 53, (row.numel(),), generator=g)
    row = torch.cat([row, row[:20], torch.full((1500,), 17)])
    col = torch.cat([col, col[:20], torch.randint(0, 53, (1500,), generator=g)])
    adj = E.SparseTensor(row=row, col=col, sparse_sizes=(37, 53))
    cnt = adj._rowptr[1:] - adj._rowptr[:-1]
    assert int(cnt[0]) == 0 and int(cnt[9]) == 0 and int(cnt[36]) == 0 and int(cnt[17]) == 1500 and adj.nnz() % 256 != 0
    return adj


@functools.lru_cache(maxsize=None)
def square_graph():
    """67 nodes, COO in (row, col) order with float32 weights in [0.1, 1.1]: stored diagonal entries of weight != 1 (node 4 twice), rows
    without a diagonal, node 66 isolated, row 23 a hub of 1 500 entries (duplicates, some of them on the diagonal)."""
    g = torch.Generator().manual_seed(11)
    n = 67
    row = torch.randint(0, 66, (300,), generator=g)
    col = torch.randint(0, 66, (300,), generator=g)
    off = row != col
    row, col = row[off], col[off]
    diag = torch.tensor([1, 4, 4, 30, 65])
    row = torch.cat([row, diag, torch.full((1500,), 23)])
    col = torch.cat([col, diag, torch.randint(0, 66, (1500,), generator=g)])
    order = torch.argsort(row * n + col, stable=True)
    row, col = row[order], col[order]
    w = torch.rand(row.numel(), generator=g) + 0.1
    assert int(((row == 23) & (col == 23)).sum()) >= 1 and not bool(((row == 66) | (col == 66)).any())
    return n, row, col, w


def dense(row, col, val, shape):
    """Dense float64 matrix of a COO list, duplicates added (what an aggregation does with them); differentiable in ``val``."""
    return torch.zeros(shape, dtype=torch.float64).index_put((row, col), val, accumulate=True)


# ------------------------------------------------------------------------------------------------
# 1. the kernel through the C ABI
# ------------------------------------------------------------------------------------------------
def c_sddmm(adj, G, X, bits, scale=None, argmax=None):
    n_rows, n_src = adj.sparse_sizes()
    if bits == 32:
        rowptr, col, b = adj._index_arrays()
        assert b == 32
    else:
        rowptr, col = adj._rowptr, adj._col     # the int64 arrays straight to the C entry point
    dval = torch.full((adj.nnz(),), float("nan"), dtype=torch.float32, device=DEV)
    rc = _lib.load().egnn_sddmm_csr_f32(n_rows, n_src, X.shape[1], _lib.ptr(rowptr), _lib.ptr(col), bits, adj.nnz(), _lib.ptr(G), G.stride(0),
                                        _lib.ptr(X), X.stride(0), _lib.ptr(scale), _lib.ptr(argmax), _lib.ptr(dval), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return dval


def sddmm_ref(adj, G, X, scale=None, mask=None):
    """(ref, bound) in float64 from the float32 inputs; ``mask`` [nnz, K] restricts the columns (max)."""
    row, col = adj._row(), adj._col
    K = X.shape[1]
    p = G.double()[row] * X.double()[col]
    if mask is not None:
        p = p * mask
    s = torch.ones(adj.sparse_size(0), dtype=torch.float64) if scale is None else scale.double()
    return p.sum(-1) * s[row], gamma(K + 2) * p.abs().sum(-1) * s[row].abs()


def views(n_rows, n_src, K, pad, seed):
    """G [n_rows, K] and X [n_src, K] as views of wider buffers (row pitch K + pad)."""
    g = torch.Generator().manual_seed(seed)
    Gb, Xb = torch.randn(n_rows, K + pad, generator=g), torch.randn(n_src, K + pad, generator=g)
    return Gb, Xb


# (K, pad): pitch K + pad.  K = 1, 5: scalar lanes (5: a group that is not full); 40: four entries per wave-instruction; 256: one; 752:
# the looping group; (40, 3) and (256, 1): float4-sized K behind a pitch that is not 16-byte aligned -> scalar lanes
SHAPES = [(1, 4), (5, 4), (40, 4), (256, 4), (752, 4), (40, 3), (256, 1)]


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("K,pad", SHAPES)
def test_sddmm_kernel_c_abi(K, pad, bits, with_scale):
    adj = rect_graph()
    Gb, Xb = views(37, 53, K, pad, seed=100 + K)
    scale = adj._inv_rowcount() if with_scale else None
    ref, bound = sddmm_ref(adj, Gb[:, :K], Xb[:, :K], scale)
    dadj = adj.to(DEV)
    Gd, Xd = Gb.to(DEV)[:, :K], Xb.to(DEV)[:, :K]
    assert Gd.stride(0) == K + pad and Xd.stride(0) == K + pad
    sd = None if scale is None else scale.to(DEV)
    got = c_sddmm(dadj, Gd, Xd, bits, sd)
    err = (got.cpu().double() - ref).abs()
    print(f"K={K} pad={pad} bits={bits} scale={with_scale}: max err / bound = {float((err / bound.clamp(min=1e-300)).max().detach()):.3f}")
    assert bool(torch.isfinite(got).all()), "an entry was not written"
    assert bool((err <= bound).all()), f"max excess {float((err - bound).max())}"
    assert torch.equal(got, c_sddmm(dadj, Gd, Xd, bits, sd)), "two calls differ"


@pytest.mark.parametrize("bits", [32, 64])
def test_sddmm_kernel_single_entry_and_empty(bits):
    one = E.SparseTensor(row=torch.tensor([1]), col=torch.tensor([1]), sparse_sizes=(3, 2))
    Gb, Xb = views(3, 2, 40, 4, seed=5)
    ref, bound = sddmm_ref(one, Gb[:, :40], Xb[:, :40])
    got = c_sddmm(one.to(DEV), Gb.to(DEV)[:, :40], Xb.to(DEV)[:, :40], bits)
    assert got.shape == (1,) and bool(((got.cpu().double() - ref).abs() <= bound).all())
    empty = E.SparseTensor(rowptr=torch.zeros(5, dtype=torch.int64), col=torch.zeros(0, dtype=torch.int64), sparse_sizes=(4, 3)).to(DEV)
    rc = _lib.load().egnn_sddmm_csr_f32(4, 3, 8, _lib.ptr(empty._rowptr), None, bits, 0, None, 8, None, 8, None, None, None, _lib.stream())
    assert rc == 0                                                                 # nnz == 0: launches nothing
    assert ops.sddmm(empty, torch.randn(4, 8, device=DEV), torch.randn(3, 8, device=DEV)).shape == (0,)


# ------------------------------------------------------------------------------------------------
# 2. autograd through ops.spmm(adj.set_value(v), x, reduce)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("K", [5, 40])
def test_spmm_value_gradient(K, reduce):
    adj = rect_graph()
    row, col, nnz = adj._row(), adj._col, adj.nnz()
    g = torch.Generator().manual_seed(200 + K)
    if reduce == "max":   # multiples of 1/8 of small magnitude: the products are exact in fp32 and the ties are real ties
        x = torch.randint(-8, 9, (53, K), generator=g).float() / 8
        v = torch.randint(-8, 9, (nnz,), generator=g).float() / 8
    else:
        x, v = torch.randn(53, K, generator=g), torch.randn(nnz, generator=g)
    gy = torch.randn(37, K, generator=g)
    dadj = adj.to(DEV)
    vg, xg = leaf(v), leaf(x)
    y = ops.spmm(dadj.set_value(vg), xg, reduce)
    assert type(y.grad_fn).__name__ == "_SpMMValuedBackward"
    (y * gy.to(DEV)).sum().backward()

    v64, x64 = v.detach().double().requires_grad_(True), x.detach().double().requires_grad_(True)
    cnt = (adj._rowptr[1:] - adj._rowptr[:-1]).clamp(min=1).double()
    if reduce == "max":
        oadj = OS.SparseTensor(row=row, col=col, value=v64.detach(), sparse_sizes=(37, 53), is_sorted=True)
        yr, arg_ref = OS.matmul_max_with_arg(oadj, x64)
        (yr * gy.double()).sum().backward()
        arg = ops.spmm_raw(dadj.set_value(vg.detach()), xg.detach(), "max")[1]
        assert torch.equal(arg.cpu(), arg_ref), "argmax: first maximal entry in CSR order"
        mask = (arg_ref[row] == torch.arange(nnz).unsqueeze(1)).double()          # m(e,k) = (argmax[r,k] == e)
        gv_ref, bound = sddmm_ref(adj, gy, x, None, mask)
        assert float(mask.sum(-1).max()) >= 1
    else:
        yr = torch.zeros(37, K, dtype=torch.float64).index_add(0, row, v64.unsqueeze(1) * x64[col])
        scale = None
        if reduce == "mean":   # mean divides by the stored-entry count, not by the sum of the values
            yr = yr / cnt.unsqueeze(1)
            scale = 1.0 / cnt            # exact in float64; the kernel's fp32 1 / cnt is one of the bound's K + 2 roundings
        (yr * gy.double()).sum().backward()
        gv_ref, bound = sddmm_ref(adj, gy, x, scale)
        close(gv_ref, v64.grad, rtol=1e-12, atol_scale=1e-14, msg="the closed form is float64 autograd's value gradient")
    close(y, yr, msg=f"y {reduce} K={K}")
    err = (vg.grad.cpu().double() - gv_ref).abs()
    print(f"{reduce} K={K}: value gradient max err / bound = {float((err / bound.clamp(min=1e-300)).max().detach()):.3f}")
    assert bool((err <= bound).all()), f"value gradient: max excess {float((err - bound).max())}"
    close(xg.grad, x64.grad, rtol=1e-4, msg=f"dX {reduce} K={K}")
    # same numbers without grad on the values: the old Function, bit-equal y, no value gradient
    v_const = vg.detach().clone()
    x2 = xg.detach().clone().requires_grad_(True)
    y2 = ops.spmm(dadj.set_value(v_const), x2, reduce)
    assert type(y2.grad_fn).__name__ == "_SpMMBackward"
    assert torch.equal(y, y2)
    (y2 * gy.to(DEV)).sum().backward()
    assert v_const.grad is None
    if reduce == "max":   # dX of max is the package's one atomic scatter (egnn_spmm_csr_max_bwd_f32): equal up to the order of its adds
        close(x2.grad, xg.grad, rtol=1e-4)
    else:
        assert torch.equal(x2.grad, xg.grad)


def test_value_graph_survives_structure_ops():
    """set_value / t() / matmul keep the value tensor's graph: the gradient of (A^T g) . 1 with respect to the values arrives."""
    adj = rect_graph().to(DEV)
    v = torch.rand(adj.nnz(), device=DEV).requires_grad_(True)
    gsrc = torch.randn(37, 8, device=DEV)
    out = adj.set_value(v).t().matmul(gsrc, "sum")            # [53, 8]
    out.sum().backward()
    ref = gsrc.double().sum(1)[adj._row()]                    # d/dv_e sum_k (A^T g)[col(e), k] = sum_k g[row(e), k]
    close(v.grad, ref, rtol=1e-5)


# ------------------------------------------------------------------------------------------------
# 3. valued gcn_norm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unsorted", [False, True])
def test_gcn_norm_valued(unsorted):
    n, row, col, w = square_graph()
    if unsorted:   # caller-provided CSR arrays whose columns are not ascending inside the rows: the values must travel with the re-sort
        g = torch.Generator().manual_seed(3)
        shuffle = torch.randperm(row.numel(), generator=g)
        order = shuffle[torch.argsort(row[shuffle], stable=True)]
        row, col, w = row[order], col[order], w[order]
        assert bool((col[1:] < col[:-1])[row[1:] == row[:-1]].any())
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)

    w64 = w.detach().double().requires_grad_(True)
    ref = OS.gcn_norm_sparse(OS.SparseTensor(row=row, col=col, value=w64, sparse_sizes=(n, n)))
    r_rowptr, r_col, r_val = ref.csr()
    c = torch.randn(r_val.numel(), generator=torch.Generator().manual_seed(4))
    (r_val * c.double()).sum().backward()

    wg = leaf(w)
    if unsorted:
        adj = E.SparseTensor(rowptr=rowptr.to(DEV), col=col.to(DEV), value=wg, sparse_sizes=(n, n))
    else:
        adj = E.SparseTensor(row=row.to(DEV), col=col.to(DEV), value=wg, sparse_sizes=(n, n), is_sorted=True)
    out = gcn_norm(adj)
    plain = gcn_norm(E.SparseTensor(row=row.to(DEV), col=col.to(DEV), sparse_sizes=(n, n)))
    o_rowptr, o_col, o_val = out.csr()
    assert torch.equal(o_rowptr, plain.csr()[0]) and torch.equal(o_col, plain.csr()[1]), "structure differs from the value-less path"
    assert torch.equal(o_rowptr.cpu(), r_rowptr) and torch.equal(o_col.cpu(), r_col)
    d_max = int((r_rowptr[1:] - r_rowptr[:-1]).max())
    assert d_max > 1400
    rel = ((o_val.detach().cpu().double() - r_val.detach()).abs() / r_val.detach().abs()).max()
    print(f"unsorted={unsorted}: values max rel err {float(rel):.3e}, bar {(d_max + 8) * 2.0 ** -23:.3e}")
    assert float(rel) <= (d_max + 8) * 2.0 ** -23
    assert torch.equal(o_val.detach(), gcn_norm(adj.set_value(wg.detach())).csr()[2]), "grad and no-grad path differ / not bit-stable"

    (o_val * c.to(DEV)).sum().backward()
    gref = w64.grad
    err = (wg.grad.cpu().double() - gref).abs().max()
    print(f"unsorted={unsorted}: weight gradient max abs err {float(err):.3e}, bar {1e-4 * float(gref.abs().max()):.3e}")
    assert float(err) <= 1e-4 * float(gref.abs().max())
    dropped = row == col
    assert int(dropped.sum()) >= 5 and bool((wg.grad.cpu()[dropped] == 0).all()), "a dropped stored diagonal has gradient exactly 0"
    assert bool((gref[dropped] == 0).all())


# ------------------------------------------------------------------------------------------------
# 4. GCNConv with weights, both input kinds
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_graph():
    """31 nodes, (source, target) edges with duplicates; node 3 has one self loop of weight 0.3, node 30 no edge at all."""
    g = torch.Generator().manual_seed(21)
    n = 31
    src, dst = torch.randint(0, 30, (140,), generator=g), torch.randint(0, 30, (140,), generator=g)
    off = src != dst
    src, dst = torch.cat([src[off], src[off][:10], torch.tensor([3])]), torch.cat([dst[off], dst[off][:10], torch.tensor([3])])
    w = torch.rand(src.numel(), generator=g) + 0.1
    w[-1] = 0.3
    return n, torch.stack([src, dst]), w


def ref_adj_hat(kind, n, ei, w64):
    """Dense float64 A^ [target, source] from the oracle's helpers; differentiable in ``w64``."""
    if kind == "sparse":    # SparseTensor branch: fill_diag(1) replaces a stored loop
        a = OS.gcn_norm_sparse(OS.SparseTensor(row=ei[1], col=ei[0], value=w64, sparse_sizes=(n, n)))
        row, col, val = a.coo()
        return dense(row, col, val, (n, n))
    ei2, ew = OS.add_remaining_self_loops(ei, w64, 1.0, n)   # edge-index branch: an existing loop keeps its weight
    s, t = ei2[0], ei2[1]
    deg = torch.zeros(n, dtype=torch.float64).index_add(0, t, ew)
    dinv = deg.pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    return dense(t, s, dinv[s] * ew * dinv[t], (n, n))


def gpu_inputs(kind, n, ei, wg):
    """(edge_index argument, edge_weight argument) of the conv for one input kind."""
    if kind == "sparse":
        return E.SparseTensor(row=ei[1].to(DEV), col=ei[0].to(DEV), value=wg, sparse_sizes=(n, n)), None
    return ei.to(DEV), wg


def make_conv(cin, cout, seed, **kw):
    torch.manual_seed(seed)
    conv = PN.GCNConv(cin, cout, **kw)
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    return conv


@pytest.mark.parametrize("cin,cout", [(12, 20), (20, 12), (5, 3)])
@pytest.mark.parametrize("kind", ["sparse", "edge_index"])
def test_gcnconv_weighted(kind, cin, cout):
    n, ei, w = conv_graph()
    conv = make_conv(cin, cout, seed=cin)
    W64, b64 = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    conv = conv.to(DEV)
    g = torch.Generator().manual_seed(cout)
    x, c = torch.randn(n, cin, generator=g), torch.randn(n, cout, generator=g)
    x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    ref = ref_adj_hat(kind, n, ei, w64) @ (x64 @ W64) + b64
    (ref * c.double()).sum().backward()

    xg, wg = leaf(x), leaf(w)
    a, ew = gpu_inputs(kind, n, ei, wg)
    out = conv(xg, a, ew)
    (out * c.to(DEV)).sum().backward()
    close(out, ref, msg="out")
    close(xg.grad, x64.grad, rtol=1e-4, msg="dx")
    close(conv.weight.grad, W64.grad, rtol=1e-4, msg="dW")
    close(conv.bias.grad, b64.grad, rtol=1e-4, msg="db")
    close(wg.grad, w64.grad, rtol=1e-4, msg="d edge weights")
    loop = float(wg.grad[-1])
    if kind == "edge_index":
        assert loop != 0.0, "the kept self loop of weight 0.3 gets a gradient"
    else:
        assert loop == 0.0, "the SparseTensor branch drops the stored loop"
    assert conv._cached_adj_t is None and conv._cached_ax is None
    # constant weights give the same numbers through the old aggregation Function
    with torch.no_grad():
        close(conv(xg.detach(), *gpu_inputs(kind, n, ei, wg.detach())), ref, msg="constant weights")


@pytest.mark.parametrize("kind", ["sparse", "edge_index"])
def test_gcnconv_learnable_weights_are_never_cached(kind):
    """Two SGD steps on the edge weights: the second forward reflects the updated weights (a stale A^ would repeat the first)."""
    n, ei, w = conv_graph()
    for cached in (False, True):
        conv = make_conv(12, 20, seed=1, cached=cached)
        W64, b64 = conv.weight.detach().double(), conv.bias.detach().double()
        conv = conv.to(DEV)
        g = torch.Generator().manual_seed(9)
        x, c = torch.randn(n, 12, generator=g), torch.randn(n, 20, generator=g)
        wg, w64 = leaf(w), w.detach().double().requires_grad_(True)
        outs = []
        for step in range(3):
            a, ew = gpu_inputs(kind, n, ei, wg)
            out = conv(x.to(DEV), a, ew)
            ref = ref_adj_hat(kind, n, ei, w64) @ (x.double() @ W64) + b64
            close(out, ref, msg=f"forward {step} cached={cached}")
            outs.append(out.detach())
            gw, = torch.autograd.grad((out * c.to(DEV)).sum(), wg)
            gr, = torch.autograd.grad((ref * c.double()).sum(), w64)
            with torch.no_grad():
                wg -= 0.05 * gw
                w64 -= 0.05 * gr
            assert conv._cached_adj_t is None
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
        a, ew = gpu_inputs(kind, n, ei, wg)
        with torch.no_grad():   # eval between steps must not leave a cached A^ behind either
            conv(x.to(DEV), a, ew)
        assert conv._cached_adj_t is None


@pytest.mark.parametrize("kind", ["sparse", "edge_index"])
def test_gcnconv_constant_weights_cache(kind):
    n, ei, w = conv_graph()
    x = torch.randn(n, 12, generator=torch.Generator().manual_seed(2)).to(DEV)
    wd = w.to(DEV).clone()
    a, ew = gpu_inputs(kind, n, ei, wd)
    conv = make_conv(12, 20, seed=1, cached=True).to(DEV)
    with torch.no_grad():
        y1 = conv(x, a, ew)
        norm = conv._cached_adj_t
        assert norm is not None
        y2 = conv(x, a, ew)
    assert conv._cached_adj_t is norm and torch.equal(y1, y2), "cached=True re-normalised"
    if kind == "edge_index":   # cached=False: the edge-list memo keys on the weight tensor too (identity + version)
        plain = make_conv(12, 20, seed=1).to(DEV)
        PN._GCN_NORM_CACHE.clear()
        with torch.no_grad():
            plain(x, a, ew)
            plain(x, a, ew)
            assert len(PN._GCN_NORM_CACHE) == 1
            wd.mul_(2.0)            # same tensor, new version: a new entry, new numbers
            y3 = plain(x, a, ew)
            assert len(PN._GCN_NORM_CACHE) == 2
            plain(x, a)             # the value-less list is its own entry
            assert len(PN._GCN_NORM_CACHE) == 3
        w64 = (w * 2.0).double()
        ref = ref_adj_hat(kind, n, ei, w64) @ (x.cpu().double() @ plain.weight.detach().cpu().double()) + plain.bias.detach().cpu().double()
        close(y3, ref)
        PN._GCN_NORM_CACHE.clear()


def test_gcnconv_weighted_epilogue_routes():
    """The block schedule's epilogues on a valued A^ whose values require grad: BatchNorm statistics with the bias in the store
    (transform-first, 64 output channels), and the eval-mode BatchNorm fold under no_grad."""
    n, ei, w = conv_graph()
    conv = make_conv(72, 64, seed=3)
    W64, b64 = conv.weight.detach().double(), conv.bias.detach().double()
    conv = conv.to(DEV)
    x = torch.randn(n, 72, generator=torch.Generator().manual_seed(6))
    wg, w64 = leaf(w), w.detach().double().requires_grad_(True)
    adj, _ = gpu_inputs("sparse", n, ei, wg)
    ref = ref_adj_hat("sparse", n, ei, w64) @ (x.double() @ W64) + b64
    out = conv(x.to(DEV), adj, want_bn_stats=True, bn_stats_shift=torch.zeros(64, device=DEV))
    close(out, ref)
    stats = getattr(out, "_egnn_bn_stats", None)
    assert stats is not None, "the statistics epilogue did not run"
    close(stats[0], ref.detach().mean(0), rtol=1e-4)
    close(stats[1], ref.detach().var(0, unbiased=False), rtol=1e-4)
    out.sum().backward()
    ref.sum().backward()
    close(wg.grad, w64.grad, rtol=1e-4)
    bn = torch.nn.BatchNorm1d(64)
    with torch.no_grad():
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    bn.eval()
    with torch.no_grad():
        ref_eval = torch.relu(bn.double()(ref.detach()))
        got = conv(x.to(DEV), adj, eval_bn=bn.float().to(DEV))
    close(got, ref_eval)
