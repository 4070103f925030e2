"""Structure-preservation metrics of the reference's analysis script (arxiv_pyg/correlation.py) on the device: did the student's
embedding space keep the teacher's structure?  Three numbers per (student, teacher) pair over the rows ``idx``:

* global structural correlation (Mantel): Pearson r between the all-pairs cosine distances (:178-181, 205-208, 212),
* local structural correlation: Pearson r between the per-edge cosine distances of the induced sub-graph (:104-106, 182, 209, 213),
* linear CKA of the row-normalised features (:78-85, 214).

* kernel (RBF) CKA with a median-heuristic bandwidth (:41-53, 70-75): ``kernel_cka``, ``rbf_bandwidth``.

Kernels in csrc/similarity.hip.  No N x N object is formed on any of the paths.  The functions return Python floats: each metric
costs one host read of its result (the six moments, or CKA's three Frobenius sums); the local metric reads the range of ``edge_index``
first, because the edge kernel addresses rows by those ids, and ``representation_similarity`` is the three metrics one after the other
plus the reads inside ``utils.subgraph``.  Kernel CKA with its own bandwidths reads its three float64 sums and nothing before them: the
medians stay on the device.  Nothing here is differentiable or captured.  CPU tensors raise ``_lib.HipExtensionError``.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _lib, ops

_K_COSINE = 0


def _moments_out(dev) -> Tensor:
    return torch.empty(6, dtype=torch.float64, device=dev)


def pair_moments(xs_hat: Tensor, xt_hat: Tensor) -> Tensor:
    """(n, sum a, sum b, sum a^2, sum b^2, sum ab) in float64 on the device over all pairs i < j of the unit rows, with
    a = <xs_i, xs_j>, b = <xt_i, xt_j> (egnn_pair_moments_f32).  Strided row-major views are taken as they are."""
    _lib.require_gpu(xs_hat, xt_hat)
    xs, xt = ops._gemm_operand(xs_hat), ops._gemm_operand(xt_hat)
    if xs.dtype != torch.float32 or xt.dtype != torch.float32:
        raise TypeError("pair_moments: expected float32 rows")
    N = xs.shape[0]
    if xt.shape[0] != N:
        raise ValueError("pair_moments: student and teacher need the same number of rows")
    if N < 2:
        raise ValueError("pair_moments: at least 2 rows are needed")
    lib, dev = _lib.load(), xs.device
    out = _moments_out(dev)
    nws = lib.egnn_pair_moments_ws_bytes(N)
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    rc = lib.egnn_pair_moments_f32(_lib.ptr(xs), xs.stride(0), xs.shape[1], _lib.ptr(xt), xt.stride(0), xt.shape[1], N, _lib.ptr(out),
                                   _lib.ptr(ws), nws, _lib.stream())
    _lib.check(rc, "egnn_pair_moments_f32")
    return out


def vector_moments(a: Tensor, b: Tensor) -> Tensor:
    """The same six float64 moments of two float32 vectors of equal length (egnn_pearson_moments_f32)."""
    _lib.require_gpu(a, b)
    a, b = a.contiguous().view(-1), b.contiguous().view(-1)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError("vector_moments: expected float32 vectors")
    n = a.numel()
    if b.numel() != n or n < 1:
        raise ValueError("vector_moments: two non-empty vectors of equal length are needed")
    lib, dev = _lib.load(), a.device
    out = _moments_out(dev)
    nws = lib.egnn_pearson_moments_ws_bytes(n)
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    rc = lib.egnn_pearson_moments_f32(_lib.ptr(a), _lib.ptr(b), n, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream())
    _lib.check(rc, "egnn_pearson_moments_f32")
    return out


def pearson_from_moments(m) -> float:
    """r = (n Sab - Sa Sb) / sqrt((n Saa - Sa^2) (n Sbb - Sb^2)) in float64 from (n, Sa, Sb, Saa, Sbb, Sab); zero variance on either
    side gives nan, as scipy.stats.pearsonr does.  ``m`` is a tensor (one host read) or any sequence of six numbers."""
    n, sa, sb, saa, sbb, sab = (float(v) for v in (m.tolist() if isinstance(m, Tensor) else m))
    va, vb = n * saa - sa * sa, n * sbb - sb * sb
    # a constant variable: the two products agree to the rounding of their own float64 arithmetic
    tiny = 64.0 * 2.220446049250313e-16
    if not (va > tiny * n * saa and vb > tiny * n * sbb):
        return math.nan
    r = (n * sab - sa * sb) / math.sqrt(va * vb)
    return max(-1.0, min(1.0, r))   # rounding can leave |r| one ulp above 1; scipy clamps likewise


def _index(idx: Tensor | None) -> Tensor | None:
    return None if idx is None else idx.to(torch.int64).contiguous().view(-1)


def _unit_rows(x: Tensor, idx: Tensor | None) -> Tensor:
    """F.normalize(x[idx]) behind a row pitch that is a multiple of 4 floats (the teacher's 750 columns take the float4 path).
    ``idx`` may repeat rows: ``ops.gather_normalize`` asks for unique rows only on behalf of its backward, and none runs here."""
    with torch.no_grad():
        return ops.pad_pitch(ops.gather_normalize(x.detach(), idx))


def _check_pair(feat: Tensor, teacher_feat: Tensor, idx: Tensor | None) -> None:
    _lib.require_gpu(feat, teacher_feat, idx)
    if feat.dim() != 2 or teacher_feat.dim() != 2 or feat.shape[0] != teacher_feat.shape[0]:
        raise ValueError("student and teacher features are [N, Ds] and [N, Dt] over the same N rows")


def _global_r(xs: Tensor, xt: Tensor) -> float:
    return pearson_from_moments(pair_moments(xs, xt))


def structural_correlation(feat: Tensor, teacher_feat: Tensor, idx: Tensor | None = None) -> float:
    """Global structural correlation (Mantel): Pearson r between the condensed all-pairs cosine-distance matrices of the teacher and
    student rows ``idx`` (all rows when None)."""
    _check_pair(feat, teacher_feat, idx)
    idx = _index(idx)
    return _global_r(_unit_rows(feat, idx), _unit_rows(teacher_feat, idx))


def _edge_cosine(x_hat: Tensor, src: Tensor, dst: Tensor) -> Tensor:
    E = src.numel()
    sim = torch.empty(E, dtype=torch.float32, device=x_hat.device)
    aux = torch.empty(E, 3, dtype=torch.float32, device=x_hat.device)
    rc = _lib.load().egnn_edge_sim_f32(_lib.ptr(x_hat), x_hat.stride(0), x_hat.shape[1], _lib.ptr(src), _lib.ptr(dst), E, _K_COSINE,
                                       _lib.ptr(sim), _lib.ptr(aux), _lib.stream())
    _lib.check(rc, "egnn_edge_sim_f32")
    return sim


def _local_r(xs: Tensor, xt: Tensor, edge_index: Tensor) -> float:
    _lib.require_gpu(edge_index)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index is a [2, E] tensor")
    E = edge_index.shape[1]
    if E < 2:
        raise ValueError("local_structural_correlation: a correlation needs at least 2 edges")
    ei = edge_index.to(torch.int64)
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(ei)).tolist())   # the edge kernel reads rows by these ids: refuse a stray one
    if lo < 0 or hi >= xs.shape[0]:
        raise ValueError(f"edge_index addresses rows {lo}..{hi} of {xs.shape[0]} (it is in the index space of the rows after `idx`)")
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    return pearson_from_moments(vector_moments(_edge_cosine(xs, src, dst), _edge_cosine(xt, src, dst)))


def local_structural_correlation(feat: Tensor, teacher_feat: Tensor, edge_index: Tensor, idx: Tensor | None = None) -> float:
    """Local structural correlation: Pearson r between the per-edge cosine distances of teacher and student.  ``edge_index`` is in the
    index space of the rows AFTER ``idx`` (what ``utils.subgraph(idx, edge_index, relabel_nodes=True)`` returns)."""
    _check_pair(feat, teacher_feat, idx)
    idx = _index(idx)
    return _local_r(_unit_rows(feat, idx), _unit_rows(teacher_feat, idx), edge_index)


def _cka(x: Tensor, y: Tensor) -> float:
    """Feature-space linear CKA, ||Xc^T Yc||_F^2 / (||Xc^T Xc||_F ||Yc^T Yc||_F) with column-centred Xc, Yc: equal to the reference's
    n x n form sum(HKH o HLH) / sqrt(...) without an n x n matrix.  The rows are centred explicitly before the products (subtracting
    n mu mu^T afterwards cancels in fp32 for post-ReLU features); the three N-long reductions run on the fp32 MFMA."""
    with torch.no_grad():
        def centred(t):
            t64 = t.to(torch.float64)
            return ops.pad_pitch((t64 - t64.mean(dim=0, keepdim=True)).to(torch.float32))
        xc, yc = centred(x), centred(y)
        fro2 = lambda g: g.to(torch.float64).square().sum()   # noqa: E731
        xy = fro2(ops.gemm_raw(xc, yc, trans_a=True))
        xx = fro2(ops.gemm_raw(xc, xc, trans_a=True))
        yy = fro2(ops.gemm_raw(yc, yc, trans_a=True))
        xy, xx, yy = torch.stack([xy, xx, yy]).tolist()
    den = math.sqrt(xx * yy)
    return xy / den if den > 0.0 else math.nan   # a side without variance: 0 / 0, as the reference's form gives


def _rows(x: Tensor, idx: Tensor | None) -> Tensor:
    x = x.detach()
    return x if idx is None else x[idx]


def linear_cka(feat: Tensor, teacher_feat: Tensor, idx: Tensor | None = None, normalize: bool = True) -> float:
    """Linear CKA of the rows ``idx`` of the two feature matrices, row-normalised first as the reference does (``normalize``)."""
    _check_pair(feat, teacher_feat, idx)
    idx = _index(idx)
    if feat.dtype != torch.float32 or teacher_feat.dtype != torch.float32:
        raise TypeError("linear_cka: expected float32 features")
    if normalize:
        return _cka(_unit_rows(feat, idx), _unit_rows(teacher_feat, idx))
    return _cka(_rows(feat, idx), _rows(teacher_feat, idx))


def _sqdist_median(x: Tensor, out2: Tensor) -> None:
    """out2 (two float64 on the device) = (median of |x_i - x_j|^2 over the pairs i < j, the pair count) (egnn_sqdist_median_f32)."""
    lib, N = _lib.load(), x.shape[0]
    nws = lib.egnn_sqdist_median_ws_bytes(N)
    ws = torch.empty(nws // 8, dtype=torch.float64, device=x.device)
    rc = lib.egnn_sqdist_median_f32(_lib.ptr(x), x.stride(0), x.shape[1], N, _lib.ptr(out2), _lib.ptr(ws), nws, _lib.stream())
    _lib.check(rc, "egnn_sqdist_median_f32")


def _kernel_rows(x: Tensor, idx: Tensor | None, normalize: bool) -> Tensor:
    """The rows the RBF kernels read: unit rows behind a padded pitch, or the rows as they are (a strided row-major view is kept)."""
    if x.dtype != torch.float32:
        raise TypeError("expected float32 features")
    x = _unit_rows(x, idx) if normalize else ops._gemm_operand(_rows(x, idx))
    if x.shape[0] < 2:
        raise ValueError("at least 2 rows are needed")
    return x


def rbf_bandwidth(x: Tensor, idx: Tensor | None = None, normalize: bool = True) -> float:
    """The median-heuristic bandwidth sigma of the reference's ``rbf(X, None)``: the square root of the median of |x_i - x_j|^2 over
    the N (N-1) / 2 pairs i < j of the rows ``idx`` (row-normalised first with ``normalize``), the mean of the two middle values when
    that count is even.  The selection is exact over the fp32 distances the kernels form.  The reference takes
    ``np.median(KX[KX != 0])`` over the full symmetric matrix: the same number whenever no two rows coincide.  Where rows do coincide
    its filter depends on whether float64 rounding left an exact zero; here every pair is kept, zeros included.  One host read."""
    _lib.require_gpu(x, idx)
    if x.dim() != 2:
        raise ValueError("rbf_bandwidth: features are [N, D]")
    x = _kernel_rows(x, _index(idx), normalize)
    out2 = torch.empty(2, dtype=torch.float64, device=x.device)
    _sqdist_median(x, out2)
    return math.sqrt(out2.tolist()[0])


def _kcka(xs: Tensor, xt: Tensor, sigma) -> float:
    dev, N = xs.device, xs.shape[0]
    if sigma is None:
        med = torch.empty(2, 2, dtype=torch.float64, device=dev)
        _sqdist_median(xs, med[0])
        _sqdist_median(xt, med[1])
        sigma2 = med[:, 0].contiguous()          # stays on the device: the kernels read it through a pointer
    else:
        ss, st = (float(v) for v in (sigma if isinstance(sigma, (tuple, list)) else (sigma, sigma)))
        if not (ss > 0.0 and st > 0.0):
            return math.nan
        sigma2 = torch.tensor([ss * ss, st * st], dtype=torch.float64, device=dev)
    lib = _lib.load()
    out3 = torch.empty(3, dtype=torch.float64, device=dev)
    nws = lib.egnn_rbf_cka_ws_bytes(N)
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    rc = lib.egnn_rbf_cka_f32(_lib.ptr(xs), xs.stride(0), xs.shape[1], _lib.ptr(xt), xt.stride(0), xt.shape[1], N, _lib.ptr(sigma2),
                              _lib.ptr(out3), _lib.ptr(ws), nws, _lib.stream())
    _lib.check(rc, "egnn_rbf_cka_f32")
    xy, xx, yy = out3.tolist()
    den = math.sqrt(xx * yy) if xx > 0.0 and yy > 0.0 else 0.0     # a zero bandwidth arrives as nan sums
    return xy / den if den > 0.0 else math.nan


def kernel_cka(feat: Tensor, teacher_feat: Tensor, idx: Tensor | None = None, sigma=None, normalize: bool = True) -> float:
    """CKA under the Gaussian kernel K_ij = exp(-|x_i - x_j|^2 / (2 sigma^2)), the reference's ``kernel_CKA``, over the rows ``idx``
    (row-normalised first with ``normalize``, as ``linear_cka``).  ``sigma`` None: each side takes its own median bandwidth
    (``rbf_bandwidth``), as two ``rbf(., None)`` calls do, and nothing is read back before the final three sums; a float: both sides
    use it; a pair: (student, teacher).  nan when a bandwidth is 0 or a side's centred kernel matrix vanishes."""
    _check_pair(feat, teacher_feat, idx)
    idx = _index(idx)
    return _kcka(_kernel_rows(feat, idx, normalize), _kernel_rows(teacher_feat, idx, normalize), sigma)


def representation_similarity(feat: Tensor, teacher_feat: Tensor, idx: Tensor | None, edge_index: Tensor | None = None,
                              kernel_cka: bool = False) -> dict:
    """The three metrics of one (student, teacher) pair over the rows ``idx``: ``dict(global_=..., local=..., cka=...)``.
    ``edge_index`` is in the index space of ALL rows; the sub-graph induced by ``idx`` is taken and relabelled here
    (``utils.subgraph(idx, edge_index, relabel_nodes=True)``).  ``local`` is None without edges.  ``kernel_cka=True`` adds ``kcka``,
    the RBF CKA of the same unit rows with each side's median bandwidth."""
    from .utils import subgraph
    _check_pair(feat, teacher_feat, idx)
    idx = _index(idx)
    xs, xt = _unit_rows(feat, idx), _unit_rows(teacher_feat, idx)
    local = None
    if edge_index is not None:
        _lib.require_gpu(edge_index)
        if idx is not None:
            edge_index = subgraph(idx, edge_index, relabel_nodes=True, num_nodes=feat.shape[0])[0]
        local = _local_r(xs, xt, edge_index)
    out = dict(global_=_global_r(xs, xt), local=local, cka=_cka(xs, xt))
    if kernel_cka:
        if xs.dtype != torch.float32 or xt.dtype != torch.float32:
            raise TypeError("kernel CKA: expected float32 features")
        out["kcka"] = _kcka(xs, xt, None)
    return out
