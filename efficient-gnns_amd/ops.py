"""autograd.Function wrappers around the C ABI (include/egnn_hip.h).  GPU only; no CPU fallback."""
from __future__ import annotations

import ctypes
import os

import torch
from torch import Tensor

from . import _cache, _lib

_REDUCE = {"sum": 0, "add": 0, "mean": 1, "max": 2}
_OVERLAP_HEAVY_ROWS = True   # (no environment switch any more; tools/spmm_pmc.py clears the attribute to trace one stream)
_SIDE_STREAMS: dict = {}


def _side_stream(device) -> "torch.cuda.Stream":
    key = torch.device(device).index
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]



def _rowmajor(x: Tensor) -> Tensor:
    """fp32, unit inner stride (the kernels take an explicit leading dimension)."""
    if x.dtype != torch.float32:
        raise TypeError(f"expected float32, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError("expected a 2-D tensor")
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


# ------------------------------------------------------------------------------------------------
# SpMM
# ------------------------------------------------------------------------------------------------
# 'blocks' (default): egnn_spmm_csr_blk_f32; 'segments': egnn_spmm_csr_seg_f32; 'classes': short / mid / long row classes
_SPMM_SCHEDULE = "blocks"   # "blocks" (row blocks, K >= 64; class widths 32 < K < 64) -> "segments" (K <= 32) -> "classes" (max / unaligned); tests pin one by setting the attribute


class HipStatsUnavailable(RuntimeError):
    """spmm_raw(want_stats=True) on a shape / schedule whose kernel has no statistics epilogue (callers fall back to the
    separate egnn_bn_stats_f32 pass)."""


def _spmm_desc(adj, rowptr, col, bits, x, y, red, src_scale, bias) -> ctypes.Structure:
    """The egnn_spmm_t descriptor (include/egnn_hip.h) of one aggregation Y = REDUCE(adj, X), without an epilogue.  Built once per call
    from the tensors at hand (the caller keeps them alive); the entry points read it only while they run."""
    n_rows, n_src = adj.sparse_sizes()
    return _lib.Spmm(n_rows, n_src, x.shape[1], _lib.ptr(rowptr), _lib.ptr(col), bits, _lib.ptr(adj._value), _lib.ptr(src_scale),
                     _lib.ptr(bias), _lib.ptr(x), x.stride(0), _lib.ptr(y), y.stride(0), red)


def class_width_enabled() -> bool:
    """False when EGNN_SPMM_CLASS_WIDTH=0 sends the class widths (32 < K < 64) back to the
    segment schedule they ran on before the block entry point had a form for them."""
    return os.environ.get("EGNN_SPMM_CLASS_WIDTH", "1") != "0"


def spmm_raw(adj, x: Tensor, reduce: str = "sum", src_scale: Tensor | None = None, use_plan: bool = True,
             bias: Tensor | None = None, out: Tensor | None = None, stat_shift: Tensor | None = None, want_stats: bool = False,
             addend: Tensor | None = None, relu: bool = False):
    """``relu``: Y = max(REDUCE(adj, X) + bias, 0), fused into the block kernel's store (eval-mode BatchNorm folded into the
    weights + ReLU, ``bn_fold``); on the other schedules a clamp follows."""
    fused = []   # filled by _spmm_raw when the kernel applied the ReLU in its store (a value, not a tag on the -- possibly caller-owned -- output buffer)
    res = _spmm_raw(adj, x, reduce, src_scale, use_plan, bias, out, stat_shift, want_stats, addend, relu, fused)
    if relu and not fused:
        res[0].clamp_(min=0)
    return res


def _spmm_raw(adj, x: Tensor, reduce: str = "sum", src_scale: Tensor | None = None, use_plan: bool = True,
              bias: Tensor | None = None, out: Tensor | None = None, stat_shift: Tensor | None = None, want_stats: bool = False,
              addend: Tensor | None = None, relu: bool = False, relu_fused: list | None = None):
    """Y = REDUCE(adj, X) on the GPU.  Returns (Y, argmax | None), or (Y, None, (mean, biased var)) with ``want_stats``.

    Schedules: 'blocks' (default; egnn_spmm_csr_blk_f32: one launch over hub segments + row blocks, int32 indices, then the
    fixed-order combine of the hub rows), 'segments' (round-1 egnn_spmm_csr_seg_f32), 'classes' (egnn_spmm_csr_f32: also the
    path of ``max`` and of shapes the float4 kernels do not take).
    ``out``: optional [n_rows, K] destination with unit column stride (e.g. a column block of a wider matrix).
    ``addend``: optional [n_rows, K] matrix added to the result in the kernel's store (Y = A X + addend; sum / mean).
    ``want_stats`` (sum / mean on the block schedule only): per-column mean and biased variance of Y over all rows, formed in
    the aggregation's epilogue (BatchNorm statistics, gnn.py:47-48); ``stat_shift`` [K]: shift of the shifted sums."""
    _lib.require_gpu(x, adj._col)
    x = _rowmajor(x)
    n_rows, n_src = adj.sparse_sizes()
    if x.shape[0] != n_src:
        raise ValueError(f"matmul: adjacency has {n_src} columns, x has {x.shape[0]} rows")
    K = x.shape[1]
    red = _REDUCE[reduce]
    if out is not None:
        if tuple(out.shape) != (n_rows, K) or out.stride(1) != 1 or out.dtype != torch.float32 or out.device != x.device:
            raise ValueError("spmm_raw: `out` must be a float32 [n_rows, K] view with unit column stride on x's device")
        y = out
    else:
        y = torch.empty(n_rows, K, dtype=torch.float32, device=x.device)
    arg = torch.empty(n_rows, K, dtype=torch.int64, device=x.device) if red == 2 else None
    if addend is not None:
        if red == 2 or tuple(addend.shape) != (n_rows, K) or addend.dtype != torch.float32:
            raise ValueError("spmm_raw: `addend` is a float32 [n_rows, K] matrix (sum / mean only)")
        addend = _rowmajor(addend)
    if adj.nnz() == 0:   # no stored entry at all: every row is empty (sum / mean / max = 0, argmax = -1), plus the bias
        y.zero_()
        if bias is not None:
            y.add_(bias)
        if addend is not None:
            y.add_(addend)
        if arg is not None:
            arg.fill_(-1)
        if want_stats:
            raise HipStatsUnavailable()
        return y, arg
    rowptr, col, bits = adj._index_arrays()
    lib = _lib.load()
    op = _spmm_desc(adj, rowptr, col, bits, x, y, red, src_scale, bias)
    op_ref = ctypes.byref(op)
    float4_ok = (use_plan and red != 2 and K % 4 == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
                 and y.stride(0) % 4 == 0 and y.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 16 == 0))
    add_fused = addend is not None and addend.stride(0) % 4 == 0 and addend.data_ptr() % 16 == 0
    # the block schedule wins from two 128-byte column slices up (K = 256: 343 vs 385 us, K = 128: 167 vs 186 us on the
    # arxiv-shaped graph); below that its 8-lane slices lose to the 16-lane form of the segment kernel (113 vs 92 us at the 40-class
    # output layer), but the class widths have a 16-lane form of their own behind the same entry point (csrc/spmm_blk.hip)
    class_width = 32 < K < 64 and not want_stats and class_width_enabled()
    if (float4_ok and _SPMM_SCHEDULE == "blocks" and bits == 32 and (K >= 64 or class_width) and n_src * x.stride(0) * 4 < 2 ** 31
            and n_rows > 0 and (addend is None or add_fused)):
        from .sparse import BLK_ROWS, SEG_MAX
        hseg, crow, cptr, slots = adj._blk_plan()
        partial = adj._scratch("partial", (max(slots, 1), K))
        loc = adj._struct.get("locality")          # opt-in: (rows_per_blk, win) of SparseTensor.stage_diagonal_blocks()
        use_lds = loc is not None and n_rows == n_src and K % 32 == 0
        rows_blk = loc[0] if use_lds else BLK_ROWS
        n_blk = (n_rows + rows_blk - 1) // rows_blk
        # Y rows are stored write-through (dropped from L2: they are not re-read here and would only evict gathered X lines)
        # (the class widths keep the plain stores of the segment schedule they ran on: their Y is the next kernel's input)
        flags = (0 if K < 64 else 4) | (8 if (relu and not want_stats) else 0)
        n_stat = lib.egnn_spmm_blk_stat_rows(n_rows, rows_blk, int(use_lds)) if want_stats else 0
        n_hub = crow.numel()
        stat_part = adj._scratch("stat", (n_stat + n_hub, 2, K)) if want_stats else None   # one partial row per wave + per hub row
        if stat_shift is not None:
            stat_shift = stat_shift.detach().contiguous()
        # the epilogue: read by the block launch and by its combine step, which share the descriptor
        op.addend, op.ld_addend = _lib.ptr(addend), 0 if addend is None else addend.stride(0)
        op.stat_part, op.stat_shift, op.flags = _lib.ptr(stat_part), _lib.ptr(stat_shift) if want_stats else None, flags
        rc = lib.egnn_spmm_csr_blk_f32(op_ref, SEG_MAX, rows_blk, None, 0, _lib.ptr(loc[1]) if use_lds else None, _lib.ptr(hseg),
                                       hseg.shape[0], _lib.ptr(partial), _lib.stream())
        if rc == 0:
            if n_hub > 0:   # the hub rows: fixed-order sum of their partial slots (+ mean / bias, + their statistics rows)
                _lib.check(lib.egnn_spmm_combine_f32(op_ref, _lib.ptr(crow), _lib.ptr(cptr), n_hub, _lib.ptr(partial), n_stat, _lib.stream()),
                           "egnn_spmm_combine_f32")
            if not want_stats:
                if flags & 8 and relu_fused is not None:
                    relu_fused.append(True)
                return y, None
            mean = torch.empty(K, dtype=torch.float32, device=x.device)
            var = torch.empty(K, dtype=torch.float32, device=x.device)
            nws = lib.egnn_bn_stats_merge_ws_floats(K)
            ws = adj._scratch("statfold", (nws,))
            _lib.check(lib.egnn_bn_stats_merge_f32(_lib.ptr(stat_part), n_stat + n_hub, K, None, 0, None, 0,
                                                   _lib.ptr(stat_shift), n_rows, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(ws), nws,
                                                   _lib.stream()), "egnn_bn_stats_merge_f32")
            return y, None, (mean, var)
        if rc != -4:   # EGNN_EALIGN: shape outside the block kernel's forms -> the schedules below, which have no epilogue
            _lib.check(rc, "egnn_spmm_csr_blk_f32")
        op.addend = op.stat_part = op.stat_shift = None
        op.ld_addend = op.flags = 0
    if want_stats:
        raise HipStatsUnavailable()
    if float4_ok and _SPMM_SCHEDULE in ("blocks", "segments"):
        # every row as ranges of <= 64 entries through the sub-group-per-row kernel (hub rows get the bulk's parallelism)
        seg, crow, cptr, slots = adj._seg_plan()
        partial = adj._scratch("partial", (max(slots, 1), K))
        rc = lib.egnn_spmm_csr_seg_f32(op_ref, _lib.ptr(seg), seg.shape[0], _lib.ptr(crow), _lib.ptr(cptr), crow.numel(), _lib.ptr(partial),
                                       slots, _lib.stream())
        if rc == 0:
            if addend is not None:
                y.add_(addend)
            return y, None
        if rc != -4:   # EGNN_EALIGN: shape outside the segment kernel's float4 forms -> classic schedule below
            _lib.check(rc, "egnn_spmm_csr_seg_f32")
    short, mid, long_ = adj._row_plan() if use_plan else (None, None, None)

    def lst(t):
        return (None, 0) if t is None or t.numel() == 0 else (_lib.ptr(t), t.numel())

    def launch(s, m, l, stream):
        return lib.egnn_spmm_csr_f32(op_ref, _lib.ptr(arg), *lst(s), *lst(m), *lst(l), stream)

    heavy = use_plan and short is not None and short.numel() > 0 and (mid.numel() + long_.numel()) > 0
    if heavy and _OVERLAP_HEAVY_ROWS:
        # the few mid / long rows run on a side stream underneath the short-row bulk (fork / join with events)
        main = torch.cuda.current_stream()
        side = _side_stream(x.device)
        fork = torch.cuda.Event()
        fork.record(main)
        side.wait_event(fork)
        rc = launch(None, mid, long_, side.cuda_stream)
        _lib.check(rc, "egnn_spmm_csr_f32")
        rc = launch(short, None, None, main.cuda_stream)
        join = torch.cuda.Event()
        join.record(side)
        main.wait_event(join)
        for t in (x, y, arg, adj._value, src_scale, bias):
            if t is not None:
                t.record_stream(side)
    else:
        rc = launch(short, mid, long_, _lib.stream())
    _lib.check(rc, "egnn_spmm_csr_f32")
    if addend is not None:
        y.add_(addend)
    return y, arg


def _spmm_forward(adj, x, reduce, bias, stat_shift, want_stats):
    """The forward both aggregation Functions share: (Y, argmax | None, (mean, var) | None)."""
    b = None if bias is None else bias.detach().contiguous()
    stats = None
    if want_stats:
        try:
            y, arg, stats = spmm_raw(adj, x, reduce, bias=b, stat_shift=stat_shift, want_stats=True)
        except HipStatsUnavailable:
            y, arg = spmm_raw(adj, x, reduce, bias=b)
    else:
        y, arg = spmm_raw(adj, x, reduce, bias=b)
    return y, arg, stats


def _spmm_dx(adj, reduce, gy, arg):
    """dX of Y = REDUCE(adj, X): the transposed aggregation with value[perm] (sum / mean), the scatter through argmax (max)."""
    if reduce in ("sum", "add"):
        return spmm_raw(adj.t(), gy, "sum")[0]
    if reduce == "mean":
        # dX = A^T (dY / cnt): per-source-row scale of the transposed aggregation
        return spmm_raw(adj.t(), gy, "sum", src_scale=adj._inv_rowcount())[0]
    n_rows, n_src = adj.sparse_sizes()
    K = gy.shape[1]
    gx = torch.zeros(n_src, K, dtype=torch.float32, device=gy.device)
    if adj.nnz() == 0:   # no stored entry: nothing receives gradient
        return gx
    _, col, bits = adj._index_arrays()
    rc = _lib.load().egnn_spmm_csr_max_bwd_f32(n_rows, K, _lib.ptr(col), bits, _lib.ptr(adj._value), _lib.ptr(arg),
                                               _lib.ptr(gy), gy.stride(0), _lib.ptr(gx), gx.stride(0), _lib.stream())
    _lib.check(rc, "egnn_spmm_csr_max_bwd_f32")
    return gx


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, reduce, bias=None, stat_shift=None, want_stats=False):
        y, arg, stats = _spmm_forward(adj, x, reduce, bias, stat_shift, want_stats)
        ctx.adj, ctx.reduce, ctx.has_bias = adj, reduce, bias is not None
        ctx.tap_box = getattr(x, "_egnn_tap", None)     # x is a tapped tensor (grad_tap): its gradient may be completed in place, see _fresh
        if arg is not None:
            ctx.save_for_backward(arg)
        if stats is None:
            return y, None, None
        ctx.mark_non_differentiable(*stats)
        return y, stats[0], stats[1]

    @staticmethod
    def backward(ctx, gy, _gm=None, _gv=None):
        adj, reduce = ctx.adj, ctx.reduce
        gy = _rowmajor(gy)
        gx = _spmm_dx(adj, reduce, gy, ctx.saved_tensors[0] if reduce == "max" else None)
        gb = colsum(gy) if ctx.has_bias and ctx.needs_input_grad[3] else None
        return _fresh(gx, ctx.tap_box), None, None, gb, None, None


class _SpMMValued(torch.autograd.Function):
    """``_SpMM`` with the adjacency's VALUES as a tensor input: the call of a valued adjacency whose values require grad (learnable edge
    weights, edge gates).  Forward: the same ``spmm_raw`` call on the detached values (Y bit-equal to ``_SpMM``'s for the same numbers).
    Backward: dX as in ``_SpMM``; dval = ``sddmm`` over the pattern (torch-sparse's ``spmm`` value backward)."""

    @staticmethod
    def forward(ctx, x, value, adj, reduce, bias=None, stat_shift=None, want_stats=False):
        adj = adj.set_value(value.detach())      # same structure (and structure caches), values outside the graph
        y, arg, stats = _spmm_forward(adj, x, reduce, bias, stat_shift, want_stats)
        ctx.adj, ctx.reduce, ctx.has_bias = adj, reduce, bias is not None
        ctx.tap_box = getattr(x, "_egnn_tap", None)
        ctx.save_for_backward(x, arg)
        if stats is None:
            return y, None, None
        ctx.mark_non_differentiable(*stats)
        return y, stats[0], stats[1]

    @staticmethod
    def backward(ctx, gy, _gm=None, _gv=None):
        adj, reduce = ctx.adj, ctx.reduce
        x, arg = ctx.saved_tensors
        gy = _rowmajor(gy)
        gx = _fresh(_spmm_dx(adj, reduce, gy, arg), ctx.tap_box) if ctx.needs_input_grad[0] else None
        gv = sddmm(adj, gy, x, reduce, arg) if ctx.needs_input_grad[1] else None
        gb = colsum(gy) if ctx.has_bias and ctx.needs_input_grad[4] else None
        return gx, gv, None, None, gb, None, None


def sddmm(adj, g: Tensor, x: Tensor, reduce: str = "sum", argmax: Tensor | None = None) -> Tensor:
    """Gradient of ``REDUCE(adj, x)`` with respect to the values of ``adj`` given ``g`` = dY (egnn_sddmm_csr_f32): the [nnz] vector
    dval[e] = <g[row(e)], x[col[e]]> for ``sum``; times 1 / max(stored entries of the row, 1) for ``mean`` (mean divides by the entry
    count, not by the sum of the values: SURVEY 9.6); restricted to the columns where ``argmax`` [n_rows, K] picked entry e for ``max``.
    Only the pattern of ``adj`` is read; every entry is written, no atomics, run-to-run bit-stable."""
    if reduce not in _REDUCE:
        raise ValueError(f"unknown reduce '{reduce}'")
    _lib.require_gpu(g, x, adj._col)
    g, x = _rowmajor(g), _rowmajor(x)
    n_rows, n_src = adj.sparse_sizes()
    K = x.shape[1]
    if tuple(g.shape) != (n_rows, K) or x.shape[0] != n_src:
        raise ValueError(f"sddmm: adjacency is {n_rows} x {n_src}, g is {tuple(g.shape)}, x is {tuple(x.shape)}")
    red = _REDUCE[reduce]
    if red == 2:
        if argmax is None or tuple(argmax.shape) != (n_rows, K) or argmax.dtype != torch.int64 or not argmax.is_contiguous():
            raise ValueError("sddmm(reduce='max') needs the forward's contiguous int64 [n_rows, K] argmax")
    else:
        argmax = None
    nnz = adj.nnz()
    dval = torch.empty(nnz, dtype=torch.float32, device=x.device)
    if nnz == 0:
        return dval
    rowptr, col, bits = adj._index_arrays()
    scale = adj._inv_rowcount() if red == 1 else None
    rc = _lib.load().egnn_sddmm_csr_f32(n_rows, n_src, K, _lib.ptr(rowptr), _lib.ptr(col), bits, nnz, _lib.ptr(g), g.stride(0),
                                        _lib.ptr(x), x.stride(0), _lib.ptr(scale), _lib.ptr(argmax), _lib.ptr(dval), _lib.stream())
    _lib.check(rc, "egnn_sddmm_csr_f32")
    return dval


def _fresh(g, tap_box):
    """Marks a gradient this package has just allocated in a backward FOR the tapped tensor whose box is ``tap_box``: nobody else
    holds it yet, so that tensor's ``_GradTap`` may add its row-compact pieces into it in place.  The mark names the box: a gradient
    that reaches a tap through a pass-through node (an add, a view: the same tensor object can then also be a sibling input's
    gradient) was produced for some OTHER tensor, carries no mark for this box, and is copied first."""
    if g is not None and tap_box is not None:
        g._egnn_fresh_for = tap_box
    return g


def colsum(g: Tensor) -> Tensor:
    """Column sums of a [n, C] gradient (bias gradients).  A gradient that comes straight out of the fused BatchNorm
    backward carries them already (formed while dx was written: egnn_bn_act_bwd_f32), tagged with the tensor
    version they belong to -- any in-place change of the gradient since then (autograd accumulation) voids the tag."""
    tag = getattr(g, "_egnn_colsum", None)
    if tag is not None and tag[1] == g._version and tag[0].shape[0] == g.shape[1]:
        return tag[0]
    _lib.require_gpu(g)
    if g.dim() != 2 or g.dtype != torch.float32 or g.shape[0] == 0:
        return g.sum(0)
    # egnn_colsum_f32, not ``g.sum(0)``: torch's multi-block reduction zeroes its semaphores with a memset node, and inside replayed
    # hipGraphs on this stack such reductions were seen to leave their output unwritten (ops_edge._LspLoss)
    g = _rowmajor(g)
    n, C = g.shape
    lib = _lib.load()
    out = torch.empty(C, dtype=torch.float32, device=g.device)
    ws = torch.empty(lib.egnn_colsum_ws_floats(C), dtype=torch.float32, device=g.device)
    _lib.check(lib.egnn_colsum_f32(_lib.ptr(g), g.stride(0), n, C, _lib.ptr(out), _lib.ptr(ws), _lib.stream()), "egnn_colsum_f32")
    return out


class _AddBias(torch.autograd.Function):
    """x + bias (broadcast over rows); the bias gradient is ``colsum`` -- not autograd's ``sum_to_size``, a long torch reduction over
    the node dimension (see _audit.py)."""

    @staticmethod
    def forward(ctx, x, bias):
        return x + bias

    @staticmethod
    def backward(ctx, g):
        return g, (colsum(g) if ctx.needs_input_grad[1] else None)


def add_bias(x: Tensor, bias: Tensor | None) -> Tensor:
    if bias is None:
        return x
    _lib.require_gpu(x)
    return _AddBias.apply(x, bias)


def _value_needs_grad(adj) -> bool:
    v = getattr(adj, "_value", None)
    return v is not None and v.requires_grad and torch.is_grad_enabled()


def spmm(adj, x: Tensor, reduce: str = "sum", bias: Tensor | None = None, bn_stats_shift: Tensor | None = None,
         want_bn_stats: bool = False, addend: Tensor | None = None) -> Tensor:
    """adj @ x with the given reduction; ``bias`` ([K]) is added in the kernel's store (sum / mean only).

    ``want_bn_stats``: the caller will BatchNorm the result next (gnn.py:47-48): the column mean / biased variance are
    formed in the aggregation's epilogue and attached to the returned tensor (``_egnn_bn_stats``) for ``ops.bn_act``;
    ``bn_stats_shift``: shift of the shifted sums (the BatchNorm's running_mean).  Where the kernel in use has no such
    epilogue nothing is attached and ``bn_act`` runs its own statistics pass."""
    if reduce not in _REDUCE:
        raise ValueError(f"unknown reduce '{reduce}'")
    if addend is not None:   # accumulating form (adj @ x + addend), used without autograd by the sharded run's own Functions
        if torch.is_grad_enabled() and (x.requires_grad or addend.requires_grad or _value_needs_grad(adj)):
            raise NotImplementedError("spmm(addend=...) is a forward-only form")
        return spmm_raw(adj, x, reduce, bias=bias, addend=addend)[0]
    if _value_needs_grad(adj):   # learnable entry values: the Function that takes them as a tensor input and returns their gradient
        if adj._value.dtype != torch.float32 or adj._value.dim() != 1:
            raise TypeError("spmm: the values of the adjacency must be a float32 [nnz] vector")

        def apply(*rest):
            return _SpMMValued.apply(x, adj._value, adj, reduce, *rest)
    else:
        def apply(*rest):
            return _SpMM.apply(x, adj, reduce, *rest)
    if bias is not None and (reduce == "max" or (x.shape[1] % 4 == 0 and bias.data_ptr() % 16 != 0)):
        return apply(None)[0] + bias
    y, mean, var = apply(bias, bn_stats_shift, bool(want_bn_stats) and reduce != "max")
    if mean is not None:
        y._egnn_bn_stats = (mean, var, y._version)   # version-checked by bn_act: an in-place edit of y voids the statistics
    return y


def spmm_max_piece(adj, x: Tensor, entry_id: Tensor | None = None, merge: bool = False, y: Tensor | None = None,
                   argmax: Tensor | None = None, src_scale: Tensor | None = None):
    """max-aggregation over ONE PIECE of a row set (egnn_spmm_csr_max_piece_f32): ``adj`` holds some of the rows' entries, ``entry_id``
    [nnz] int64 the id ``argmax`` records for each of them (None: the entry's own position; strictly increasing within a row).
    ``merge=False`` writes (Y, argmax) from scratch; ``merge=True`` merges the piece into the state ``y`` / ``argmax`` hold, in place
    (larger value wins, equal values: smaller id; a state with argmax < 0 is empty).  Returns (Y, argmax).  No autograd: the
    sharded run's ``dist._MaxAggregate`` drives it."""
    _lib.require_gpu(x, adj._col)
    x = _rowmajor(x)
    n_rows, n_src = adj.sparse_sizes()
    if x.shape[0] != n_src:
        raise ValueError(f"spmm_max_piece: adjacency has {n_src} columns, x has {x.shape[0]} rows")
    K = x.shape[1]
    if merge:
        if (y is None or argmax is None or tuple(y.shape) != (n_rows, K) or tuple(argmax.shape) != (n_rows, K) or y.dtype != torch.float32
                or argmax.dtype != torch.int64 or y.stride(1) != 1 or not argmax.is_contiguous()):
            raise ValueError("spmm_max_piece(merge=True) needs the float32 [n_rows, K] / contiguous int64 [n_rows, K] state of the earlier pieces")
    else:
        y = torch.empty(n_rows, K, dtype=torch.float32, device=x.device)
        argmax = torch.empty(n_rows, K, dtype=torch.int64, device=x.device)
    if n_rows == 0 or K == 0:
        return y, argmax
    if adj.nnz() == 0:   # a piece without entries changes no state; from scratch every row is empty
        if not merge:
            y.zero_()
            argmax.fill_(-1)
        return y, argmax
    if entry_id is not None and (entry_id.dtype != torch.int64 or entry_id.numel() != adj.nnz() or not entry_id.is_contiguous()):
        raise ValueError("spmm_max_piece: `entry_id` is a contiguous int64 [nnz] vector")
    rowptr, col, bits = adj._index_arrays()
    op = _spmm_desc(adj, rowptr, col, bits, x, y, _REDUCE["max"], src_scale, None)
    rc = _lib.load().egnn_spmm_csr_max_piece_f32(ctypes.byref(op), _lib.ptr(entry_id), int(bool(merge)), _lib.ptr(argmax), _lib.stream())
    _lib.check(rc, "egnn_spmm_csr_max_piece_f32")
    return y, argmax


def spmm_max_bwd_rows(t_adj, t_eid: Tensor, val: Tensor | None, argmax: Tensor, gy: Tensor, addend: Tensor | None = None) -> Tensor:
    """Backward of a max piece as a gather (egnn_spmm_csr_max_bwd_rows_f32): ``t_adj`` is the TRANSPOSED piece ([n_src, n_rows]: its
    rowptr / col are t_rowptr / t_row), ``t_eid`` [nnz] int64 the forward id of every transposed entry, ``val`` the values indexed by
    forward id (None = 1).  Returns dX [n_src, K] with every row written: ``addend`` + the picked gradients, added in entry order."""
    _lib.require_gpu(gy, t_adj._col)
    gy = _rowmajor(gy)
    n_src, n_rows = t_adj.sparse_sizes()
    K = gy.shape[1]
    if gy.shape[0] != n_rows or tuple(argmax.shape) != (n_rows, K) or argmax.dtype != torch.int64 or not argmax.is_contiguous():
        raise ValueError("spmm_max_bwd_rows: dY is [n_rows, K] and argmax a contiguous int64 [n_rows, K]")
    if addend is not None:
        if tuple(addend.shape) != (n_src, K):
            raise ValueError("spmm_max_bwd_rows: `addend` is a float32 [n_src, K] matrix")
        addend = _rowmajor(addend)
    gx = torch.empty(n_src, K, dtype=torch.float32, device=gy.device)
    if n_src == 0 or K == 0:
        return gx
    if t_adj.nnz() == 0:   # nobody picked anything
        return gx.zero_() if addend is None else gx.copy_(addend)
    if t_eid.dtype != torch.int64 or t_eid.numel() != t_adj.nnz() or not t_eid.is_contiguous():
        raise ValueError("spmm_max_bwd_rows: `t_eid` is a contiguous int64 [nnz] vector")
    rowptr, col, bits = t_adj._index_arrays()
    rc = _lib.load().egnn_spmm_csr_max_bwd_rows_f32(n_src, n_rows, K, _lib.ptr(rowptr), _lib.ptr(col), bits, _lib.ptr(t_eid), _lib.ptr(val),
                                                    _lib.ptr(argmax), _lib.ptr(gy), gy.stride(0), _lib.ptr(addend),
                                                    0 if addend is None else addend.stride(0), _lib.ptr(gx), gx.stride(0), _lib.stream())
    _lib.check(rc, "egnn_spmm_csr_max_bwd_rows_f32")
    return gx


# ------------------------------------------------------------------------------------------------
# row ids that may repeat: the plan of egnn_rows_plan_build_i64 and the run-sum of the gathers' backward (csrc/rows_sum.hip)
# ------------------------------------------------------------------------------------------------
class RowsPlan:
    """What ``duplicates="sum"`` knows about one index tensor: ``idx`` (the wrapped copy when an entry was negative), the counters, and
    -- only when a row is named more than once -- the sorted (row, position) keys ``egnn_rows_add_runs_f32`` walks.  ``all_keys`` are
    the sorted keys whether or not a row repeats (``scatter`` always walks them) and ``rows`` the row ids as ``egnn_scatter_bwd_f32``
    reads them.  A ``deferred`` plan (``rows_plan(check="deferred")``) was built without a host read: ``dups`` / ``negatives`` /
    ``longest`` are unknown (None: "may repeat", the keys are kept), ``idx`` is safe to gather by (an id out of range reads row 0)
    and ``rows`` marks such an id with -1, so it gets no gradient."""
    __slots__ = ("idx", "n_rows", "S", "dups", "negatives", "longest", "keys", "shift", "all_keys", "rows", "deferred")

    def __init__(self, idx, n_rows, S, dups=0, negatives=0, longest=0, keys=None, shift=1, all_keys=None, rows=None, deferred=False):
        self.idx, self.n_rows, self.S, self.dups, self.negatives, self.longest, self.keys, self.shift = idx, n_rows, S, dups, negatives, longest, keys, shift
        self.all_keys, self.rows, self.deferred = all_keys, idx if rows is None else rows, deferred


_ROWS_PLANS = _cache.TensorKeyedCache(capacity=16, max_bytes=1 << 30)
_ROWS_OOB: dict = {}      # device -> int32 [1]: row ids that deferred plans found out of range (and the kernels therefore dropped)


def rows_oob(device, reset: bool = True) -> int:
    """How many row ids the plans built with ``rows_plan(check="deferred")`` on ``device`` found outside [-n_rows, n_rows) since the
    last reset; the kernels dropped those entries.  A host read, made on demand (the deferred plans themselves make none)."""
    c = _ROWS_OOB.get(_indexed_device(device))
    if c is None:
        return 0
    n = int(c.item())
    if reset and n:
        c.zero_()
    return n


def _indexed_device(device) -> torch.device:
    dev = torch.device(device)
    return dev if dev.index is not None or dev.type != "cuda" else torch.device(dev.type, torch.cuda.current_device())


def _rows_plan_launch(ids: Tensor, n_rows: int):
    lib = _lib.load()
    S = ids.numel()
    keys = torch.empty(S, dtype=torch.int64, device=ids.device)      # the bits of the uint64 keys
    counters = torch.empty(4, dtype=torch.int32, device=ids.device)
    nws = lib.egnn_rows_plan_ws_bytes(S, n_rows)
    ws = torch.empty(nws, dtype=torch.uint8, device=ids.device)
    _lib.check(lib.egnn_rows_plan_build_i64(_lib.ptr(ids), S, n_rows, _lib.ptr(keys), _lib.ptr(counters), _lib.ptr(ws), nws, _lib.stream()),
               "egnn_rows_plan_build_i64")
    return keys, counters


def _rows_plan_deferred(idx: Tensor, n_rows: int) -> RowsPlan:
    ids, S = idx.contiguous(), idx.numel()
    if S == 0:
        return RowsPlan(ids, n_rows, 0, None, None, None, deferred=True)
    if n_rows <= 0:     # (known without a read: every id is out of range, and there is no row 0 a dropped id could be gathered as)
        raise IndexError(f"index out of range: {S} row ids into a tensor of {n_rows} rows")
    dev = ids.device
    counter = _ROWS_OOB.get(dev)
    if counter is None:
        if torch.cuda.graphs.is_current_stream_capturing():
            raise RuntimeError("rows_plan(check='deferred'): the device's out-of-range counter does not exist yet and must outlive the graph: "
                               "run one warm-up step (or call ops.rows_oob_counter(device)) before the capture")
        counter = rows_oob_counter(dev)
    keys, counters = _rows_plan_launch(ids, n_rows)
    counter += counters[:1]
    rows = torch.empty_like(ids)
    _lib.check(_lib.load().egnn_rows_wrap_i64(_lib.ptr(ids), S, n_rows, _lib.ptr(rows), _lib.stream()), "egnn_rows_wrap_i64")
    return RowsPlan(rows.clamp_min(0), n_rows, S, None, None, None, keys, max(1, (S - 1).bit_length()), keys, rows, True)


def rows_oob_counter(device) -> Tensor:
    """The int32 [1] counter behind ``rows_oob`` (created on first use; a graph capture needs it to exist beforehand)."""
    dev = _indexed_device(device)
    c = _ROWS_OOB.get(dev)
    if c is None:
        c = _ROWS_OOB[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return c


def rows_plan(idx: Tensor, n_rows: int, check: str = "host") -> RowsPlan:
    """The plan of ``idx`` (1-D int64, GPU) over a tensor of ``n_rows`` rows.

    ``check="host"`` (default): built once per index tensor (identity + version, like the package's other integer preprocessing) with
    ONE host read, of the four counters.  An id outside [-n_rows, n_rows) raises ``IndexError``; the build cannot happen inside a graph
    capture (it reads the counters): a warm-up step builds it.

    ``check="deferred"``: for index tensors that are new every step (``edge_index[:, mask]`` of a mini-batch).  No host read and no
    entry in the identity cache (fresh tensors would evict the long-lived plans); usable inside a graph capture.  Negative ids are
    wrapped on the device, the keys are always kept (``dups`` is unknown: "may repeat"), and an id out of range is DROPPED by the
    kernels -- gathered as row 0, without a gradient, and left out of every aggregation -- and added to the per-device counter that
    ``rows_oob`` reads on demand."""
    if not (isinstance(idx, Tensor) and idx.dtype == torch.int64 and idx.dim() == 1):
        raise TypeError("rows_plan: `idx` must be a 1-D int64 tensor")
    if check not in ("host", "deferred"):
        raise ValueError(f"check must be 'host' or 'deferred', got {check!r}")
    _lib.require_gpu(idx)
    n_rows = int(n_rows)
    if check == "deferred":
        return _rows_plan_deferred(idx, n_rows)

    def build():
        if torch.cuda.graphs.is_current_stream_capturing():
            raise RuntimeError("rows_plan: the plan of an index tensor (duplicates='sum') is built with a host read of its counters and cannot "
                               "be built while a graph is being captured: run one warm-up step with this index tensor before the capture")
        ids, S = idx.contiguous(), idx.numel()
        if S == 0:
            return RowsPlan(ids, n_rows, 0)
        keys, counters = _rows_plan_launch(ids, n_rows)
        oob, dups, neg, longest = counters.tolist()                      # the one host read
        if oob:
            raise IndexError(f"index out of range: {oob} of {S} row ids are outside [-{n_rows}, {n_rows})")
        if neg:
            ids = torch.where(ids < 0, ids + n_rows, ids)
        return RowsPlan(ids, n_rows, S, dups, neg, longest, keys if dups else None, max(1, (S - 1).bit_length()), keys)
    return _ROWS_PLANS.get((idx,), (n_rows,), build)


def _plan_for(idx, n_rows: int, what: str) -> RowsPlan:
    """``idx`` as a plan over ``n_rows`` rows: a ready ``RowsPlan`` (checked against the operand) or the host-checked plan of a tensor."""
    if isinstance(idx, RowsPlan):
        if idx.n_rows != int(n_rows):
            raise ValueError(f"{what}: the plan was built for {idx.n_rows} rows, the operand has {int(n_rows)}")
        return idx
    return rows_plan(idx, n_rows)


def _check_duplicates(duplicates) -> bool:
    if duplicates not in ("unique", "sum"):
        raise ValueError(f"duplicates must be 'unique' or 'sum', got {duplicates!r}")
    return duplicates == "sum"


def _rows_add_runs(dst: Tensor, plan: RowsPlan, rows: Tensor, accumulate: bool) -> None:
    """dst[r] = (dst[r] if accumulate else 0) + the rows of ``rows`` that ``plan`` assigns to r, in the kernel's documented order."""
    rows = _rowmajor(rows)
    lib = _lib.load()
    S, C = rows.shape
    nws = lib.egnn_rows_add_runs_ws_bytes(S, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=rows.device) if nws else None
    _lib.check(lib.egnn_rows_add_runs_f32(_lib.ptr(dst), dst.stride(0), dst.shape[0], _lib.ptr(plan.keys), S, plan.shift, _lib.ptr(rows),
                                          rows.stride(0), C, 1 if accumulate else 0, _lib.ptr(ws), nws, _lib.stream()), "egnn_rows_add_runs_f32")


def _tap_rows_add(g: Tensor, idx, rows: Tensor) -> None:
    """One pending piece of a ``_TapBox`` joins the dense gradient ``g``: ``idx`` is the id tensor (unique ids) or a ``RowsPlan``."""
    rows = _rowmajor(rows)
    if isinstance(idx, RowsPlan):
        _rows_add_runs(g, idx, rows, True)
        return
    _lib.check(_lib.load().egnn_rows_add_f32(_lib.ptr(g), g.stride(0), _lib.ptr(idx), _lib.ptr(rows), rows.stride(0), rows.shape[0],
                                             rows.shape[1], _lib.stream()), "egnn_rows_add_f32")


class _TakeRows(torch.autograd.Function):
    """x[idx]: for UNIQUE row ids the backward is a plain scatter (ATen's index backward sorts the ids every step); with the plan of an
    index that repeats rows (``plan``), the run-sum of csrc/rows_sum.hip into an uninitialised gradient."""

    @staticmethod
    def forward(ctx, x, idx, plan=None):
        ctx.save_for_backward(idx)
        ctx.n, ctx.plan = x.shape[0], plan
        return x.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        if ctx.plan is not None:
            gx = torch.empty(ctx.n, *g.shape[1:], dtype=g.dtype, device=g.device)
            _rows_add_runs(gx.view(ctx.n, -1), ctx.plan, g.reshape(g.shape[0], -1), False)
            return gx, None, None
        gx = torch.zeros(ctx.n, *g.shape[1:], dtype=g.dtype, device=g.device)
        gx.index_copy_(0, idx, g)
        return gx, None, None


def take_rows(x: Tensor, idx: Tensor, duplicates: str = "unique") -> Tensor:
    """``x[idx]`` for a 1-D int64 ``idx``.  ``duplicates="unique"`` (default): the caller knows the ids to be unique and in range;
    nothing is checked.  ``"sum"``: torch's rules for any ``idx`` -- negative ids wrap, an id out of range raises ``IndexError``, and
    the gradients of a row named several times are summed (``rows_plan``; with unique ids the same kernels and bits as "unique").
    ``idx`` may be a ready ``RowsPlan`` (``duplicates`` is then not consulted): nothing is built, and the same plan can serve
    ``scatter``."""
    if isinstance(idx, RowsPlan):
        _lib.require_gpu(x)
    elif not _check_duplicates(duplicates):
        return _TakeRows.apply(x, idx)
    plan = _plan_for(idx, x.shape[0], "take_rows")
    return _TakeRows.apply(x, plan.idx, plan if plan.keys is not None else None)


# ------------------------------------------------------------------------------------------------
# aggregation by an unsorted index (csrc/scatter.hip): torch_scatter.scatter along dim 0, the aggregate step of nn.MessagePassing
# ------------------------------------------------------------------------------------------------
_SCATTER_REDUCE = {"sum": 0, "add": 0, "mean": 1, "max": 2, "min": 3}


class _Scatter(torch.autograd.Function):
    """out[r] = reduce of src[p] over index[p] == r (egnn_scatter_runs_f32 over the plan's sorted keys); the backward is the gather
    form egnn_scatter_bwd_f32 into an uninitialised gradient.  First derivatives only."""

    @staticmethod
    def forward(ctx, src, plan, red):
        src = _rowmajor(src)
        lib = _lib.load()
        S, C = src.shape
        n, dev = plan.n_rows, src.device
        out = torch.empty((n, C), dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev) if red == 1 else None
        arg = torch.empty((n, C), dtype=torch.int64, device=dev) if red >= 2 else None
        nws = lib.egnn_scatter_runs_ws_bytes(S, C, red)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
        _lib.check(lib.egnn_scatter_runs_f32(_lib.ptr(out), out.stride(0), n, _lib.ptr(count), _lib.ptr(arg), _lib.ptr(plan.all_keys), S,
                                             plan.shift if S else 0, _lib.ptr(src), src.stride(0), C, red, _lib.ptr(ws), nws, _lib.stream()),
                   "egnn_scatter_runs_f32")
        ctx.plan, ctx.red, ctx.S, ctx.count, ctx.arg = plan, red, S, count, arg
        if arg is None:
            return out, None
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g, _garg=None):
        g = _rowmajor(g)
        plan, C = ctx.plan, g.shape[1]
        dsrc = torch.empty((ctx.S, C), dtype=torch.float32, device=g.device)
        _lib.check(_lib.load().egnn_scatter_bwd_f32(_lib.ptr(dsrc), dsrc.stride(0), ctx.S, _lib.ptr(plan.rows), plan.n_rows, _lib.ptr(g),
                                                    g.stride(0), C, ctx.red, _lib.ptr(ctx.count), _lib.ptr(ctx.arg), _lib.stream()),
                   "egnn_scatter_bwd_f32")
        return dsrc, None, None


def scatter(src: Tensor, index, dim_size: int, reduce: str = "sum", plan: RowsPlan | None = None, return_arg: bool = False):
    """``out[r] = reduce(src[p] for p with index[p] == r)`` -> [dim_size, ...]: ``torch_scatter.scatter(src, index, 0, dim_size=dim_size)``.
    ``src`` float32 GPU [E, ...] (trailing dims are flattened for the kernel), ``index`` 1-D int64 [E] in any order, with repeats and
    negative ids; ``reduce`` in sum | add | mean | max | min.  No float atomics: sum (and mean's sum) add in the run-sum's documented
    order, so two calls are bit-equal; max / min are exact, a row no id names is 0 and ``arg`` (``return_arg=True``: ``(out, arg)``,
    arg None for sum / mean) holds the smallest position attaining the extreme, E for such a row.  ``plan``: a ready ``rows_plan`` of
    ``index`` over ``dim_size`` rows (``index`` itself may then be None) -- the plan a gather by the same ids used; without one the
    host-checked plan of ``index`` is built (cached per index tensor).  First derivatives."""
    if reduce not in _SCATTER_REDUCE:
        raise ValueError(f"reduce must be one of {sorted(_SCATTER_REDUCE)}, got {reduce!r}")
    fused = getattr(src, "_egnn_gather_scatter", None)     # rows of lazy.py that nobody has formed yet: gather_scatter forms none
    if fused is not None and FUSE_LAZY_ROWS and _SCATTER_REDUCE[reduce] <= 1:
        out = fused(plan if plan is not None else index, dim_size, reduce)
        if out is not None:
            return (out, None) if return_arg else out
    src = _lib.real(src)
    _lib.require_gpu(src, index if isinstance(index, Tensor) else None)
    if src.dtype != torch.float32 or src.dim() < 1:
        raise TypeError("scatter: `src` must be a float32 tensor [E, ...]")
    if plan is None:
        plan = rows_plan(index, dim_size)
    elif plan.n_rows != int(dim_size):
        raise ValueError(f"scatter: the plan was built for {plan.n_rows} rows, dim_size is {int(dim_size)}")
    if plan.S != src.shape[0] or (isinstance(index, Tensor) and index.numel() != src.shape[0]):
        raise ValueError(f"scatter: {src.shape[0]} rows of src, {plan.S} ids")
    tail = tuple(src.shape[1:])
    C = 1
    for d in tail:
        C *= d
    if C == 0 or int(dim_size) == 0:
        out = src.new_zeros((int(dim_size),) + tail)
        return (out, None) if return_arg else out
    out, arg = _Scatter.apply(src.reshape(src.shape[0], C), plan, _SCATTER_REDUCE[reduce])
    out = out.view((plan.n_rows,) + tail)
    if return_arg:
        return out, (arg.view((plan.n_rows,) + tail) if arg is not None else None)
    return out


# ------------------------------------------------------------------------------------------------
# lift, per-edge weight and aggregation in one walk (csrc/gather_scatter.hip): no [E, C] message tensor forward or backward
# ------------------------------------------------------------------------------------------------
# nn.MessagePassing's default message and the unformed rows of lazy.py (accel) go to gather_scatter instead of take_rows + scatter.
# On: DESIGN 3.5c's condition (the fused median does not exceed the unfused composition's at the two C = 256 full-graph cases) held:
# 2.61 against 4.60 ms without and 3.37 against 8.24 ms with a weight, forward + backward (profiles/gather_scatter_bench.jsonl).
FUSE_LAZY_ROWS = True


def _gather_scatter_launch(out, count, keys, S, shift, frm, x, from_count, w, C, red) -> None:
    lib = _lib.load()
    nws = lib.egnn_gather_scatter_ws_bytes(S, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
    _lib.check(lib.egnn_gather_scatter_runs_f32(_lib.ptr(out), out.stride(0), out.shape[0], _lib.ptr(count), _lib.ptr(keys), S, shift if S else 0,
                                                _lib.ptr(frm), _lib.ptr(x), x.stride(0), x.shape[0], _lib.ptr(from_count), _lib.ptr(w),
                                                w.stride(0) if w is not None else 0, w.shape[1] if w is not None else 1, C, red, _lib.ptr(ws), nws,
                                                _lib.stream()), "egnn_gather_scatter_runs_f32")


class _GatherScatter(torch.autograd.Function):
    """out[r] = sum | mean over dst[p] == r of x[src[p]] * w[p] (egnn_gather_scatter_runs_f32 over the target plan's keys).  Backward:
    dx by the same entry point over the source plan's keys (it gathers g by the target rows), dw by egnn_edge_dot_f32; only for the
    operands that need one, into uninitialised gradients.  First derivatives only."""

    @staticmethod
    def forward(ctx, x, w, plan_src, plan_dst, red):
        x = _rowmajor(x)
        w = None if w is None else _rowmajor(w)
        S, n, C = plan_dst.S, plan_dst.n_rows, x.shape[1]
        out = torch.empty((n, C), dtype=torch.float32, device=x.device)
        count = torch.empty(n, dtype=torch.int32, device=x.device) if red == 1 else None
        _gather_scatter_launch(out, count, plan_dst.all_keys, S, plan_dst.shift, plan_src.idx, x, None, w, C, red)
        ctx.plans, ctx.count = (plan_src, plan_dst), count
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _rowmajor(g)
        x, w = ctx.saved_tensors
        plan_src, plan_dst = ctx.plans
        S, C = plan_dst.S, x.shape[1]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((plan_src.n_rows, C), dtype=torch.float32, device=g.device)
            _gather_scatter_launch(dx, None, plan_src.all_keys, S, plan_src.shift, plan_dst.rows, g, ctx.count, w, C, 0)
        if w is not None and ctx.needs_input_grad[1]:
            dw = torch.empty(w.shape, dtype=torch.float32, device=g.device)
            _lib.check(_lib.load().egnn_edge_dot_f32(_lib.ptr(dw), dw.stride(0), S, w.shape[1], C, _lib.ptr(plan_dst.rows), _lib.ptr(g), g.stride(0),
                                                     g.shape[0], _lib.ptr(plan_src.idx), _lib.ptr(x), x.stride(0), x.shape[0],
                                                     _lib.ptr(ctx.count), _lib.stream()), "egnn_edge_dot_f32")
        return dx, dw, None, None, None


def _endpoint_plan(end, n_rows: int, what: str) -> RowsPlan:
    """One endpoint of ``gather_scatter`` as a plan: a ready ``RowsPlan``, the plan the running ``propagate`` call holds for this very
    tensor (``nn.running_end_plan``), or the host-checked plan of the tensor."""
    if not isinstance(end, RowsPlan):
        if not (isinstance(end, Tensor) and end.dtype == torch.int64 and end.dim() == 1):
            raise TypeError(f"gather_scatter: `{what}` must be a 1-D int64 tensor or a RowsPlan")
        from . import nn as _nn
        running = _nn.running_end_plan(end, n_rows, what)
        if running is not None:
            return running
    return _plan_for(end, n_rows, f"gather_scatter ({what})")


def gather_scatter(x: Tensor, src, dst, dim_size: int, weight: Tensor | None = None, reduce: str = "sum") -> Tensor:
    """``out[r] = reduce over the edges p with dst[p] == r of x[src[p]] * weight[p]`` -> [dim_size, ...]: the lift, the per-edge weight
    and the aggregation of a message-passing layer in ONE kernel walk, forward and backward, without an [E, C] tensor.  ``x`` float32
    GPU [N_src, ...] (trailing dims are flattened for the kernel); ``src`` / ``dst`` each a 1-D int64 tensor [E] (any order, repeats,
    negative ids) or a ready ``RowsPlan`` (over N_src / ``dim_size`` rows); ``weight`` None, [E], [E, 1], [E, H] or [E, H, 1] with H
    dividing the flattened width (head h weighs the h-th block of C / H columns; for ``x`` [N, H, D], H is ``x.shape[1]``);
    ``reduce`` in sum | add | mean.  The value and every gradient except ``weight``'s are bit-equal to
    ``scatter(take_rows(x, plan_src) * weight, None, dim_size, reduce, plan=plan_dst)`` -- the same order of additions, and with
    deferred plans the same treatment of ids out of range (a dropped source id reads row 0 and gets no gradient, a dropped target id
    is left out and its weight gets gradient 0).  ``weight``'s gradient is the per-edge dot of ``egnn_edge_dot_f32`` (a fixed order
    of its own).  Each plan is built at most once (cached per index tensor; inside a running ``propagate`` the call's own plans are
    taken).  First derivatives."""
    if reduce not in _SCATTER_REDUCE:
        raise ValueError(f"reduce must be one of ['add', 'mean', 'sum'], got {reduce!r}")
    if _SCATTER_REDUCE[reduce] > 1:
        raise ValueError(f"gather_scatter: reduce must be sum, add or mean; {reduce!r} keeps an argument per element: use ops.scatter")
    x = _lib.real(x)
    if not isinstance(x, Tensor) or x.dtype != torch.float32 or x.dim() < 1:
        raise TypeError("gather_scatter: `x` must be a float32 tensor [N, ...]")
    dim_size = int(dim_size)
    C = 1
    for d in x.shape[1:]:
        C *= d
    E = src.S if isinstance(src, RowsPlan) else (src.numel() if isinstance(src, Tensor) else None)
    E_dst = dst.S if isinstance(dst, RowsPlan) else (dst.numel() if isinstance(dst, Tensor) else None)
    if E is not None and E_dst is not None and E != E_dst:
        raise ValueError(f"gather_scatter: {E} source ids, {E_dst} target ids")
    for end, n, what in ((src, x.shape[0], "src"), (dst, dim_size, "dst")):
        if isinstance(end, RowsPlan) and end.n_rows != n:
            raise ValueError(f"gather_scatter ({what}): the plan was built for {end.n_rows} rows, the operand has {n}")
    w2 = None
    if weight is not None:
        weight = _lib.real(weight)
        if not isinstance(weight, Tensor) or weight.dtype != torch.float32:
            raise TypeError("gather_scatter: `weight` must be a float32 tensor")
        if weight.dim() not in (1, 2, 3) or (weight.dim() == 3 and weight.shape[2] != 1):
            raise ValueError(f"gather_scatter: `weight` is [E], [E, 1], [E, H] or [E, H, 1], got {list(weight.shape)}")
        if E is not None and weight.shape[0] != E:
            raise ValueError(f"gather_scatter: {weight.shape[0]} weights for {E} edges")
        H = weight.shape[1] if weight.dim() > 1 else 1
        if H < 1 or (H > 1 and (C % H != 0 or (x.dim() == 3 and H != x.shape[1]))):
            raise ValueError(f"gather_scatter: {H} weight columns do not divide x's {list(x.shape[1:])} into heads")
        w2 = weight.reshape(weight.shape[0], H)
    _lib.require_gpu(x, w2, src if isinstance(src, Tensor) else None, dst if isinstance(dst, Tensor) else None)
    plan_src = _endpoint_plan(src, x.shape[0], "src")
    plan_dst = _endpoint_plan(dst, dim_size, "dst")
    if plan_src.S != plan_dst.S:
        raise ValueError(f"gather_scatter: {plan_src.S} source ids, {plan_dst.S} target ids")
    if C == 0 or dim_size == 0:
        return x.new_zeros((dim_size,) + tuple(x.shape[1:]))
    out = _GatherScatter.apply(x.reshape(x.shape[0], C), w2, plan_src, plan_dst, _SCATTER_REDUCE[reduce])
    return out.view((dim_size,) + tuple(x.shape[1:]))


# ------------------------------------------------------------------------------------------------
# lift, the edge's own row, activation and aggregation in one walk (csrc/gather_edge_scatter.hip): relu(x_j + edge_attr) without an
# [E, C] message tensor forward, and with dedge as the only [E, C] tensor backward
# ------------------------------------------------------------------------------------------------
# nn.GINEConv and the unformed `x_j + edge_attr` of lazy.py (accel) go to gather_add_scatter instead of take_rows + add + relu + scatter.
# On: DESIGN 3.5d's condition (3.5c's: the fused median does not exceed the unfused composition's at both cases of tools/gine_bench.py)
# held: 5.04 against 8.06 ms at the arxiv message graph (C = 256) and 0.211 against 0.284 ms on a molhiv_like batch of 512 graphs
# (C = 300), forward + backward (profiles/gine_bench.jsonl).
FUSE_EDGE_ROWS = True
_EDGE_ACTS = {None: 0, "relu": 1}      # act -> the forward's mode of egnn_gather_edge_scatter_runs_f32 (2, GATE, is relu's backward)


def _gather_edge_scatter_launch(out, count, keys, S, shift, frm, x, from_count, e, own, mode, C, red) -> None:
    lib = _lib.load()
    nws = lib.egnn_gather_edge_scatter_ws_bytes(S, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
    _lib.check(lib.egnn_gather_edge_scatter_runs_f32(_lib.ptr(out), out.stride(0), out.shape[0], _lib.ptr(count), _lib.ptr(keys), S,
                                                     shift if S else 0, _lib.ptr(frm), _lib.ptr(x), x.stride(0), x.shape[0], _lib.ptr(from_count),
                                                     _lib.ptr(e), e.stride(0) if e is not None else 0, _lib.ptr(own),
                                                     own.stride(0) if own is not None else 0, mode, C, red, _lib.ptr(ws), nws, _lib.stream()),
               "egnn_gather_edge_scatter_runs_f32")


class _GatherAddScatter(torch.autograd.Function):
    """out[r] = sum | mean over dst[p] == r of act(x[src[p]] + edge[p]) (egnn_gather_edge_scatter_runs_f32 over the target plan's keys).
    Backward: dx by the same entry point over the source plan's keys in GATE mode (ADD without an edge operand for act=None: it gathers
    g by the target rows), dedge by egnn_edge_gate_f32; only for the operands that need one, into uninitialised gradients.  Saves x,
    edge and the counts; dedge is the only [E, C] tensor of either direction.  First derivatives only."""

    @staticmethod
    def forward(ctx, x, edge, plan_src, plan_dst, mode, red):
        x, edge = _rowmajor(x), _rowmajor(edge)
        S, n, C = plan_dst.S, plan_dst.n_rows, x.shape[1]
        out = torch.empty((n, C), dtype=torch.float32, device=x.device)
        count = torch.empty(n, dtype=torch.int32, device=x.device) if red == 1 else None
        _gather_edge_scatter_launch(out, count, plan_dst.all_keys, S, plan_dst.shift, plan_src.idx, x, None, edge, None, mode, C, red)
        ctx.plans, ctx.count, ctx.mode = (plan_src, plan_dst), count, mode
        ctx.save_for_backward(x, edge)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _rowmajor(g)
        x, edge = ctx.saved_tensors
        plan_src, plan_dst = ctx.plans
        S, C, relu = plan_dst.S, x.shape[1], ctx.mode == 1
        dx = dedge = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((plan_src.n_rows, C), dtype=torch.float32, device=g.device)
            _gather_edge_scatter_launch(dx, None, plan_src.all_keys, S, plan_src.shift, plan_dst.rows, g, ctx.count, edge if relu else None,
                                        x if relu else None, 2 if relu else 0, C, 0)
        if ctx.needs_input_grad[1]:
            dedge = torch.empty((S, C), dtype=torch.float32, device=g.device)
            _lib.check(_lib.load().egnn_edge_gate_f32(_lib.ptr(dedge), dedge.stride(0), S, C, _lib.ptr(plan_src.idx), _lib.ptr(x), x.stride(0),
                                                      x.shape[0], _lib.ptr(edge), edge.stride(0), _lib.ptr(plan_dst.rows), _lib.ptr(g),
                                                      g.stride(0), g.shape[0], _lib.ptr(ctx.count), ctx.mode, _lib.stream()),
                       "egnn_edge_gate_f32")
        return dx, dedge, None, None, None, None


def gather_add_scatter(x: Tensor, src, dst, dim_size: int, edge: Tensor, act: str | None = "relu", reduce: str = "sum") -> Tensor:
    """``out[r] = reduce over the edges p with dst[p] == r of act(x[src[p]] + edge[p])`` -> [dim_size, C]: the lift, the edge's own
    feature row, the activation and the aggregation of an edge-feature conv (GINE's ``relu(x_j + edge_attr)``) in ONE kernel walk.
    ``x`` float32 GPU [N_src, C], ``edge`` float32 GPU [E, C]; ``src`` / ``dst`` each a 1-D int64 tensor [E] or a ready ``RowsPlan``,
    resolved as ``gather_scatter`` resolves them; ``act`` "relu" or None; ``reduce`` in sum | add | mean.  No [E, C] tensor is
    allocated forward, and ``edge``'s gradient is the only one backward.  The value and both gradients are bit-equal to
    ``scatter(torch.relu(take_rows(x, plan_src) + edge), None, dim_size, reduce, plan=plan_dst)`` and its autograd gradients
    (relu'(0) = 0) -- the same order of additions, and with deferred plans the same treatment of ids out of range.  With
    ``FUSE_EDGE_ROWS`` off that composition runs instead.  First derivatives."""
    if reduce not in _SCATTER_REDUCE:
        raise ValueError(f"reduce must be one of ['add', 'mean', 'sum'], got {reduce!r}")
    if _SCATTER_REDUCE[reduce] > 1:
        raise ValueError(f"gather_add_scatter: reduce must be sum, add or mean; {reduce!r} keeps an argument per element: use ops.scatter")
    if act not in _EDGE_ACTS:
        raise ValueError(f"gather_add_scatter: act must be 'relu' or None, got {act!r}")
    x, edge = _lib.real(x), _lib.real(edge)
    if not isinstance(x, Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("gather_add_scatter: `x` must be a float32 tensor [N, C]")
    if not isinstance(edge, Tensor) or edge.dtype != torch.float32 or edge.dim() != 2:
        raise TypeError("gather_add_scatter: `edge` must be a float32 tensor [E, C]")
    if edge.shape[1] != x.shape[1]:
        raise ValueError(f"gather_add_scatter: `edge` has {edge.shape[1]} columns, `x` has {x.shape[1]}")
    dim_size = int(dim_size)
    E = edge.shape[0]
    for end, n, what in ((src, x.shape[0], "src"), (dst, dim_size, "dst")):
        if isinstance(end, RowsPlan):
            if end.n_rows != n:
                raise ValueError(f"gather_add_scatter ({what}): the plan was built for {end.n_rows} rows, the operand has {n}")
        elif not (isinstance(end, Tensor) and end.dtype == torch.int64 and end.dim() == 1):
            raise TypeError(f"gather_add_scatter: `{what}` must be a 1-D int64 tensor or a RowsPlan")
        if (end.S if isinstance(end, RowsPlan) else end.numel()) != E:
            raise ValueError(f"gather_add_scatter: {end.S if isinstance(end, RowsPlan) else end.numel()} {what} ids for {E} edge rows")
    _lib.require_gpu(x, edge, src if isinstance(src, Tensor) else None, dst if isinstance(dst, Tensor) else None)
    plan_src = _endpoint_plan(src, x.shape[0], "src")
    plan_dst = _endpoint_plan(dst, dim_size, "dst")
    if not FUSE_EDGE_ROWS:
        m = take_rows(x, plan_src) + edge
        return scatter(torch.relu(m) if act == "relu" else m, None, dim_size, reduce, plan=plan_dst)
    if x.shape[1] == 0 or dim_size == 0:
        return x.new_zeros((dim_size, x.shape[1]))
    return _GatherAddScatter.apply(x, edge, plan_src, plan_dst, _EDGE_ACTS[act], _SCATTER_REDUCE[reduce])


# ------------------------------------------------------------------------------------------------
# softmax over the groups of an unsorted index (csrc/scatter_softmax.hip): torch_scatter.scatter_softmax along dim 0, the attention
# step of a user-defined conv between the lift and the aggregation
# ------------------------------------------------------------------------------------------------
class _ScatterSoftmax(torch.autograd.Function):
    """out[p] = softmax (log: log-softmax) of src[p] among the positions that share index[p] (egnn_scatter_softmax_fwd_f32 over the
    plan's sorted keys); the backward is one more run walk and a gather (egnn_scatter_softmax_bwd_f32) into an uninitialised
    gradient.  Saves ``out`` and the plan.  First derivatives only."""

    @staticmethod
    def forward(ctx, src, plan, eps, log):
        src = _rowmajor(src)
        lib = _lib.load()
        S, C = src.shape
        n, dev = plan.n_rows, src.device
        out = torch.empty((S, C), dtype=torch.float32, device=dev)
        stats = torch.empty((2, n, C), dtype=torch.float32, device=dev)
        nws = lib.egnn_scatter_softmax_ws_bytes(S, C)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
        _lib.check(lib.egnn_scatter_softmax_fwd_f32(_lib.ptr(out), out.stride(0), _lib.ptr(stats[0]), _lib.ptr(stats[1]), n,
                                                    _lib.ptr(plan.all_keys), S, plan.shift, _lib.ptr(plan.rows), _lib.ptr(src), src.stride(0), C,
                                                    float(eps), int(log), _lib.ptr(ws), nws, _lib.stream()), "egnn_scatter_softmax_fwd_f32")
        ctx.plan, ctx.log = plan, int(log)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _rowmajor(g)
        (out,) = ctx.saved_tensors
        plan = ctx.plan
        lib = _lib.load()
        S, C = out.shape
        dsrc = torch.empty((S, C), dtype=torch.float32, device=g.device)
        dot = torch.empty((plan.n_rows, C), dtype=torch.float32, device=g.device)
        nws = lib.egnn_scatter_softmax_ws_bytes(S, C)
        ws = torch.empty(nws, dtype=torch.uint8, device=g.device) if nws else None
        _lib.check(lib.egnn_scatter_softmax_bwd_f32(_lib.ptr(dsrc), dsrc.stride(0), _lib.ptr(dot), plan.n_rows, _lib.ptr(plan.all_keys), S,
                                                    plan.shift, _lib.ptr(plan.rows), _lib.ptr(out), out.stride(0), _lib.ptr(g), g.stride(0), C,
                                                    ctx.log, _lib.ptr(ws), nws, _lib.stream()), "egnn_scatter_softmax_bwd_f32")
        return dsrc, None, None, None


def scatter_softmax(src: Tensor, index, dim_size: int, plan: RowsPlan | None = None, eps: float = 0.0, log: bool = False) -> Tensor:
    """``out[p] = exp(src[p] - M[r]) / (Z[r] + eps)`` with ``r = index[p]``, ``M[r]`` the maximum and ``Z[r] = sum exp(src - M[r])`` over
    the positions that name ``r`` (``log=True``: ``(src[p] - M[r]) - log(Z[r] + eps)``): ``torch_scatter.scatter_softmax`` /
    ``scatter_log_softmax`` along dim 0 (``eps=0``) and ``torch_geometric.utils.softmax`` (``eps=1e-16``).  ``src`` float32 GPU
    [E, ...] (trailing dims -- the heads -- are flattened for the kernel; the result has the shape of ``src``), ``index`` 1-D int64
    [E] in any order, with repeats and negative ids.  No float atomics: the sums are added in the kernel's documented order, so two
    calls are bit-equal and the columns are independent of one another.  ``plan`` as in ``scatter``: a ready ``rows_plan`` of
    ``index`` over ``dim_size`` rows (``index`` itself may then be None; an id that a deferred plan dropped gets 0 and no gradient);
    without one the host-checked plan of ``index`` is built (cached per index tensor).  First derivatives."""
    if plan is not None and plan.n_rows != int(dim_size):
        raise ValueError(f"scatter_softmax: the plan was built for {plan.n_rows} rows, dim_size is {int(dim_size)}")
    src = _lib.real(src)
    _lib.require_gpu(src, index if isinstance(index, Tensor) else None)
    if src.dtype != torch.float32 or src.dim() < 1:
        raise TypeError("scatter_softmax: `src` must be a float32 tensor [E, ...]")
    if plan is None and not isinstance(index, Tensor):
        raise TypeError("scatter_softmax: `index` must be a 1-D int64 tensor when no plan is given")
    ids = plan.S if plan is not None else index.numel()
    if ids != src.shape[0] or (isinstance(index, Tensor) and index.numel() != src.shape[0]):
        raise ValueError(f"scatter_softmax: {src.shape[0]} rows of src, {ids} ids")
    C = 1
    for d in src.shape[1:]:
        C *= d
    if C == 0 or src.shape[0] == 0 or int(dim_size) == 0:      # nothing to normalise: no plan, no launch
        return torch.zeros_like(src)
    if plan is None:
        plan = rows_plan(index, dim_size)
    return _ScatterSoftmax.apply(src.reshape(src.shape[0], C), plan, float(eps), bool(log)).view(src.shape)


# ------------------------------------------------------------------------------------------------
# dense GEMM (fp32 MFMA)
# ------------------------------------------------------------------------------------------------
def gemm_backend() -> str:
    """Always 'hip': every GEMM of the package runs on the hand-written kernels (egnn_gemm_f32 and relatives).  The
    rocBLAS comparison lives in tools/kernel_bench.py, outside the product."""
    return "hip"


def _pitch_ok(t: Tensor) -> bool:
    """2-D, unit column stride, rows 16-byte aligned: the kernels' float4 path takes it as it is."""
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def _gemm_operand(t: Tensor) -> Tensor:
    """A row-major view the kernels can address: kept as it is when only its row pitch is padded (see pad_pitch)."""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    return _rowmajor(t)


def pad_pitch(t: Tensor) -> Tensor:
    """The same [n, C] values behind a row pitch that is a multiple of 4 floats (a view of an [n, C+pad] buffer), so
    that rows start 16-byte aligned and the GEMM / gather kernels can use float4 loads (C = 750 teacher features)."""
    n, C = t.shape
    if C % 4 == 0 and _pitch_ok(t):
        return t
    buf = torch.zeros(n, (C + 3) // 4 * 4, dtype=t.dtype, device=t.device)
    buf[:, :C] = t
    return buf[:, :C]


def gemm_raw(a: Tensor, b: Tensor, trans_a: bool = False, trans_b: bool = False, bias: Tensor | None = None,
             alpha: float = 1.0, split_k: int | None = None, a_rows: Tensor | None = None, b_rows: Tensor | None = None,
             relu: bool = False, addend: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """C = alpha * op(a) @ op(b) (+ bias) (+ addend [M,N], added in the kernel's store) via egnn_gemm_f32 / egnn_gemm_rows_f32.

    a_rows [M] (trans_a False): op(a) = a[a_rows];  b_rows [K] (trans_b False): b = b[b_rows] -- the gather is fused
    into the operand load.
    ``out``: a caller-owned float32 [M, N] view with unit column stride and ``out.stride(0) >= N`` (a column block of a wider
    buffer) that receives the product and is returned; None allocates."""
    _lib.require_gpu(a, b)
    a, b = _gemm_operand(a), _gemm_operand(b)
    if a_rows is not None:
        M, K = a_rows.numel(), a.shape[1]
    else:
        M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    if b_rows is not None:
        Kb, N = b_rows.numel(), b.shape[1]
    else:
        Kb, N = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if K != Kb:
        raise ValueError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    if out is not None:
        _lib.require_gpu(out)
        if (out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (M, N) or out.device != a.device
                or (N > 1 and out.stride(1) != 1) or (M > 1 and out.stride(0) < N)):
            raise ValueError(f"gemm_raw: `out` must be a float32 [{M}, {N}] view with unit column stride and a row pitch >= {N}")
    if K == 0 or M == 0 or N == 0:
        # an empty reduction (dW = dY^T X[rows] on a shard that owns no train row) or an empty output: exact zeros (+ bias / addend),
        # no launch -- the entry points take non-null operands only
        c = torch.zeros(M, N, dtype=torch.float32, device=a.device)
        if bias is not None and M > 0 and N > 0:
            c += bias
        if addend is not None:
            c += addend
        c = c.clamp_(min=0) if relu else c
        return c if out is None else out.copy_(c)
    c = torch.empty(M, N, dtype=torch.float32, device=a.device) if out is None else out
    ldc = c.stride(0) if M > 1 else max(c.stride(0), N)
    if split_k is None:
        # reductions over many rows into a small output (dW = X^T dY): spread K over the chip
        # (two workgroups per CU = 512 slots: 2 or 4 output tiles take 128 ranges -- 163 vs 178 us on 256 x 256 x 169 343, 106 vs 140 us on
        # 128 x 256 x 169 343; from 6 tiles on 64 ranges stay ahead: profiles/r05_splitk_sweep.txt)
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        split_k = 1 if tiles >= 128 or K < 4096 else max(1, min(128 if tiles <= 4 else 64, 512 // max(tiles, 1), K // 1024))
    lib = _lib.load()
    ws = None
    # split-K partials, the skinny kernels' row-chunk partials, the bf16 planes of a small B operand (gemm_split.h)
    nws = lib.egnn_gemm_ws_floats(int(trans_a), int(trans_b), M, N, K, split_k)
    if a_rows is not None or b_rows is not None:
        nws = max(nws, split_k * M * N if split_k > 1 else 0)
    if nws > 0:
        ws = torch.empty(nws, dtype=torch.float32, device=a.device)
    if addend is not None:
        if a_rows is not None or b_rows is not None or relu or tuple(addend.shape) != (M, N):
            raise ValueError("gemm_raw: `addend` is an [M, N] matrix (no fused gather, no ReLU)")
        addend = _rowmajor(addend)
        rc = lib.egnn_gemm_add_f32(int(trans_a), int(trans_b), M, N, K, float(alpha), _lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0),
                                   _lib.ptr(bias), _lib.ptr(addend), addend.stride(0), _lib.ptr(c), ldc, split_k, _lib.ptr(ws),
                                   0 if ws is None else ws.numel() * 4, _lib.stream())
        _lib.check(rc, "egnn_gemm_add_f32")
    elif a_rows is None and b_rows is None:
        rc = lib.egnn_gemm_ex_f32(int(trans_a), int(trans_b), M, N, K, float(alpha), _lib.ptr(a), a.stride(0), _lib.ptr(b),
                                  b.stride(0), _lib.ptr(bias), _lib.ptr(c), ldc, split_k, _lib.ptr(ws),
                                  0 if ws is None else ws.numel() * 4, 1 if relu else 0, _lib.stream())
        _lib.check(rc, "egnn_gemm_ex_f32")
    else:
        _lib.require_gpu(*(t for t in (a_rows, b_rows) if t is not None))
        rc = lib.egnn_gemm_rows_f32(int(trans_a), int(trans_b), M, N, K, float(alpha), _lib.ptr(a), a.stride(0), _lib.ptr(a_rows),
                                    _lib.ptr(b), b.stride(0), _lib.ptr(b_rows), _lib.ptr(bias), _lib.ptr(c), ldc, split_k,
                                    _lib.ptr(ws), 0 if ws is None else ws.numel() * 4, _lib.stream())
        _lib.check(rc, "egnn_gemm_rows_f32")
        if relu:
            c.clamp_(min=0)
    return c


def gemm_last_route() -> int:
    """Which kernel this thread's last gemm_raw call ran (egnn_gemm_last_route; encoding in include/egnn_hip.h): low byte = form
    (1 skinny_fwd_tile ... 8 general 128x128), bit 8 vec4, bit 9 wide_store, bit 10 split pipe, bits 11 / 12 gather A / B, bits 16+ the
    split_k in effect.  0 when the call launched nothing."""
    return int(_lib.load().egnn_gemm_last_route())


def bn_fold(weight: Tensor, bias: Tensor | None, bn: "torch.nn.BatchNorm1d"):
    """(W', b') with  relu(bn_eval(x W + b)) == relu(x W' + b')  (egnn_bn_fold_f32): an eval-mode BatchNorm1d folded into the
    [in, out] weight and the bias of the layer in front of it -- also across a (linear) aggregation between the two."""
    _lib.require_gpu(weight, bn.running_mean)
    w = _rowmajor(weight.detach())
    rows, C = w.shape
    wo = torch.empty(rows, C, dtype=torch.float32, device=w.device)
    bo = torch.empty(C, dtype=torch.float32, device=w.device)
    rc = _lib.load().egnn_bn_fold_f32(_lib.ptr(w), w.stride(0), rows, C, _lib.ptr(None if bias is None else bias.detach()),
                                      _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), _lib.ptr(None if bn.weight is None else bn.weight.detach()),
                                      _lib.ptr(None if bn.bias is None else bn.bias.detach()), float(bn.eps), _lib.ptr(wo), wo.stride(0), _lib.ptr(bo),
                                      _lib.stream())
    _lib.check(rc, "egnn_bn_fold_f32")
    return wo, bo


class _MatMul(torch.autograd.Function):
    """y = x @ w (+ bias); w stored [K,N] (``transposed=False``, GCNConv) or [N,K] (nn.Linear layout)."""

    @staticmethod
    def forward(ctx, x, w, bias, transposed):
        ctx.save_for_backward(x, w)
        ctx.transposed, ctx.has_bias = transposed, bias is not None
        ctx.tap_box = getattr(x, "_egnn_tap", None)
        return gemm_raw(x, w, False, transposed, bias)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _rowmajor(gy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = gemm_raw(gy, w, False, not ctx.transposed)           # dX = dY W^T  (or dY W)
        if ctx.needs_input_grad[1]:
            gw = gemm_raw(gy, x, True, False) if ctx.transposed else gemm_raw(x, gy, True, False)  # dW = dY^T X | X^T dY
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = colsum(gy)
        return _fresh(gx, ctx.tap_box), gw, gb, None


def _matmul_into(x, w, bias, transposed, out):
    """The ``out=`` form of matmul / linear: the product lands in the caller's view.  Forward-only, like ``spmm(addend=...)``: an
    autograd node cannot hand out a view of somebody else's buffer; the hop-batched Functions (``linear_blocks``) own theirs."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w, bias)):
        raise NotImplementedError("matmul / linear (out=...) is a forward-only form")
    return gemm_raw(x, w, False, transposed, bias, out=out)


def matmul(x: Tensor, w: Tensor, bias: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """x [M,K] @ w [K,N] (+ bias [N], added in the GEMM's store); ``out``: see ``gemm_raw`` (forward-only)."""
    if out is not None:
        return _matmul_into(x, w, bias, False, out)
    return _MatMul.apply(x, w, bias, False)


class _SageLayer(torch.autograd.Function):
    """SAGEConv (PyG <= 1.7: ``lin_l(aggr_j x_j) + lin_r(x_i)``; gnn.py:79-84) as ONE node of the autograd graph, so that
    neither ``lin_l(..) + lin_r(..)`` nor the two-path sum of the input gradient is an element-wise pass over [N, C]: the second
    product of each pair is added in the store of the kernel that forms it (GEMM ``addend`` / SpMM ``addend``).
    ``narrow``: aggregate ``x W_l^T`` instead of x (mean / sum are linear; taken when out < in: the gather moves `out` floats)."""

    @staticmethod
    def forward(ctx, x, adj, wl, bl, wr, reduce, narrow):
        ctx.tap_box = getattr(x, "_egnn_tap", None)
        x = _rowmajor(x)
        r = gemm_raw(x, wr, False, True)                                   # lin_r(x)
        if narrow:
            t = gemm_raw(x, wl, False, True)                               # x W_l^T, then aggregated with bias + lin_r(x) in the store
            out = spmm_raw(adj, t, reduce, bias=bl, addend=r)[0]
            agg = None
        else:
            agg = spmm_raw(adj, x, reduce)[0]
            out = gemm_raw(agg, wl, False, True, bias=bl, addend=r)        # lin_l(agg) + lin_r(x) in one store
        ctx.save_for_backward(x, wl, wr, *([] if agg is None else [agg]))
        ctx.adj, ctx.reduce, ctx.narrow, ctx.has_bias = adj, reduce, narrow, bl is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, wl, wr = ctx.saved_tensors[:3]
        agg = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        adj, reduce = ctx.adj, ctx.reduce
        g = _rowmajor(g)
        need_x = ctx.needs_input_grad[0]
        scale = adj._inv_rowcount() if reduce == "mean" else None          # dX = A^T (dY / cnt) for the mean
        gx = gwl = gbl = gwr = None
        if ctx.needs_input_grad[4]:
            gwr = gemm_raw(g, x, True, False)                              # dW_r = g^T x
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gbl = colsum(g)
        if ctx.narrow:
            need_t = need_x or ctx.needs_input_grad[2]
            dt = spmm_raw(adj.t(), g, "sum", src_scale=scale)[0] if need_t else None
            if ctx.needs_input_grad[2]:
                gwl = gemm_raw(dt, x, True, False)                         # dW_l = dt^T x
            if need_x:
                gx = gemm_raw(dt, wl, False, False, addend=gemm_raw(g, wr, False, False))     # dt W_l + g W_r
        else:
            if ctx.needs_input_grad[2]:
                gwl = gemm_raw(g, agg, True, False)                        # dW_l = g^T agg
            if need_x:
                d_agg = gemm_raw(g, wl, False, False)
                gx = spmm_raw(adj.t(), d_agg, "sum", src_scale=scale, addend=gemm_raw(g, wr, False, False))[0]   # A^T d_agg + g W_r
        return _fresh(gx, ctx.tap_box), None, gwl, gbl, gwr, None, None


class _LinearAdd(torch.autograd.Function):
    """x @ w^T + bias + addend with the sum formed in the GEMM's store (egnn_gemm_add_f32): SAGEConv's ``lin_l(agg) + lin_r(x)`` on
    node-range shards, where the aggregation is a collective operator of its own (dist._OverlapAggregate)."""

    @staticmethod
    def forward(ctx, x, w, bias, addend):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.tap_box = getattr(x, "_egnn_tap", None)
        return gemm_raw(x, w, False, True, bias, addend=addend)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _rowmajor(gy)
        gx = gemm_raw(gy, w, False, False) if ctx.needs_input_grad[0] else None
        gw = gemm_raw(gy, x, True, False) if ctx.needs_input_grad[1] else None
        gb = colsum(gy) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return _fresh(gx, ctx.tap_box), gw, gb, (gy if ctx.needs_input_grad[3] else None)


def linear_add(x: Tensor, weight: Tensor, bias: Tensor | None, addend: Tensor) -> Tensor:
    """F.linear(x, weight, bias) + addend, one store."""
    _lib.require_gpu(x)
    if x.shape[0] == 0:
        return torch.nn.functional.linear(x, weight, bias) + addend
    return _LinearAdd.apply(x, weight, bias, addend)


def sage_layer(x: Tensor, adj, lin_l, lin_r, reduce: str, narrow: bool) -> Tensor:
    return _SageLayer.apply(x, adj, lin_l.weight, lin_l.bias, lin_r.weight, reduce, narrow)


class _TapBox:
    """Row-compact gradient pieces of one tapped tensor, waiting for its ``_GradTap.backward``."""
    __slots__ = ("pending",)

    def __init__(self):
        self.pending = []


class _GradTap(torch.autograd.Function):
    """Identity with a side door for row-compact gradients.  The student's last hidden state h feeds the next conv AND
    ``student_proj(h[train_idx])`` (gnn.py:150-156); autograd would add the two gradients as dense [N,C] tensors (zero
    fill + scatter of the projection's rows + a full-size add: ~160 us at N = 169 343).  Consumers that only touch some
    rows (``linear_rows``) leave (ids, rows) in the box and return NO gradient for the tapped tensor -- the graph edge
    still orders them before this node -- and the rows are added into the dense gradient of the other consumer here."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box, ctx.meta = box, (x.shape, x.dtype, x.device)
        ctx.set_materialize_grads(False)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        pend, ctx.box.pending = ctx.box.pending, []
        if not pend:
            return g, None
        if g is None:
            shape, dtype, dev = ctx.meta
            g = torch.zeros(shape, dtype=dtype, device=dev)
        elif g.is_sparse or not g.is_contiguous():
            g = g.to_dense().contiguous() if g.is_sparse else g.contiguous()
        elif getattr(g, "_egnn_fresh_for", None) is not ctx.box:
            # autograd forbids changing a grad_output in place: a consumer whose backward hands its own grad_output through
            # (add, a view, identity) or a caller-supplied gradient would be corrupted.  Only a tensor one of this package's
            # backward functions has just allocated FOR THIS tapped tensor (``_fresh`` names the box) is added into directly.
            g = g.clone()
        for idx, rows in pend:   # unique ids: a plain read-modify-write of those rows; a RowsPlan: its run-sum; both deterministic
            _tap_rows_add(g, idx, rows)
        return g, None


_SPLIT_IDS = _cache.TensorKeyedCache(capacity=16)


def split_ids(split_idx: dict, n: int, device) -> Tensor:
    """int8 [n]: 0 / 1 / 2 for the train / valid / test nodes of ``split_idx``, -1 elsewhere (a node listed twice keeps the
    later split); built once per split dict (keyed on the identity and version of its index tensors, which the entry keeps alive)."""
    names = ("train", "valid", "test")

    def build():
        sid = torch.full((n,), -1, dtype=torch.int8, device=device)
        for i, k in enumerate(names):
            sid[split_idx[k].to(device)] = i
        return sid
    return _SPLIT_IDS.get(tuple(split_idx[k] for k in names), (n, str(device)), build)


def split_accuracy(logits: Tensor, y: Tensor, split_idx: dict, counts: bool = False, out: Tensor | None = None) -> Tensor:
    """float64 [3]: the Evaluator accuracies of test() (gnn.py:198-218) for train / valid / test in one pass over the
    logits (egnn_split_accuracy_f32: first-max argmax, integer hit counts over split sizes).
    ``counts``: float64 [6] = (hits of the three splits, sizes of the three splits) instead of the ratios (a shard's contribution
    to the all-rank accuracies)."""
    _lib.require_gpu(logits, y)
    logits = _rowmajor(logits)
    n, C = logits.shape
    yv = y.reshape(-1)
    if yv.dtype != torch.int64 or yv.numel() != n:
        raise TypeError("split_accuracy: labels must be int64 [n] or [n,1]")
    if n == 0:
        return torch.zeros(6, dtype=torch.float64, device=logits.device) if counts else torch.full((3,), float("nan"), dtype=torch.float64, device=logits.device)
    yv = yv.contiguous()
    sid = split_ids(split_idx, n, logits.device)
    lib = _lib.load()
    nws = lib.egnn_split_accuracy_ws_ints()
    ws = torch.empty(nws, dtype=torch.int32, device=logits.device)
    acc = out if out is not None else torch.empty(6 if counts else 3, dtype=torch.float64, device=logits.device)
    if acc.dtype != torch.float64 or acc.numel() != (6 if counts else 3) or not acc.is_contiguous() or acc.device != logits.device:
        raise TypeError("split_accuracy: `out` must be a contiguous float64 tensor of 3 (6 with counts) elements on the logits' device")
    fn, name = (lib.egnn_split_counts_f32, "egnn_split_counts_f32") if counts else (lib.egnn_split_accuracy_f32, "egnn_split_accuracy_f32")
    _lib.check(fn(_lib.ptr(logits), logits.stride(0), n, C, _lib.ptr(yv), _lib.ptr(sid), _lib.ptr(acc), _lib.ptr(ws), nws, _lib.stream()), name)
    return acc


def grad_tap(x: Tensor) -> Tensor:
    """``x`` again, marked so that ``linear_rows(x, idx, ...)`` hands its input gradient over in row-compact form."""
    if not (torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.dim() == 2):
        return x
    box = _TapBox()
    y = _GradTap.apply(x, box)
    y._egnn_tap = box
    return y


_CONST_PLANES = _cache.TensorKeyedCache(capacity=4, max_bytes=2 << 30)    # plane images of constant operands: at most 2 GiB of the 288


def _dw_const_rows(gy: Tensor, x: Tensor, idx: Tensor):
    """dW = gy^T x[idx] for a CONSTANT x (the teacher's features under the teacher projection head, gnn.py:155,303-306): x[idx] is cut
    once per (x, idx) identity + version into bf16 planes with the row position as the reduction index (egnn_gemm_tn_planes_pack_f32,
    6 bytes per element: 419 MB for [90 941, 750], kept as long as the cache entry lives); the per-step product then takes the
    transposed-operand x planes form of the DMA pipeline (egnn_gemm_tn_planes_f32).  None = shape not taken (the caller's generic
    gather-fused GEMM)."""
    K, M = gy.shape
    N = x.shape[1]
    if not (M % 256 == 0 and K >= 16384 and gy.stride(0) % 4 == 0 and gy.data_ptr() % 16 == 0 and x.stride(1) == 1 and idx.numel() == K):
        return None
    lib = _lib.load()

    def build():
        nbytes = lib.egnn_gemm_tn_planes_bytes(N, K)
        planes = _aligned_bytes(nbytes, x.device)
        _lib.check(lib.egnn_gemm_tn_planes_pack_f32(_lib.ptr(x), x.stride(0), _lib.ptr(idx), N, K, _lib.ptr(planes), nbytes, _lib.stream()),
                   "egnn_gemm_tn_planes_pack_f32")
        return planes
    planes = _CONST_PLANES.get((x, idx), (), build)
    gw = torch.empty(M, N, dtype=torch.float32, device=gy.device)
    nws = lib.egnn_gemm_tn_planes_ws_floats(M, N, K)
    ws = torch.empty(nws, dtype=torch.float32, device=gy.device)
    rc = lib.egnn_gemm_tn_planes_f32(M, N, K, 1.0, _lib.ptr(gy), gy.stride(0), _lib.ptr(planes), _lib.ptr(gw), gw.stride(0), _lib.ptr(ws), nws,
                                     _lib.stream())
    if rc == _lib.EGNN_EALIGN:
        return None
    _lib.check(rc, "egnn_gemm_tn_planes_f32")
    return gw


_CONST_ROW_PLANES = _cache.TensorKeyedCache(capacity=4, max_bytes=2 << 30)


def _aligned_bytes(nbytes: int, device) -> Tensor:
    """uint8 [nbytes] starting on a 1 KB boundary (the DMA pipeline copies plane tiles in 1 KB pieces)."""
    buf = torch.empty(nbytes + 1024, dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % 1024
    return buf[off:off + nbytes]


def _fwd_const_rows(x: Tensor, idx: Tensor, w: Tensor, bias: Tensor | None):
    """y = x[idx] @ w^T + bias for a CONSTANT x (see ``_dw_const_rows``): the gathered rows live as tile-packed bf16 planes, cut once
    per (x, idx); w is cut per call (egnn_gemm_rows_planes_f32: planes x planes on the DMA pipeline).  None = shape not taken."""
    M, K = idx.numel(), x.shape[1]
    N = w.shape[0]
    if not (N % 128 == 0 and M >= 16384 and x.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K):
        return None
    lib = _lib.load()

    def build():
        nbytes = lib.egnn_gemm_rows_planes_bytes(M, K)
        planes = _aligned_bytes(nbytes, x.device)
        _lib.check(lib.egnn_gemm_rows_planes_pack_f32(_lib.ptr(x), x.stride(0), _lib.ptr(idx), M, K, _lib.ptr(planes), nbytes, _lib.stream()),
                   "egnn_gemm_rows_planes_pack_f32")
        return planes
    planes = _CONST_ROW_PLANES.get((x, idx), (), build)
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    nws = lib.egnn_gemm_rows_planes_ws_bytes(N, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    rc = lib.egnn_gemm_rows_planes_f32(M, N, K, 1.0, _lib.ptr(planes), _lib.ptr(w), w.stride(0), _lib.ptr(bias), _lib.ptr(y), y.stride(0),
                                       _lib.ptr(ws), nws, _lib.stream())
    if rc == _lib.EGNN_EALIGN:
        return None
    _lib.check(rc, "egnn_gemm_rows_planes_f32")
    return y


class _LinearRows(torch.autograd.Function):
    """y = x[idx] @ weight^T + bias for UNIQUE row ids, without materialising x[idx] (egnn_gemm_rows_f32): the forward
    gathers in the A-operand load, dW = dY^T x[idx] in the B-operand load, dx scatters the rows of dY W (or leaves
    them with the tap of a ``grad_tap`` tensor)."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, box, const_input=False, plan=None):
        w = pad_pitch(weight) if not _pitch_ok(weight) else weight   # 0.8 MB at 256 x 750: rows 16-byte aligned
        ctx.save_for_backward(x, idx, w)
        ctx.has_bias, ctx.box, ctx.plan = bias is not None, box, plan   # plan: the ids repeat rows (duplicates="sum"), dx is a run-sum
        # a CONSTANT input (the caller says so: the teacher's features, gnn.py:155): its gathered rows as planes, cut once per (x, idx)
        ctx.const_input = bool(const_input) and not x.requires_grad
        y = _fwd_const_rows(x, idx, w, bias) if ctx.const_input else None
        return y if y is not None else gemm_raw(x, w, False, True, bias, a_rows=idx)

    @staticmethod
    def backward(ctx, gy):
        x, idx, w = ctx.saved_tensors
        gy = _rowmajor(gy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            rows = gemm_raw(gy, w, False, False)
            if ctx.box is not None:
                ctx.box.pending.append((idx if ctx.plan is None else ctx.plan, rows))
            elif ctx.plan is not None:
                gx = torch.empty(x.shape, dtype=gy.dtype, device=gy.device)
                _rows_add_runs(gx, ctx.plan, rows, False)
            else:
                gx = torch.zeros(x.shape, dtype=gy.dtype, device=gy.device)
                gx.index_copy_(0, idx, rows)
        if ctx.needs_input_grad[2]:
            gw = _dw_const_rows(gy, x, idx) if ctx.const_input else None
            if gw is None:
                gw = gemm_raw(gy, x, True, False, b_rows=idx)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = colsum(gy)
        return gx, None, gw, gb, None, None, None


def linear_rows(x: Tensor, idx: Tensor, weight: Tensor, bias: Tensor | None = None, const_input: bool = False,
                duplicates: str = "unique") -> Tensor:
    """``F.linear(x[idx], weight, bias)`` with the row gather fused into the GEMM (unique ``idx``; ``duplicates="sum"``: any ``idx``,
    by torch's rules, see ``take_rows`` -- the forward and dW read a row as often as it is named, dx becomes a run-sum).
    ``const_input=True`` (opt-in; the teacher projection head): ``x`` does not change between calls -- its gathered rows are re-laid
    ONCE per (x, idx) identity + version as tile-packed bf16 planes (6 bytes per element, held by a byte-bounded cache) and the forward /
    weight-gradient products run on the planes x planes forms.  Without the flag no plane image is ever built: activations under
    ``no_grad`` (requires_grad False as well) or RGCN's per-node-type calls take the gather-fused GEMM."""
    summing = isinstance(idx, RowsPlan) or _check_duplicates(duplicates)   # (a ready plan in place of the ids: nothing is built)
    _lib.require_gpu(x)
    plan = None
    if summing:
        plan = _plan_for(idx, x.shape[0], "linear_rows")
        idx, plan = plan.idx, plan if plan.keys is not None else None
    return _LinearRows.apply(x, idx, weight, bias, getattr(x, "_egnn_tap", None) if torch.is_grad_enabled() else None, const_input, plan)


def linear(x: Tensor, weight: Tensor, bias: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """x @ weight^T + bias with ``weight`` in nn.Linear layout [out, in]; ``out``: see ``gemm_raw`` (forward-only)."""
    if out is not None:
        return _matmul_into(x, weight, bias, True, out)
    return _MatMul.apply(x, weight, bias, True)


# ------------------------------------------------------------------------------------------------
# cross entropy (+ logit KD)
# ------------------------------------------------------------------------------------------------
class _CeKd(torch.autograd.Function):
    """(mean CE, mean KD) of the rows ``rows`` (None: all) of logits / teacher with labels[rows] (fused row gathers)."""

    @staticmethod
    def forward(ctx, logits, labels, teacher, T, rows=None):
        _lib.require_gpu(logits, labels, teacher, rows)
        logits = _rowmajor(logits)
        teacher = None if teacher is None else _rowmajor(teacher)
        # the kernels index with the labels: PyTorch's own checks (class-index targets are int64 [n]) are kept on the host;
        # out-of-range values (incl. ignore_index = -100) are ignored inside the kernel, never used as an address
        if labels.dtype != torch.int64:
            raise TypeError(f"cross_entropy: expected int64 class-index labels, got {labels.dtype} "
                            "(multi-label float targets are the PPI path: criterion.ppi_kd_criterion)")
        if labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
            raise ValueError(f"cross_entropy: labels must have shape ({logits.shape[0]},), got {tuple(labels.shape)}")
        if teacher is not None and teacher.shape != logits.shape:
            raise ValueError(f"kd: teacher logits {tuple(teacher.shape)} do not match the student's {tuple(logits.shape)}")
        labels = labels.contiguous()
        if rows is not None:
            if rows.dtype != torch.int64 or rows.dim() != 1:
                raise TypeError("cross_entropy: `rows` must be a 1-D int64 index tensor")
            rows = rows.contiguous()
        n = logits.shape[0] if rows is None else rows.numel()
        C = logits.shape[1]
        lib = _lib.load()
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        ws = torch.empty(lib.egnn_ce_kd_ws_floats(n), dtype=torch.float32, device=logits.device)
        rc = lib.egnn_ce_kd_fwd_f32(_lib.ptr(logits), logits.stride(0), _lib.ptr(teacher), 0 if teacher is None else teacher.stride(0),
                                    _lib.ptr(labels), _lib.ptr(rows), n, C, float(T), _lib.ptr(out), _lib.ptr(ws), _lib.stream())
        _lib.check(rc, "egnn_ce_kd_fwd_f32")
        ctx.save_for_backward(logits, labels, out, *([] if teacher is None else [teacher]), *([] if rows is None else [rows]))
        ctx.T, ctx.has_teacher, ctx.has_rows, ctx.n = float(T), teacher is not None, rows is not None, n
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cls, g_kd):
        saved = list(ctx.saved_tensors)
        logits, labels, out = saved[:3]
        rest = saved[3:]
        teacher = rest.pop(0) if ctx.has_teacher else None
        rows = rest.pop(0) if ctx.has_rows else None
        n_total, C = logits.shape
        dl = torch.empty_like(logits)
        g_cls = None if g_cls is None else g_cls.contiguous().to(torch.float32)
        g_kd = None if g_kd is None else g_kd.contiguous().to(torch.float32)
        rc = _lib.load().egnn_ce_kd_bwd_f32(_lib.ptr(logits), logits.stride(0), _lib.ptr(teacher),
                                            0 if teacher is None else teacher.stride(0), _lib.ptr(labels), _lib.ptr(rows), n_total, ctx.n,
                                            C, ctx.T, _lib.ptr(out), _lib.ptr(g_cls), _lib.ptr(g_kd), _lib.ptr(dl), dl.stride(0), _lib.stream())
        _lib.check(rc, "egnn_ce_kd_bwd_f32")
        return dl, None, None, None, None


def cross_entropy(logits: Tensor, labels: Tensor, rows: Tensor | None = None) -> Tensor:
    """mean CE (F.cross_entropy) on the fused kernel; ``rows``: evaluate logits[rows] against labels[rows] without the copies."""
    return _CeKd.apply(logits, labels, None, 1.0, rows)[0]


def ce_and_kd(logits: Tensor, labels: Tensor, teacher_logits: Tensor, T: float, rows: Tensor | None = None):
    """(mean CE, F.kl_div(log_softmax(logits/T), softmax(teacher/T)) with reduction='mean'); ``rows`` as in cross_entropy."""
    return _CeKd.apply(logits, labels, teacher_logits, T, rows)


# ------------------------------------------------------------------------------------------------
# gather + L2 normalise
# ------------------------------------------------------------------------------------------------
class _GatherNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, eps, plan=None):
        _lib.require_gpu(x, idx)
        x = _rowmajor(x)
        ctx.plan = plan
        n = x.shape[0] if idx is None else idx.numel()
        D = x.shape[1]
        out = torch.empty(n, D, dtype=torch.float32, device=x.device)
        inv = torch.empty(n, dtype=torch.float32, device=x.device)
        rc = _lib.load().egnn_gather_normalize_rows_f32(_lib.ptr(x), x.stride(0), _lib.ptr(idx), n, D, float(eps), _lib.ptr(out),
                                                        out.stride(0), _lib.ptr(inv), _lib.stream())
        _lib.check(rc, "egnn_gather_normalize_rows_f32")
        ctx.save_for_backward(out, inv, *([] if idx is None else [idx]))
        ctx.eps, ctx.n_in = float(eps), x.shape[0]
        return out

    @staticmethod
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        out, inv = saved[0], saved[1]
        idx = saved[2] if len(saved) > 2 else None
        gout = _rowmajor(gout)
        n, D = out.shape
        if ctx.plan is not None:     # ids that repeat rows: the row-compact gradients (idx == NULL form), then their run-sum into dx
            idx = None
        dx = torch.zeros(ctx.n_in, D, dtype=torch.float32, device=out.device) if idx is not None else torch.empty_like(out)
        rc = _lib.load().egnn_normalize_rows_bwd_f32(_lib.ptr(out), out.stride(0), _lib.ptr(gout), gout.stride(0), _lib.ptr(inv),
                                                     _lib.ptr(idx), n, D, ctx.eps, _lib.ptr(dx), dx.stride(0), 0, _lib.stream())
        _lib.check(rc, "egnn_normalize_rows_bwd_f32")
        if ctx.plan is not None:
            rows, dx = dx, torch.empty(ctx.n_in, D, dtype=torch.float32, device=out.device)
            _rows_add_runs(dx, ctx.plan, rows, False)
        return dx, None, None, None


def gather_normalize(x: Tensor, idx: Tensor | None = None, eps: float = 1e-12, duplicates: str = "unique") -> Tensor:
    """F.normalize(x[idx], p=2, dim=-1) fused (rows of ``idx`` must be unique, as np.random.choice(replace=False) gives;
    ``duplicates="sum"``: any ``idx`` by torch's rules, see ``take_rows``)."""
    if not _check_duplicates(duplicates) or idx is None:
        return _GatherNormalize.apply(x, idx, eps)
    plan = rows_plan(idx, x.shape[0])
    return _GatherNormalize.apply(x, plan.idx, eps, plan if plan.dups else None)


# ------------------------------------------------------------------------------------------------
# FitNet / attention-transfer losses (criterion.py:24-54) as row kernels
# ------------------------------------------------------------------------------------------------
class _FeatureLoss(torch.autograd.Function):
    """kind 'fitnet': mse(F.normalize(f), F.normalize(t));  kind 'at': mse of the per-node energies normalised ACROSS nodes."""

    @staticmethod
    def forward(ctx, f, t, kind, eps):
        _lib.require_gpu(f, t)
        f, t = _rowmajor(f), _rowmajor(t)
        if f.dim() != 2 or t.dim() != 2 or f.shape[0] != t.shape[0] or (kind == "fitnet" and f.shape[1] != t.shape[1]):
            raise ValueError(f"{kind}: student features {tuple(f.shape)} and teacher features {tuple(t.shape)} do not match")
        n = f.shape[0]
        lib, dev = _lib.load(), f.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = lib.egnn_feature_loss_ws_floats(n)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        if kind == "fitnet":
            rc = lib.egnn_fitnet_fwd_f32(_lib.ptr(f), f.stride(0), _lib.ptr(t), t.stride(0), n, f.shape[1], float(eps), _lib.ptr(loss),
                                         _lib.ptr(ws), nws, _lib.stream())
        else:
            rc = lib.egnn_at_fwd_f32(_lib.ptr(f), f.stride(0), f.shape[1], _lib.ptr(t), t.stride(0), t.shape[1], n, float(eps), _lib.ptr(loss),
                                     _lib.ptr(ws), nws, _lib.stream())
        _lib.check(rc, f"egnn_{kind}_fwd_f32")
        ctx.save_for_backward(f, t, ws)
        ctx.kind, ctx.eps = kind, float(eps)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        f, t, ws = ctx.saved_tensors
        n = f.shape[0]
        g = g.contiguous().to(torch.float32).reshape(1)
        df = torch.empty_like(f) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        lib = _lib.load()
        if ctx.kind == "fitnet":
            rc = lib.egnn_fitnet_bwd_f32(_lib.ptr(f), f.stride(0), _lib.ptr(t), t.stride(0), n, f.shape[1], ctx.eps, _lib.ptr(g),
                                         _lib.ptr(df), 0 if df is None else df.stride(0), _lib.ptr(dt), 0 if dt is None else dt.stride(0),
                                         _lib.stream())
        else:
            rc = lib.egnn_at_bwd_f32(_lib.ptr(f), f.stride(0), f.shape[1], _lib.ptr(t), t.stride(0), t.shape[1], n, ctx.eps, _lib.ptr(ws),
                                     _lib.ptr(g), _lib.ptr(df), 0 if df is None else df.stride(0), _lib.ptr(dt),
                                     0 if dt is None else dt.stride(0), _lib.stream())
        _lib.check(rc, f"egnn_{ctx.kind}_bwd_f32")
        return df, dt, None, None


def fitnet_loss(feat: Tensor, teacher_feat: Tensor, eps: float = 1e-12) -> Tensor:
    """F.mse_loss(F.normalize(feat), F.normalize(teacher_feat)) in one pass per direction (egnn_fitnet_*_f32)."""
    return _FeatureLoss.apply(feat, teacher_feat, "fitnet", eps)


def at_loss(feat: Tensor, teacher_feat: Tensor, eps: float = 1e-12) -> Tensor:
    """criterion.py:44-50: per-node energies sum_d x^2, each length-n vector L2-normalised across the nodes, then mse."""
    return _FeatureLoss.apply(feat, teacher_feat, "at", eps)


# The same loss on node-range shards (dist._DistAT): three steps with the ranks' two all-reduces in between.  No autograd here -- the
# caller's Function owns the graph.  A rank without rows launches nothing: empty energies, zero sums.
def at_energy(f: Tensor, t: Tensor):
    """(es [n], et [n], sumsq [2]): the row energies sum_d f^2 / sum_d t^2 of this rank's rows and {sum es^2, sum et^2} over them."""
    _lib.require_gpu(f, t)
    f, t = _rowmajor(f), _rowmajor(t)
    if f.dim() != 2 or t.dim() != 2 or f.shape[0] != t.shape[0]:
        raise ValueError(f"at: student features {tuple(f.shape)} and teacher features {tuple(t.shape)} do not match")
    n, dev = f.shape[0], f.device
    if n == 0:
        return f.new_empty(0), f.new_empty(0), torch.zeros(2, dtype=torch.float32, device=dev)
    lib = _lib.load()
    es, et = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    sumsq = torch.empty(2, dtype=torch.float32, device=dev)
    nws = lib.egnn_feature_loss_ws_floats(n)
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    _lib.check(lib.egnn_at_energy_f32(_lib.ptr(f), f.stride(0), f.shape[1], _lib.ptr(t), t.stride(0), t.shape[1], n, _lib.ptr(es), _lib.ptr(et),
                                      _lib.ptr(sumsq), _lib.ptr(ws), nws, _lib.stream()), "egnn_at_energy_f32")
    return es, et, sumsq


def at_partial(es: Tensor, et: Tensor, sumsq_global: Tensor, eps: float = 1e-12):
    """(scal [4] = {ns, nt, raw |e_s|, raw |e_t|}, sums [3] = {sum d^2, sum d es, sum d et} over this rank's rows) for
    d = es / ns - et / nt under the all-rank norms ns = max(sqrt(sumsq_global[0]), eps), nt likewise."""
    _lib.require_gpu(es, et, sumsq_global)
    n, dev = es.shape[0], sumsq_global.device
    sums = torch.empty(3, dtype=torch.float32, device=dev)
    scal = torch.empty(4, dtype=torch.float32, device=dev)
    if n == 0:                         # nothing reads scal on a rank without rows
        return scal, sums.zero_()
    lib = _lib.load()
    nws = lib.egnn_feature_loss_ws_floats(n)
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    _lib.check(lib.egnn_at_partial_f32(_lib.ptr(es), _lib.ptr(et), n, _lib.ptr(sumsq_global), float(eps), _lib.ptr(scal), _lib.ptr(sums),
                                       _lib.ptr(ws), nws, _lib.stream()), "egnn_at_partial_f32")
    return scal, sums


def at_rows_bwd(f: Tensor, t: Tensor, n_global: int, es: Tensor, et: Tensor, scal: Tensor, sums_global: Tensor, g: Tensor,
                eps: float = 1e-12, need_df: bool = True, need_dt: bool = True):
    """(df, dt) of this rank's rows for loss = sums_global[0] / n_global and the upstream gradient ``g``; None where not needed."""
    _lib.require_gpu(f, t)
    f, t = _rowmajor(f), _rowmajor(t)
    n = f.shape[0]
    df = torch.empty_like(f) if need_df else None
    dt = torch.empty_like(t) if need_dt else None
    if n == 0:
        return df, dt
    g = g.contiguous().to(torch.float32).reshape(1)
    _lib.check(_lib.load().egnn_at_bwd_rows_f32(_lib.ptr(f), f.stride(0), f.shape[1], _lib.ptr(t), t.stride(0), t.shape[1], n, int(n_global),
                                                _lib.ptr(es), _lib.ptr(et), _lib.ptr(scal), _lib.ptr(sums_global), float(eps), _lib.ptr(g),
                                                _lib.ptr(df), 0 if df is None else df.stride(0), _lib.ptr(dt),
                                                0 if dt is None else dt.stride(0), _lib.stream()), "egnn_at_bwd_rows_f32")
    return df, dt


# ------------------------------------------------------------------------------------------------
# G-CRD / InfoNCE on unit rows
# ------------------------------------------------------------------------------------------------
class _NCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fhat, that, tau):
        _lib.require_gpu(fhat, that)
        fhat, that = fhat.contiguous(), that.contiguous()
        S, P = fhat.shape
        if that.shape != fhat.shape:
            raise ValueError("nce: student and teacher features must have the same shape")
        lib = _lib.load()
        dev = fhat.device
        Z = torch.empty(S, S, dtype=torch.float32, device=dev)
        lse = torch.empty(S, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = lib.egnn_nce_ws_floats(S)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        rc = lib.egnn_nce_fwd_f32(_lib.ptr(fhat), _lib.ptr(that), S, P, fhat.stride(0), float(tau), 1, _lib.ptr(Z), _lib.ptr(lse),
                                  _lib.ptr(loss), _lib.ptr(ws), nws, _lib.stream())
        _lib.check(rc, "egnn_nce_fwd_f32")
        ctx.save_for_backward(fhat, that, Z, lse)
        ctx.tau = float(tau)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        fhat, that, Z, lse = ctx.saved_tensors
        S, P = fhat.shape
        g = g.contiguous().to(torch.float32)
        df = torch.empty_like(fhat) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(that) if ctx.needs_input_grad[1] else None
        lib = _lib.load()
        nws = lib.egnn_nce_bwd_ws_floats(S, S, P)
        ws = torch.empty(nws, dtype=torch.float32, device=fhat.device)
        rc = lib.egnn_nce_bwd_f32(_lib.ptr(fhat), _lib.ptr(that), S, P, fhat.stride(0), ctx.tau, 1, _lib.ptr(Z), _lib.ptr(lse),
                                  _lib.ptr(g), _lib.ptr(df), _lib.ptr(dt), _lib.ptr(ws), nws, _lib.stream())
        _lib.check(rc, "egnn_nce_bwd_f32")
        return df, dt, None


def nce_unit(fhat: Tensor, that: Tensor, tau: float) -> Tensor:
    """mean_i(logsumexp_j(fhat_i . that_j / tau) - fhat_i . that_i / tau) for unit-norm rows."""
    return _NCE.apply(fhat, that, tau)


def nce_block_fwd(fhat: Tensor, t_all: Tensor, diag_off: int, tau: float, inv_count: float, unit_rows: bool = True):
    """Row block of the G-CRD loss (egnn_nce_block_fwd_f32): returns (Z [Sr,Sc], lse [Sr], loss_sum*inv_count [1]).
    Z is the saved score matrix for nce_block_bwd: logits, or exp(logit - 1.0001/tau) in the unit-rows form
    (egnn_nce_saves_exp); pass the same tau / unit_rows to the backward."""
    _lib.require_gpu(fhat, t_all)
    Sr, P = fhat.shape
    Sc = t_all.shape[0]
    lib, dev = _lib.load(), fhat.device
    Z = torch.empty(Sr, Sc, dtype=torch.float32, device=dev)
    lse = torch.empty(Sr, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    nws = lib.egnn_nce_ws_floats(Sr)
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    rc = lib.egnn_nce_block_fwd_f32(_lib.ptr(fhat), fhat.stride(0), _lib.ptr(t_all), t_all.stride(0), Sr, Sc, diag_off, P, float(tau),
                                    float(inv_count), int(unit_rows), _lib.ptr(Z), _lib.ptr(lse), _lib.ptr(loss), _lib.ptr(ws), nws, _lib.stream())
    _lib.check(rc, "egnn_nce_block_fwd_f32")
    return Z, lse, loss


def nce_block_bwd(fhat: Tensor, t_all: Tensor, diag_off: int, scale: float, Z: Tensor, lse: Tensor, g: Tensor, tau: float,
                  unit_rows: bool = True):
    """(dfhat [Sr,P], this rank's contribution to dthat_all [Sc,P]) via egnn_nce_block_bwd_f32."""
    Sr, P = fhat.shape
    Sc = t_all.shape[0]
    df, dt = torch.empty_like(fhat), torch.empty_like(t_all)
    nws = _lib.load().egnn_nce_bwd_ws_floats(Sr, Sc, P)
    ws = torch.empty(nws, dtype=torch.float32, device=fhat.device)
    rc = _lib.load().egnn_nce_block_bwd_f32(_lib.ptr(fhat), fhat.stride(0), _lib.ptr(t_all), t_all.stride(0), Sr, Sc, diag_off, P,
                                            float(tau), float(scale), int(unit_rows), _lib.ptr(Z), _lib.ptr(lse), _lib.ptr(g), _lib.ptr(df), df.stride(0),
                                            _lib.ptr(dt), dt.stride(0), _lib.ptr(ws), nws, _lib.stream())
    _lib.check(rc, "egnn_nce_block_bwd_f32")
    return df, dt


# ------------------------------------------------------------------------------------------------
# fused BatchNorm1d (+ ReLU + dropout)
# ------------------------------------------------------------------------------------------------
# Optional per-step dropout seed kept ON THE DEVICE (int64 [1]): the kernels add it to the per-call host seed.  A captured
# hipGraph of the train step (models.GraphedEpoch) refreshes it before every replay, so that replays draw fresh masks.
_DROPOUT_SEED_DEV: Tensor | None = None


def _draw_dropout_seed() -> int:
    """The per-call 63-bit seed of a fused dropout mask, from torch's HOST generator (``torch.manual_seed`` reproducible).  The mask of
    element (r, c) is a counter hash of (seed [+ the device-side per-step seed], r * C + c): csrc/bn_common.h.  One function so that
    the training-parity harness (oracle/training_parity.py) can record the seeds and rebuild the masks for the oracle."""
    return int(torch.empty((), dtype=torch.int64).random_()) & 0x7FFFFFFFFFFFFFFF


def _bn_shape_ok(x: Tensor) -> bool:
    C = x.shape[1]
    return x.is_cuda and C % 4 == 0 and C <= 1024 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0


# an empty ``pick`` (a shard without sampled rows) may have no storage; the C side still needs a non-NULL pick to take the picked-rows
# form and reads no entry of it (n_pick = 0)
_NO_PICKED_ROW = ctypes.c_int64(-1)


def _bn_desc(x, gamma, beta, mean, var, eps, relu, p, seed, seed_dev, pick=None) -> ctypes.Structure:
    """The egnn_bn_act_t descriptor (include/egnn_hip.h) of one fused BatchNorm call over the rows of ``x``: every row, or the output
    rows ``pick``.  Built per call from the tensors at hand; the entry points read it only while they run."""
    n, C = x.shape
    pick_ptr = None if pick is None else (pick.data_ptr() or ctypes.addressof(_NO_PICKED_ROW))
    return _lib.BnAct(_lib.ptr(x), x.stride(0), n, C, _lib.ptr(mean), _lib.ptr(var), float(eps), _lib.ptr(gamma), _lib.ptr(beta),
                      int(relu), float(p), int(seed), _lib.ptr(seed_dev), pick_ptr, 0 if pick is None else pick.numel())


def _sync_sums(sums: Tensor, sync) -> Tensor:
    """[sum d | sum d*xhat] of ALL ranks divided by their row total: ONE all-reduce, scaled on the device (no host read of the count)."""
    import torch.distributed as dist
    total, group = sync
    if dist.get_world_size(group) > 1:
        sums = sums.clone()
        dist.all_reduce(sums, group=group)
    return sums / total


def _bn_act_fwd(x, gamma, beta, mean, var, eps, relu, p, seed, seed_dev, pick=None) -> Tensor:
    """y = drop(relu(bn(x))) with the given statistics: every row, or only the rows ``pick``.  An empty result (a shard without rows,
    an empty ``pick``) launches nothing."""
    n, C = x.shape
    y = torch.empty(n if pick is None else pick.numel(), C, dtype=torch.float32, device=x.device)
    if y.shape[0] == 0:
        return y
    bn = _bn_desc(x, gamma, beta, mean, var, eps, relu, p, seed, seed_dev, pick)
    _lib.check(_lib.load().egnn_bn_act_fwd_f32(ctypes.byref(bn), _lib.ptr(y), y.stride(0), _lib.stream()), "egnn_bn_act_fwd_f32")
    return y


class _BnAct(torch.autograd.Function):
    """y = drop(relu(bn(x))) with the statistics (mean, var) taken by the caller.  ``pick`` (int64 [S], unique row ids) = form only the
    output rows ``pick``: y[i] = act(bn(x[pick[i]])) -- the statistics still span all rows of x, and so does dx.
    ``sync`` = None: statistics of this tensor alone.  ``sync`` = (total rows [1] on the device, group): statistics of the rows of ALL
    ranks (``_sync_stats``; node-range shards, where ``pick`` may hold no row of this shard) -- the backward all-reduces
    [sum d, sum d*xhat] between its reduce half and its apply half; the parameter gradients stay this shard's local sums."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, var, eps, relu, p, seed, batch_stats, pick=None, sync=None):
        if not x.is_cuda:    # (the kernels take device pointers: a host tensor must never reach a launch)
            raise RuntimeError(f"bn_act: the HIP kernels need a GPU tensor, got one on {x.device}")
        x = _rowmajor(x)
        n = x.shape[0]
        if pick is not None and (pick.dtype != torch.int64 or pick.dim() != 1 or not pick.is_contiguous() or pick.numel() > n
                                 or (sync is None and pick.numel() == 0)):
            raise ValueError("bn_act: `pick` must be a non-empty contiguous 1-D int64 tensor of unique row ids" if sync is None else
                             "sync_bn_act: `pick` must be a contiguous 1-D int64 tensor of unique row ids")
        seed_dev = _DROPOUT_SEED_DEV if p > 0 else None     # the per-step seed of a replayed graph (fresh masks in every replay)
        y = _bn_act_fwd(x, gamma, beta, mean, var, eps, relu, p, seed, seed_dev, pick)
        ctx.save_for_backward(x, gamma, beta, mean, var, *([] if pick is None else [pick]))
        ctx.cfg = (float(eps), int(relu), float(p), int(seed), int(batch_stats))
        ctx.seed_dev, ctx.sync = seed_dev, sync
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, var = ctx.saved_tensors[:5]
        pick = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        eps, relu, p, seed, batch_stats = ctx.cfg
        gy = _rowmajor(gy)
        n, C = x.shape
        lib, dev = _lib.load(), x.device
        bn = ctypes.byref(_bn_desc(x, gamma, beta, mean, var, eps, relu, p, seed, ctx.seed_dev, pick))
        sums = torch.empty(2 * C, dtype=torch.float32, device=dev)   # [dbeta | dgamma] of this tensor
        dx = torch.empty_like(x)
        nws = lib.egnn_bn_ws_floats(C)
        ws = torch.empty(nws, dtype=torch.float32, device=dev) if n > 0 else None
        # the producer of x usually added a bias (GCNConv / nn.Linear in front of the BatchNorm): its gradient is the column sum of dx,
        # formed in the same pass (ops.colsum picks the tag up)
        cs = torch.empty(C, dtype=torch.float32, device=dev) if (batch_stats and n > 0) else None
        if ctx.sync is None:
            # statistics of this tensor alone: one call, no collective between its halves
            _lib.check(lib.egnn_bn_act_bwd_f32(bn, _lib.ptr(gy), gy.stride(0), batch_stats, _lib.ptr(sums[C:]), _lib.ptr(sums), _lib.ptr(dx),
                                               dx.stride(0), _lib.ptr(cs), _lib.ptr(ws), nws, _lib.stream()), "egnn_bn_act_bwd_f32")
        else:
            # all ranks: reduce half, ONE all-reduce of [sum d | sum d*xhat], apply half; the parameter grads stay local (the flat
            # all-reduce sums them)
            if (n if pick is None else pick.numel()) > 0:          # rows that carry a gradient
                _lib.check(lib.egnn_bn_act_bwd_reduce_f32(bn, _lib.ptr(gy), gy.stride(0), _lib.ptr(sums[C:]), _lib.ptr(sums), _lib.ptr(ws),
                                                          nws, _lib.stream()), "egnn_bn_act_bwd_reduce_f32")
            else:
                sums.zero_()
            scaled = _sync_sums(sums, ctx.sync)
            if n > 0:
                _lib.check(lib.egnn_bn_act_bwd_apply_f32(bn, _lib.ptr(gy), gy.stride(0), _lib.ptr(scaled), _lib.ptr(scaled[C:]), 1.0,
                                                         _lib.ptr(sums), _lib.ptr(dx), dx.stride(0), _lib.ptr(cs), _lib.ptr(ws), nws,
                                                         _lib.stream()), "egnn_bn_act_bwd_apply_f32")
        if cs is not None:
            dx._egnn_colsum = (cs, dx._version)
        return dx, sums[C:], sums[:C], None, None, None, None, None, None, None, None, None


def _bn_prepare(x: Tensor, bn, p: float, training: bool):
    """Statistics + module state update of a fused BatchNorm call; None when the kernels do not take the shape (torch fallback).
    Returns (x row-major, mean, var, use_batch, drop, seed)."""
    x_in = x
    if not _bn_shape_ok(_rowmajor(x)) or not bn.track_running_stats or bn.weight is None:
        return None
    x = _rowmajor(x)
    n, C = x.shape
    use_batch = training  # nn.BatchNorm1d: batch statistics in training mode, running statistics in eval mode
    if use_batch:
        lib, dev = _lib.load(), x.device
        pre = getattr(x_in, "_egnn_bn_stats", None)   # formed in the producing aggregation's epilogue (ops.spmm)
        if pre is not None and pre[0].shape[0] == C and pre[2] == x_in._version:
            mean, var = pre[0], pre[1]
        else:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            var = torch.empty(C, dtype=torch.float32, device=dev)
            nws = lib.egnn_bn_ws_floats(C)
            ws = torch.empty(nws, dtype=torch.float32, device=dev)
            _lib.check(lib.egnn_bn_stats_f32(_lib.ptr(x), x.stride(0), n, C, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(ws), nws, _lib.stream()),
                       "egnn_bn_stats_f32")
        with torch.no_grad():   # nn.BatchNorm1d's state update, one launch (momentum=None: the cumulative average, formed on the device)
            rm, rv, nbt = bn.running_mean, bn.running_var, bn.num_batches_tracked
            if rm.dtype == torch.float32 and rv.dtype == torch.float32 and nbt.dtype == torch.int64 and rm.is_contiguous() and rv.is_contiguous():
                _lib.check(lib.egnn_bn_running_update_f32(_lib.ptr(mean), _lib.ptr(var), C, n, -1.0 if bn.momentum is None else float(bn.momentum),
                                                          _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt), _lib.stream()), "egnn_bn_running_update_f32")
            else:
                bn.num_batches_tracked += 1
                m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1 - m).add_(mean, alpha=m)
                bn.running_var.mul_(1 - m).add_(var, alpha=m * n / max(n - 1, 1))
    else:
        mean, var = bn.running_mean, bn.running_var
    drop = p if (training and p > 0) else 0.0
    seed = _draw_dropout_seed() if drop > 0 else 0
    return x, mean, var, use_batch, drop, seed


def bn_act(x: Tensor, bn: "torch.nn.BatchNorm1d", relu: bool = True, p: float = 0.0, training: bool | None = None,
           pick: Tensor | None = None) -> Tensor:
    """dropout(relu(bn(x)), p) in two kernels (statistics + apply); same module state updates as nn.BatchNorm1d.
    ``pick``: return only the rows ``pick`` of that result (unique int64 ids; the statistics still span all rows of x).

    Falls back to the torch operators (still on the GPU) for shapes the kernel does not take (C % 4 != 0, C > 1024)."""
    training = bn.training if training is None else training
    prep = _bn_prepare(x, bn, p, training)
    if prep is None:
        y = bn(x)
        y = torch.relu(y) if relu else y
        y = torch.nn.functional.dropout(y, p, training) if p > 0 else y
        return y if pick is None else y[pick]
    x, mean, var, use_batch, drop, seed = prep
    return _BnAct.apply(x, bn.weight, bn.bias, mean, var, bn.eps, relu, drop, seed, use_batch, pick)


_INV_ROWS = _cache.TensorKeyedCache(capacity=16)


def _inverse_rows(idx: Tensor, n: int) -> Tensor:
    """int32 [n]: position of row r in the unique id list ``idx``, -1 where r is not listed.  Built once per index tensor (identity +
    version + length: the train split does not change between steps); the entry keeps ``idx`` alive (_cache.py)."""
    def build():
        inv = torch.full((n,), -1, dtype=torch.int32, device=idx.device)
        inv[idx] = torch.arange(idx.numel(), dtype=torch.int32, device=idx.device)
        return inv
    return _INV_ROWS.get((idx,), (n,), build)


def _bn_act_linear_fwd(x, w, gamma, beta, mean, var, eps, relu, p, seed, seed_dev):
    """(h, h @ w) for h = drop(relu(bn(x))) with the given statistics: one pass over x, h stored and multiplied by w while its pieces
    are in registers (egnn_bn_act_linear_fwd_f32); where that kernel refuses the shape (EGNN_EALIGN), ``_bn_act_fwd`` + ``gemm_raw``.
    A shard without rows launches nothing."""
    n, C = x.shape
    if n > 0 and w.stride(0) % 4 == 0 and w.data_ptr() % 16 == 0:
        h = torch.empty(n, C, dtype=torch.float32, device=x.device)
        xw = torch.empty(n, w.shape[1], dtype=torch.float32, device=x.device)
        bn = _bn_desc(x, gamma, beta, mean, var, eps, relu, p, seed, seed_dev)
        rc = _lib.load().egnn_bn_act_linear_fwd_f32(ctypes.byref(bn), _lib.ptr(w), w.stride(0), 0, w.shape[1], _lib.ptr(h), h.stride(0),
                                                    _lib.ptr(xw), xw.stride(0), _lib.stream())
        if rc != _lib.EGNN_EALIGN:
            _lib.check(rc, "egnn_bn_act_linear_fwd_f32")
            return h, xw
    h = _bn_act_fwd(x, gamma, beta, mean, var, eps, relu, p, seed, seed_dev)
    return h, (gemm_raw(h, w, False, False) if n > 0 else torch.empty(0, w.shape[1], dtype=torch.float32, device=x.device))


class _BnActLinear(torch.autograd.Function):
    """(h, h @ w) with h = drop(relu(bn(x))) and a NARROW w [C, Ks] (the class count): the student's last hidden layer feeding its
    output conv (gnn.py:47-52).  h also carries the gradient tap of ``grad_tap`` (the projection head's row-compact input gradient).
    Backward: dh = G w^T + tap rows (+ any dense gradient of h) is formed in MFMA tiles and goes through the BatchNorm backward
    without being stored (egnn_skinny_dx_bn_bwd_reduce_f32): one pass over [n, C] instead of four.  ``sync``: as in ``_BnAct`` (all-rank
    statistics; the backward's reduce and apply halves around ONE all-reduce, see ``_tail_backward``)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, var, eps, relu, p, seed, batch_stats, w, box, sync=None):
        x = _rowmajor(x)
        w = _rowmajor(w)
        seed_dev = _DROPOUT_SEED_DEV if p > 0 else None
        h, xw = _bn_act_linear_fwd(x, w, gamma, beta, mean, var, eps, relu, p, seed, seed_dev)
        ctx.save_for_backward(x, gamma, beta, mean, var, h, w)
        ctx.cfg = (float(eps), int(relu), float(p), int(seed), int(batch_stats))
        ctx.seed_dev, ctx.box, ctx.w_index, ctx.sync = seed_dev, box, 10, sync
        ctx.set_materialize_grads(False)
        return h, xw

    @staticmethod
    def backward(ctx, g_h, g_xw):
        x, gamma, beta, mean, var, h, w = ctx.saved_tensors
        eps, relu, p, seed, batch_stats = ctx.cfg
        dx, dgamma, dbeta, gw = _tail_backward(ctx, g_h, g_xw, x, gamma, beta, mean, var, h, w, eps, relu, p, seed, batch_stats, ctx.sync)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, gw, None, None


def _tail_backward(ctx, g_h, g_xw, x, gamma, beta, mean, var, h, w, eps, relu, p, seed, batch_stats, sync):
    """Backward of (h, h @ w) = tail(x): dW = h^T G; dh = G w^T (+ tap rows, + dense g_h) through the BatchNorm backward.
    ``sync`` = None: statistics of this tensor alone (1 / n).  ``sync`` = (total rows [1] on the device, group): the column sums
    (sum d, sum d xhat) are all-reduced between the reduce half and the apply half (SyncBN on node-range shards); the returned
    dgamma / dbeta are then this shard's LOCAL sums (the flat gradient all-reduce adds the shards)."""
    pend = []
    if ctx.box is not None:
        pend, ctx.box.pending = ctx.box.pending, []
        pend = [(i, r) for i, r in pend if r.shape[0] > 0]      # (a shard without train rows taps zero rows: nothing to add)
    n, C = x.shape
    Ks = w.shape[1]
    lib, dev = _lib.load(), x.device
    gw = None
    if g_xw is not None:
        g_xw = _rowmajor(g_xw)
        if ctx.needs_input_grad[ctx.w_index]:
            gw = gemm_raw(h, g_xw, True, False) if n > 0 else torch.zeros_like(w)     # dW = h^T G
    if not ctx.needs_input_grad[0]:
        return None, None, None, gw
    dx = torch.empty_like(x)
    sums = torch.empty(2 * C, dtype=torch.float32, device=dev)       # [dbeta | dgamma]; written by the reduce half (zeroed on an empty shard)
    if n == 0:
        sums.zero_()
    dbeta, dgamma = sums[:C], sums[C:]
    cs = torch.empty(C, dtype=torch.float32, device=dev) if (batch_stats and n > 0) else None
    if g_h is not None:
        g_h = _rowmajor(g_h.to_dense() if g_h.is_sparse else g_h)
    fused = (n > 0 and g_xw is not None and len(pend) <= 1 and C % 64 == 0 and Ks <= 64 and x.stride(0) % 4 == 0
             and (g_h is None or (g_h.stride(0) % 4 == 0 and g_h.data_ptr() % 16 == 0)))
    rows = inv = None
    if fused and pend:
        idx, rows = pend[0]
        rows = _rowmajor(rows)
        # (the fused kernel reads the tap rows through an inverse row map, which exists for unique ids only: a RowsPlan takes the separate passes)
        fused = rows.stride(0) % 4 == 0 and rows.data_ptr() % 16 == 0 and rows.shape[1] == C and not isinstance(idx, RowsPlan)
        if fused:
            inv = _inverse_rows(idx, n)

    bn = ctypes.byref(_bn_desc(x, gamma, beta, mean, var, eps, relu, p, seed, ctx.seed_dev))

    def apply_sums():
        """(sum_dbeta, sum_dgamma, inv_count) the apply half uses; the all-rank sum on shards."""
        if sync is None:
            return dbeta, dgamma, (1.0 / n if batch_stats else 0.0)
        red = _sync_sums(sums, sync)
        return red[:C], red[C:], 1.0

    done = False
    if fused:
        nws = lib.egnn_skinny_dx_bn_ws_floats(n, C)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        rc = lib.egnn_skinny_dx_bn_bwd_reduce_f32(_lib.ptr(g_xw), g_xw.stride(0), _lib.ptr(w), w.stride(0), 0, Ks, 1.0, _lib.ptr(g_h),
                                                  0 if g_h is None else g_h.stride(0), _lib.ptr(rows), 0 if rows is None else rows.stride(0),
                                                  _lib.ptr(inv), bn, _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dx), dx.stride(0), _lib.ptr(ws),
                                                  nws, _lib.stream())
        if rc != _lib.EGNN_EALIGN:     # EGNN_EALIGN: beyond the kernel's 32-bit element offsets (n * ld >= 2^31) -> the separate passes below
            _lib.check(rc, "egnn_skinny_dx_bn_bwd_reduce_f32")
            sb, sg, inv_count = apply_sums()
            _lib.check(lib.egnn_bn_bwd_apply_stored_f32(bn, _lib.ptr(sb), _lib.ptr(sg), inv_count, _lib.ptr(dx), dx.stride(0), _lib.ptr(cs),
                                                        _lib.ptr(ws), nws, _lib.stream()), "egnn_bn_bwd_apply_stored_f32")
            done = True
    if not done:
        # the separate passes: dense dh, the tap rows added into it, the BatchNorm backward (reduce, [all-reduce,] apply; the column
        # sums of dx -- the bias gradient of the conv in front -- in the apply pass, as on the fused route)
        dh = None
        if n > 0:
            dh = gemm_raw(g_xw, w, False, True) if g_xw is not None else None
            if dh is None:
                dh = g_h.clone() if g_h is not None else torch.zeros_like(x)
            elif g_h is not None:
                dh = dh + g_h
            for idx, rows in pend:
                _tap_rows_add(dh, idx, rows)
            nws = lib.egnn_bn_ws_floats(C)
            ws = torch.empty(nws, dtype=torch.float32, device=dev)
            _lib.check(lib.egnn_bn_act_bwd_reduce_f32(bn, _lib.ptr(dh), dh.stride(0), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), nws,
                                                      _lib.stream()), "egnn_bn_act_bwd_reduce_f32")
        sb, sg, inv_count = apply_sums()
        if n > 0:
            _lib.check(lib.egnn_bn_act_bwd_apply_f32(bn, _lib.ptr(dh), dh.stride(0), _lib.ptr(sb), _lib.ptr(sg), inv_count, None, _lib.ptr(dx),
                                                     dx.stride(0), _lib.ptr(cs), _lib.ptr(ws), nws, _lib.stream()), "egnn_bn_act_bwd_apply_f32")
    if cs is not None:
        dx._egnn_colsum = (cs, dx._version)
    return dx, dgamma, dbeta, gw


def bn_act_linear(x: Tensor, bn: "torch.nn.BatchNorm1d", w: Tensor, relu: bool = True, p: float = 0.0, training: bool | None = None):
    """(h, h @ w) for h = dropout(relu(bn(x)), p) and a narrow ``w`` [C, Ks <= 64] -- ``bn_act`` + ``grad_tap`` + ``matmul`` with ONE
    backward pass over the [n, C] tensors (see _BnActLinear).  h carries the tap for ``linear_rows``.  None when the fused kernels do
    not take the shape (the caller then composes the three calls)."""
    training = bn.training if training is None else training
    if not (torch.is_grad_enabled() and x.is_cuda and x.dim() == 2 and w.dim() == 2 and w.shape[0] == x.shape[1] and w.shape[1] <= 64
            and x.shape[1] % 64 == 0):
        return None
    prep = _bn_prepare(x, bn, p, training)
    if prep is None:
        return None
    x, mean, var, use_batch, drop, seed = prep
    box = _TapBox()
    h, xw = _BnActLinear.apply(x, bn.weight, bn.bias, mean, var, bn.eps, relu, drop, seed, use_batch, w, box)
    h._egnn_tap = box
    return h, xw


# ------------------------------------------------------------------------------------------------
# the same fused BatchNorm + ReLU + dropout with batch statistics that span all ranks (node-range shards)
# ------------------------------------------------------------------------------------------------
_ROW_COUNTS: dict = {}


def _row_count(n: int, dev) -> Tensor:
    """float32 [1] device constant holding ``n`` (made once per value and device, never written)."""
    key = (int(n), str(dev))
    t = _ROW_COUNTS.get(key)
    if t is None:
        # never evicted (4 bytes each): captured graphs read these constants through raw pointers for as long as they live
        t = _ROW_COUNTS[key] = torch.full((1,), float(n), dtype=torch.float32, device=dev)
    return t


def _sync_stats(x: Tensor, group):
    """(mean, biased var, total rows [1]) of the rows of ALL ranks: the per-shard (mean, var, n) triples are all-gathered and merged in
    rank order (Chan's parallel-variance formula, identical on every rank).  An empty shard contributes n = 0."""
    import torch.distributed as dist
    n, C = x.shape
    lib, dev = _lib.load(), x.device
    world = dist.get_world_size(group)
    stats = torch.empty(2 * C + 1, dtype=torch.float32, device=dev)  # [mean | var | n]
    if n == 0:
        stats.zero_()
    else:
        nws = lib.egnn_bn_ws_floats(C)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        _lib.check(lib.egnn_bn_stats_f32(_lib.ptr(x), x.stride(0), n, C, _lib.ptr(stats), _lib.ptr(stats[C:]), _lib.ptr(ws), nws,
                                         _lib.stream()), "egnn_bn_stats_f32")
    if world == 1:
        return stats[:C], stats[C:2 * C], _row_count(n, dev)          # (a cached constant: no fill launch per call)
    if n > 0:
        stats[2 * C:].fill_(float(n))     # a fill kernel, not a host->device copy
    allst = torch.empty(world, 2 * C + 1, dtype=torch.float32, device=dev)
    dist.all_gather_into_tensor(allst, stats, group=group)
    merged = torch.empty(2 * C + 1, dtype=torch.float32, device=dev)
    mean, var, total = merged[:C], merged[C:2 * C], merged[2 * C:]
    _lib.check(lib.egnn_bn_merge_shards_f32(_lib.ptr(allst), world, C, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(total), _lib.stream()),
               "egnn_bn_merge_shards_f32")
    return mean, var, total


def sync_bn_act(x: Tensor, bn, relu: bool, p: float, training: bool, group=None, pick: Tensor | None = None):
    """Training-mode dropout(relu(bn(x))) with all-rank statistics; returns (y, mean, biased var, total rows) so that the
    module can update its running statistics.  ``bn`` needs weight / bias / eps (dist.SyncBatchNorm1d).  ``pick``: only those rows of
    the result (unique int64 row ids, may be empty; the statistics, and dx, still span every row of every rank -- the projection
    heads under a sampled criterion, gnn.py:296-306 -> criterion.py:62-65,134-137).  Two small collectives per direction: the
    statistics all-gather (``_sync_stats``) and the backward's all-reduce (``_BnAct``)."""
    drop = p if (training and p > 0) else 0.0
    seed = _draw_dropout_seed() if drop > 0 else 0
    x = _rowmajor(x)
    mean, var, total = _sync_stats(x, group)
    y = _BnAct.apply(x, bn.weight, bn.bias, mean, var, bn.eps, relu, drop, seed, True, pick, (total, group))
    return y, mean, var, total


def sync_bn_act_linear(x: Tensor, bn, w: Tensor, relu: bool, p: float, training: bool, group=None):
    """(h, h @ w, mean, var, total) -- ``bn_act_linear`` with all-rank statistics (dist.SyncBatchNorm1d.fused_act_linear); None when
    the fused kernels do not take the shape.  Forward: statistics all-gather, then the one-pass tail kernel; backward: the tail's
    reduce half, ONE all-reduce of [sum d | sum d xhat], the apply half."""
    if not (training and torch.is_grad_enabled() and x.is_cuda and x.dim() == 2 and w.dim() == 2 and w.shape[0] == x.shape[1]
            and w.shape[1] <= 64 and x.shape[1] % 64 == 0 and _bn_shape_ok(_rowmajor(x))):
        return None
    drop = p if p > 0 else 0.0
    seed = _draw_dropout_seed() if drop > 0 else 0
    x = _rowmajor(x)
    mean, var, total = _sync_stats(x, group)
    box = _TapBox()
    h, xw = _BnActLinear.apply(x, bn.weight, bn.bias, mean, var, bn.eps, relu, drop, seed, True, w, box, (total, group))
    h._egnn_tap = box
    return h, xw, mean, var, total


def bn_shape_ok(x: Tensor) -> bool:
    return _bn_shape_ok(_rowmajor(x))


# ------------------------------------------------------------------------------------------------
# SIGN: hop-batched Linear -> PReLU -> dropout (csrc/sign.hip; /root/reference/arxiv_dgl/sign.py:105-162)
# ------------------------------------------------------------------------------------------------
_SIGN_MAX_SEG = 16


def _sign_seeds(H: int, p: float, training: bool, seeds):
    """One dropout seed per segment, drawn in segment order -- and only when a mask is drawn at all (``training and p > 0``);
    ``seeds``: the caller drew them already (models.SIGN draws in the reference's dropout call order)."""
    if not (training and p > 0):
        return None
    if seeds is None:
        seeds = [_draw_dropout_seed() for _ in range(H)]
    if len(seeds) != H:
        raise ValueError(f"expected {H} dropout seeds, got {len(seeds)}")
    return tuple(int(s) for s in seeds)


def _sign_desc(B, Cs, H, p, seeds, slopes=None, srcs=None, batch=None):
    """The egnn_sign_seg_t descriptor (include/egnn_hip.h) and the host arrays it points at (kept alive by the returned tuple)."""
    u64 = (ctypes.c_uint64 * H)(*(seeds if seeds is not None else [0] * H))
    keep = [u64]
    d = _lib.SignSeg()
    d.B, d.Cs, d.H = B, Cs, H
    d.p = float(p) if seeds is not None else 0.0
    d.seed = ctypes.addressof(u64) if seeds is not None else None
    d.seed_dev = _lib.ptr(_DROPOUT_SEED_DEV) if seeds is not None else None
    if slopes is not None:
        arr = (ctypes.c_void_p * H)(*[t.data_ptr() for t in slopes])
        keep.append(arr)
        d.slope = ctypes.addressof(arr)
    if srcs is not None:
        arr = (ctypes.c_void_p * H)(*[t.data_ptr() for t in srcs])
        lds = (ctypes.c_int64 * H)(*[t.stride(0) for t in srcs])
        keep += [arr, lds]
        d.src, d.ld_src, d.n_src = ctypes.addressof(arr), ctypes.addressof(lds), srcs[0].shape[0]
        d.batch = _lib.ptr(batch)
    return d, keep


def sign_gather_drop(feats, batch: Tensor, p: float, training: bool, seeds=None) -> Tensor:
    """``torch.cat([F.dropout(x[batch], p, training) for x in feats], 1)`` -> [B, H*F] in ONE launch (egnn_sign_gather_drop_f32): the
    batch gather, ``input_drop`` and the layout the first Linear of every hop reads (sign.py:236,151).  The hop features are
    constants: no backward.  One seed per hop from ``_draw_dropout_seed``, in hop order (``training and p > 0`` only)."""
    feats = [_rowmajor(_lib.real(f)) for f in feats]
    _lib.require_gpu(batch, *feats)
    H = len(feats)
    if any(f.requires_grad for f in feats) and torch.is_grad_enabled():
        raise NotImplementedError("sign_gather_drop: the hop features are constants (no backward)")
    if H == 0 or any(f.shape != feats[0].shape for f in feats):
        raise ValueError("sign_gather_drop: expected hop feature matrices of one shape")
    if H > _SIGN_MAX_SEG:
        raise _lib.HipExtensionError(f"sign_gather_drop: at most {_SIGN_MAX_SEG} hops per call")
    if batch.dtype != torch.int64 or batch.dim() != 1:
        raise TypeError("sign_gather_drop: `batch` must be an int64 vector of row ids")
    batch = batch.contiguous()
    N, Fdim = feats[0].shape
    B = batch.numel()
    seeds = _sign_seeds(H, p, training, seeds)
    out = torch.empty(B, H * Fdim, dtype=torch.float32, device=feats[0].device)
    if B > 0 and Fdim > 0:
        d, keep = _sign_desc(B, Fdim, H, p, seeds, srcs=feats, batch=batch)
        _lib.check(_lib.load().egnn_sign_gather_drop_f32(ctypes.byref(d), _lib.ptr(out), out.stride(0), _lib.stream()),
                   "egnn_sign_gather_drop_f32")
    return out


class _PreluDrop(torch.autograd.Function):
    """y = drop(prelu(z, a_h)) per column segment of z [B, H*Cs]; saves z (never a mask).  The backward forms dz, every slope gradient
    and the column sums of dz in one pass; dz carries the column sums (``_egnn_colsum``) for the Linear that produced z."""

    @staticmethod
    def forward(ctx, z, Cs, p, seeds, *slopes):
        z = _rowmajor(z)
        B, HC = z.shape
        H = len(slopes)
        y = torch.empty(B, HC, dtype=torch.float32, device=z.device)
        if B > 0:
            d, keep = _sign_desc(B, Cs, H, p, seeds, slopes=slopes)
            _lib.check(_lib.load().egnn_prelu_drop_fwd_f32(ctypes.byref(d), _lib.ptr(z), z.stride(0), _lib.ptr(y), y.stride(0),
                                                           _lib.stream()), "egnn_prelu_drop_fwd_f32")
        ctx.save_for_backward(z, *slopes)
        ctx.cfg = (int(Cs), float(p), seeds)
        return y

    @staticmethod
    def backward(ctx, gy):
        z, *slopes = ctx.saved_tensors
        Cs, p, seeds = ctx.cfg
        gy = _rowmajor(gy)
        B, HC = z.shape
        H, dev = len(slopes), z.device
        lib = _lib.load()
        dz = torch.empty(B, HC, dtype=torch.float32, device=dev)
        if B == 0:
            return (dz, None, None, None, *[torch.zeros_like(a) for a in slopes])
        da = torch.empty(H, dtype=torch.float32, device=dev)
        cs = torch.empty(HC, dtype=torch.float32, device=dev)
        nws = lib.egnn_prelu_drop_ws_floats(B, Cs, H)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        d, keep = _sign_desc(B, Cs, H, p, seeds, slopes=slopes)
        _lib.check(lib.egnn_prelu_drop_bwd_f32(ctypes.byref(d), _lib.ptr(z), z.stride(0), _lib.ptr(gy), gy.stride(0), _lib.ptr(dz),
                                               dz.stride(0), _lib.ptr(da), _lib.ptr(cs), _lib.ptr(ws), nws, _lib.stream()),
                   "egnn_prelu_drop_bwd_f32")
        dz._egnn_colsum = (cs, dz._version)
        return (dz, None, None, None, *[da[h:h + 1].view(a.shape) for h, a in enumerate(slopes)])


def prelu_drop(z: Tensor, slopes, Cs: int, p: float, training: bool, seeds=None) -> Tensor:
    """``F.dropout(F.prelu(z_h, a_h), p, training)`` for every column segment z_h = z[:, h*Cs:(h+1)*Cs] in ONE launch
    (egnn_prelu_drop_fwd_f32 / _bwd_f32; sign.py:132,155).  ``slopes``: one learnable one-element tensor per segment, read from
    device memory by every launch.  One seed per segment from ``_draw_dropout_seed`` in segment order, only when ``training and
    p > 0`` (``seeds``: already drawn by the caller).  Gradients: z and every slope."""
    z = _lib.real(z)
    slopes = list(slopes)
    _lib.require_gpu(z, *slopes)
    H = len(slopes)
    if z.dim() != 2 or H < 1 or z.shape[1] != H * Cs:
        raise ValueError(f"prelu_drop: z must be [B, {H} * {Cs}]")
    if any(a.numel() != 1 or a.dtype != torch.float32 for a in slopes):
        raise ValueError("prelu_drop: every slope is a one-element float32 tensor (nn.PReLU())")
    if H > _SIGN_MAX_SEG:
        raise _lib.HipExtensionError(f"prelu_drop: at most {_SIGN_MAX_SEG} segments per call")
    return _PreluDrop.apply(z, int(Cs), float(p), _sign_seeds(H, p, training, seeds), *slopes)


def _block_operand(x, h: int, H: int, rows):
    """(A operand, a_rows) of hop h: a column block of the shared [B, H*Cin] buffer, or hop h's own matrix with the rows ``rows``
    (int64 ids: gathered in the GEMM's operand load; a ``range``: a slice; None: all)."""
    if torch.is_tensor(x):
        Cin = x.shape[1] // H
        return x[:, h * Cin:(h + 1) * Cin], None
    if isinstance(rows, range):
        return x[h][rows.start:rows.stop], None
    return x[h], rows


class _LinearBlocks(torch.autograd.Function):
    """z[:, h*Cout:(h+1)*Cout] = x_h @ W_h^T + b_h for H hops as ONE autograd node over ONE [B, H*Cout] buffer: every GEMM writes its
    column block (``gemm_raw(out=)``: no torch.cat), the backward reads the blocks of dz as strided operands (no split copy), writes
    dX into the blocks of one buffer, and takes the bias gradients from the column sums dz carries (``colsum``)."""

    @staticmethod
    def forward(ctx, x, rows, H, *tensors):
        feats, ws, bs = tensors[:len(tensors) - 2 * H], tensors[len(tensors) - 2 * H:len(tensors) - H], tensors[len(tensors) - H:]
        src = x if x is not None else [_gemm_operand(f) for f in feats]
        a0, r0 = _block_operand(src, 0, H, rows)
        B = a0.shape[0] if r0 is None else r0.numel()
        Cout = ws[0].shape[0]
        z = torch.empty(B, H * Cout, dtype=torch.float32, device=ws[0].device)
        for h in range(H):
            a, r = _block_operand(src, h, H, rows)
            gemm_raw(a, ws[h], False, True, bs[h], a_rows=r, out=z[:, h * Cout:(h + 1) * Cout])
        ctx.save_for_backward(*([x] if x is not None else []), *([rows] if torch.is_tensor(rows) else []), *feats, *ws)
        ctx.cfg = (H, x is not None, rows if not torch.is_tensor(rows) else "tensor", len(feats))
        ctx.tap_box = getattr(x, "_egnn_tap", None) if x is not None else None
        return z

    @staticmethod
    def backward(ctx, gz):
        H, has_x, rows, n_feat = ctx.cfg
        saved = list(ctx.saved_tensors)
        x = saved.pop(0) if has_x else None
        if rows == "tensor":
            rows = saved.pop(0)
        feats, ws = saved[:n_feat], saved[n_feat:]
        src = x if has_x else feats
        gz = _rowmajor(gz)
        Cout = ws[0].shape[0]
        need_w, need_b = ctx.needs_input_grad[3 + n_feat:3 + n_feat + H], ctx.needs_input_grad[3 + n_feat + H:]
        cs = colsum(gz) if any(need_b) else None
        gx = torch.empty_like(x) if has_x and ctx.needs_input_grad[0] else None
        gws, gbs = [], []
        for h in range(H):
            g = gz[:, h * Cout:(h + 1) * Cout]
            a, r = _block_operand(src, h, H, rows)
            if gx is not None:
                Cin = x.shape[1] // H
                gemm_raw(g, ws[h], False, False, out=gx[:, h * Cin:(h + 1) * Cin])        # dX_h = dZ_h W_h
            gws.append(gemm_raw(g, a, True, False, b_rows=r) if need_w[h] else None)      # dW_h = dZ_h^T X_h
            gbs.append(cs[h * Cout:(h + 1) * Cout] if need_b[h] else None)
        return (_fresh(gx, ctx.tap_box), None, None, *([None] * n_feat), *gws, *gbs)


def linear_blocks(x, weights, biases, rows=None) -> Tensor:
    """H independent ``nn.Linear`` layers over the H hops into ONE [B, H*out] buffer (block-diagonal product; sign.py:130 for every hop
    of one level).  ``x``: the previous level's [B, H*in] buffer, or a list of the H constant hop feature matrices [N, in] whose rows
    ``rows`` are used (int64 ids, fused into the operand load; a ``range``: a slice; None: all rows).  ``weights`` [out, in] and
    ``biases`` [out] per hop, all of one shape."""
    weights, biases = list(weights), list(biases)
    H = len(weights)
    if H < 1 or len(biases) != H or any(w.shape != weights[0].shape for w in weights) or any(b is None for b in biases):
        raise ValueError("linear_blocks: one [out, in] weight and one bias per hop, all of one shape")
    if torch.is_tensor(x):
        x = _lib.real(x)
        _lib.require_gpu(x)
        if x.dim() != 2 or x.shape[1] != H * weights[0].shape[1] or rows is not None:
            raise ValueError("linear_blocks: a shared input buffer is [B, H * in] and takes no `rows`")
        return _LinearBlocks.apply(_rowmajor(x), None, H, *weights, *biases)
    feats = [_lib.real(f) for f in x]
    _lib.require_gpu(*feats)
    if len(feats) != H or any(f.requires_grad for f in feats):
        raise ValueError("linear_blocks: one constant feature matrix per hop")
    if torch.is_tensor(rows):
        _lib.require_gpu(rows)
    return _LinearBlocks.apply(None, rows, H, *feats, *weights, *biases)


# ------------------------------------------------------------------------------------------------
# MAG group_input (mag_pyg/gnn.py:117-127) in one launch; the read side of the row-lazy Adam (optim.py)
# ------------------------------------------------------------------------------------------------
_GROUP_INPUT_MAX_TYPES = 8
_GROUP_OOB: dict = {}     # device -> int32 [1]: rows group_input wrote as zeros because their type / index was out of range


def group_input_oob(device, reset: bool = True) -> int:
    """How many rows ``group_input`` zero-filled on ``device`` because their node type or index was out of range, since the last reset.
    A host read: ``LazyRowAdam.flush`` asks (and raises), next to its own counter reads."""
    c = _GROUP_OOB.get(torch.device(device))
    if c is None:
        return 0
    n = int(c.item())
    if reset and n:
        c.zero_()
    return n


def _group_input_fwd(tables, node_type: Tensor, local_idx: Tensor, D: int, oob: Tensor | None = None) -> Tensor:
    """``tables``: list indexed by node type (None: no table, zeros).  One egnn_group_input_f32 launch, no host read."""
    n, T = node_type.numel(), len(tables)
    dev = node_type.device
    if oob is None:
        oob = _GROUP_OOB.get(dev)
        if oob is None:
            oob = _GROUP_OOB[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    h = torch.empty((n, D), dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_void_p * T)(*[None if t is None else t.data_ptr() for t in tables])
    rows = (ctypes.c_int64 * T)(*[0 if t is None else t.shape[0] for t in tables])
    _lib.check(_lib.load().egnn_group_input_f32(ctypes.addressof(ptrs), ctypes.addressof(rows), T, _lib.ptr(node_type), _lib.ptr(local_idx),
                                                n, D, _lib.ptr(h), h.stride(0), _lib.ptr(oob), _lib.stream()), "egnn_group_input_f32")
    return h


class _GroupInput(torch.autograd.Function):
    """h[i] = tables[node_type[i]][local_idx[i]].  A table under the row-lazy Adam (``t._egnn_rows``) is caught up on the rows about to
    be read before the gather, and its backward leaves the gradient rows with that state instead of forming a dense gradient."""

    @staticmethod
    def forward(ctx, node_type, local_idx, D, oob, keys, states, *tensors):
        tables = [None] * (max(keys) + 1)
        for k, t, st in zip(keys, tensors, states):
            if st is not None:
                st.catch_up(k, node_type, local_idx)
            tables[k] = t.detach()
        ctx.keys, ctx.states, ctx.shapes = keys, states, [t.shape for t in tensors]
        ctx.save_for_backward(node_type, local_idx)
        return _group_input_fwd(tables, node_type, local_idx, D, oob)

    @staticmethod
    def backward(ctx, g):
        node_type, local_idx = ctx.saved_tensors
        g = g.contiguous()
        grads = []
        for j, (k, st, shape) in enumerate(zip(ctx.keys, ctx.states, ctx.shapes)):
            if st is not None:
                st.deposit(g, node_type, local_idx, k)
                grads.append(None)
            elif ctx.needs_input_grad[6 + j]:
                # the forward's own range test: rows it zero-filled (and counted) carry no gradient; no nonzero, no host wait
                ok = (node_type == k) & (local_idx >= 0) & (local_idx < shape[0])
                gt = torch.zeros(shape, dtype=g.dtype, device=g.device)
                if shape[0] > 0:
                    gt.index_add_(0, local_idx.clamp(0, shape[0] - 1), g * ok.unsqueeze(1).to(g.dtype))
                grads.append(gt)
            else:
                grads.append(None)
        return (None, None, None, None, None, None, *grads)


def group_input(sources: dict, node_type: Tensor, local_idx: Tensor, D: int, oob: Tensor | None = None) -> Tensor:
    """``h[i] = sources[node_type[i]][local_idx[i]]`` -> [n, D] in ONE launch: ``RGCN.group_input`` (mag_pyg/gnn.py:117-127) without a
    mask, a ``nonzero`` or a host wait per node type.  ``sources``: {node type id (0..7): contiguous fp32 [rows, D] tensor}; a type
    without a source gives zero rows, like the mask form.  A type or an index out of range gives a zero row and is counted in ``oob``
    (int32 [1] on the device; default: a per-device counter that ``group_input_oob`` reads and ``LazyRowAdam.flush`` raises on).  Sources stepped by ``optim.LazyRowAdam``
    are first caught up on the rows read (also under ``no_grad``) and get their gradient rows deposited for the optimiser's step;
    ``param.grad`` stays None.  Other sources that require grad get a dense gradient."""
    keys = tuple(int(k) for k in sources)
    tensors = [_lib.real(sources[k]) for k in sources]
    _lib.require_gpu(node_type, local_idx, *tensors)
    if not keys or min(keys) < 0 or max(keys) >= _GROUP_INPUT_MAX_TYPES or len(set(keys)) != len(keys):
        raise ValueError(f"group_input: node type ids must be distinct and in [0, {_GROUP_INPUT_MAX_TYPES})")
    if D % 4 != 0:
        raise _lib.HipExtensionError("group_input: D must be a multiple of 4")
    for t in tensors:
        if t.dim() != 2 or t.shape[1] != D or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"group_input: every source must be a contiguous fp32 [rows, {D}] tensor")
    if node_type.dtype != torch.int64 or local_idx.dtype != torch.int64 or node_type.shape != local_idx.shape or node_type.dim() != 1:
        raise TypeError("group_input: node_type and local_idx must be int64 vectors of one length")
    from .optim import row_state
    states = tuple(row_state(t) for t in tensors)
    return _GroupInput.apply(node_type.contiguous(), local_idx.contiguous(), int(D), oob, keys, states, *tensors)
