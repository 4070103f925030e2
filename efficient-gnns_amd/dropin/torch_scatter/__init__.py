"""Drop-in shim for ``torch_scatter``'s reductions along dim 0 on ``efficient_gnns_amd.ops.scatter`` (csrc/scatter.hip): what a
user-defined ``MessagePassing.aggregate`` calls -- and for its composite softmax functions on ``ops.scatter_softmax``
(csrc/scatter_softmax.hip; also importable from ``torch_scatter.composite``).  ``src`` float32 on the GPU, ``index`` 1-D int64; no float
atomics."""
from efficient_gnns_amd import ops as _ops


def _checked(src, index, dim, out, dim_size):
    if out is not None:
        raise NotImplementedError("torch_scatter shim: `out=` is not supported (the result is always a new tensor)")
    if dim not in (0, -src.dim()):
        raise NotImplementedError(f"torch_scatter shim: `dim` must be 0 (or {-src.dim()}), got {dim}")
    if index.dim() != 1:
        raise NotImplementedError(f"torch_scatter shim: `index` must be 1-D with one id per row of `src`, got shape {tuple(index.shape)}")
    if dim_size is None:
        dim_size = int(index.max()) + 1 if index.numel() else 0      # (a host read, as in torch_scatter: pass dim_size to avoid it)
    return int(dim_size)


def scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    if reduce not in ("sum", "add", "mean", "max", "min"):
        raise ValueError(f"torch_scatter shim: reduce must be sum | add | mean | max | min, got {reduce!r}")
    n = _checked(src, index, dim, out, dim_size)
    if reduce in ("max", "min"):
        return _ops.scatter(src, index, n, reduce, return_arg=True)[0]
    return _ops.scatter(src, index, n, reduce)


def scatter_add(src, index, dim=-1, out=None, dim_size=None):
    return _ops.scatter(src, index, _checked(src, index, dim, out, dim_size), "sum")


scatter_sum = scatter_add


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    return _ops.scatter(src, index, _checked(src, index, dim, out, dim_size), "mean")


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    return _ops.scatter(src, index, _checked(src, index, dim, out, dim_size), "max", return_arg=True)


def scatter_min(src, index, dim=-1, out=None, dim_size=None):
    return _ops.scatter(src, index, _checked(src, index, dim, out, dim_size), "min", return_arg=True)


def _softmax(src, index, dim, dim_size, log):
    """The composite functions on ``ops.scatter_softmax`` (csrc/scatter_softmax.hip; eps 0, as torch_scatter): inside a running
    ``MessagePassing.propagate`` whose target-side endpoint tensor ``index`` is, the call's own plan is used."""
    from efficient_gnns_amd.nn import running_plan
    _checked(src, index, dim, None, 0)                                   # the shim's `dim` / `index` errors (no host read)
    found = running_plan(index, dim_size, "dim_size")
    if found is not None:
        return _ops.scatter_softmax(src, index, found[1], plan=found[0], eps=0.0, log=log)
    return _ops.scatter_softmax(src, index, _checked(src, index, dim, None, dim_size), eps=0.0, log=log)


def scatter_softmax(src, index, dim=-1, dim_size=None):
    return _softmax(src, index, dim, dim_size, False)


def scatter_log_softmax(src, index, dim=-1, dim_size=None):
    return _softmax(src, index, dim, dim_size, True)
