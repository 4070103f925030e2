"""Host checks of the softmax over an unsorted index (csrc/scatter_softmax.hip, ``ops.scatter_softmax``, the multi-dimensional
``utils.softmax``, the ``torch_scatter`` composite shim): the C ABI additions against ``_lib.SIGNATURES``, the argument errors that must
come back before any launch, the drop-in imports and the option errors.  No GPU (the kernels: tests/test_gpu_scatter_softmax.py)."""
import ctypes
import importlib
import inspect
import os
import re
import sys

import pytest
import torch

from efficient_gnns_amd import _lib, ops, utils
from conftest import ROOT

EINVAL, EWORKSPACE, EALIGN = -1, -3, _lib.EGNN_EALIGN
NEW = ("egnn_scatter_softmax_ws_bytes", "egnn_scatter_softmax_fwd_f32", "egnn_scatter_softmax_bwd_f32")
CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
DROPIN = os.path.join(ROOT, "efficient-gnns_amd", "dropin")


def _header():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def _chunk():
    return int(re.search(r"#define\s+EGNN_ROWS_SUM_CHUNK\s+(\d+)", _header()).group(1))


@pytest.mark.parametrize("name", NEW)
def test_header_prototype_matches_the_binding_argument_by_argument(name):
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;{]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/egnn_hip.h"
    res, argtypes = _lib.SIGNATURES[name]
    assert res is CTYPE[m.group(1)]
    decls = [a.strip() for a in m.group(2).split(",")]
    assert len(decls) == len(argtypes), (decls, argtypes)
    for decl, ct in zip(decls, argtypes):
        want = ctypes.c_void_p if "*" in decl else CTYPE[re.sub(r"\bconst\b", "", decl).split()[0]]
        assert ct is want, (name, decl, ct)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"


def test_the_abi_is_still_9_and_the_source_is_listed():
    assert re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", _header())
    assert _lib.load().egnn_abi_version() == 9
    build = importlib.import_module("efficient_gnns_amd.build")
    assert "scatter_softmax.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "scatter_softmax.hip"))
    text = open(os.path.join(build.CSRC, "scatter_softmax.hip")).read()
    assert '#include "rows_runs.h"' in text and "atomic" not in text.split("namespace {", 1)[1]     # no atomics of any kind in the code
    runs = open(os.path.join(build.CSRC, "rows_runs.h")).read()
    assert '#include "rows_keys.h"' in runs and "atomic" not in runs
    # the run-sum's cut, not a constant of its own: the chunk, the cut, the slot rule and the size helpers are the shared header's
    assert "EGNN_ROWS_SUM_CHUNK" in text and "CHUNK = EGNN_ROWS_SUM_CHUNK;" in runs and "chunk_start(" in text and "key_usable(" in text
    for own in ("int64_t lower_bound", "int64_t part_slot", "int64_t part_pitch", "bool sizes_ok", "int64_t blocks_for", "EGNN_ROWS_SUM_CHUNK;"):
        assert own not in text and own in runs, own


def _buf():
    keep = (ctypes.c_float * 64)()                       # a 16-byte aligned stand-in: nothing is launched on these paths
    return (ctypes.addressof(keep) + 15) & ~15, keep


def test_workspace_is_zero_up_to_one_chunk_and_positive_above():
    lib, chunk = _lib.load(), _chunk()
    for C in (1, 3, 8, 256):
        assert lib.egnn_scatter_softmax_ws_bytes(0, C) == 0
        assert lib.egnn_scatter_softmax_ws_bytes(1, C) == 0
        assert lib.egnn_scatter_softmax_ws_bytes(chunk, C) == 0                   # no run can be longer than one chunk
        for S in (chunk + 1, 10 * chunk, 1_000_000):
            need = lib.egnn_scatter_softmax_ws_bytes(S, C)
            assert need >= 2 * 4 * C * 2 * ((S + chunk - 1) // chunk)             # a (max, sum) pair per column for two slots per window
    assert lib.egnn_scatter_softmax_ws_bytes(10 * chunk, 0) == 0


def _fwd(lib, base, **kw):
    S = kw.get("S", 3)
    shift = kw.get("shift", max(1, (S - 1).bit_length()))
    return lib.egnn_scatter_softmax_fwd_f32(kw.get("out", base), kw.get("ld_out", 8), kw.get("row_max", base), kw.get("row_den", base),
                                            kw.get("n_rows", 4), kw.get("keys", base), S, shift, kw.get("rows", base), kw.get("src", base),
                                            kw.get("ld_src", 8), kw.get("C", 8), kw.get("eps", 0.0), kw.get("form", 0), kw.get("ws", None),
                                            kw.get("ws_bytes", 0), None)


def _bwd(lib, base, **kw):
    S = kw.get("S", 3)
    shift = kw.get("shift", max(1, (S - 1).bit_length()))
    return lib.egnn_scatter_softmax_bwd_f32(kw.get("dsrc", base), kw.get("ld_dsrc", 8), kw.get("row_dot", base), kw.get("n_rows", 4),
                                            kw.get("keys", base), S, shift, kw.get("rows", base), kw.get("out", base), kw.get("ld_out", 8),
                                            kw.get("g", base), kw.get("ld_g", 8), kw.get("C", 8), kw.get("form", 0), kw.get("ws", None),
                                            kw.get("ws_bytes", 0), None)


def test_forward_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    chunk = _chunk()
    call = lambda **kw: _fwd(lib, base, **kw)   # noqa: E731
    for form in (0, 1):
        assert lib.egnn_scatter_softmax_fwd_f32(None, 8, None, None, 4, None, 0, 0, None, None, 8, 8, 0.0, form, None, 0, None) == 0   # S == 0
    assert call(form=2) == EINVAL and call(form=-1) == EINVAL
    assert call(C=0) == EINVAL and call(C=-3) == EINVAL and call(ld_out=7) == EINVAL and call(ld_src=4) == EINVAL
    assert call(S=-1) == EINVAL and call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL and call(shift=5) == EINVAL
    for name in ("out", "row_max", "row_den", "keys", "rows", "src"):
        assert call(**{name: None}) == EINVAL, name
    S = 3 * chunk + 5
    need = lib.egnn_scatter_softmax_ws_bytes(S, 8)
    assert need > 0
    assert call(S=S, ws=None, ws_bytes=need) == EWORKSPACE and call(S=S, ws=base, ws_bytes=need - 1) == EWORKSPACE
    assert call(S=S, ws=base + 4, ws_bytes=need) == EALIGN
    assert call(keys=base + 4) == EALIGN and call(rows=base + 4) == EALIGN
    for name in ("out", "row_max", "row_den", "src"):
        assert call(**{name: base + 2}) == EALIGN, name


def test_backward_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    chunk = _chunk()
    call = lambda **kw: _bwd(lib, base, **kw)   # noqa: E731
    for form in (0, 1):
        assert lib.egnn_scatter_softmax_bwd_f32(None, 8, None, 4, None, 0, 0, None, None, 8, None, 8, 8, form, None, 0, None) == 0       # S == 0
    assert call(form=2) == EINVAL and call(form=-1) == EINVAL
    assert call(C=0) == EINVAL and call(ld_dsrc=7) == EINVAL and call(ld_out=7) == EINVAL and call(ld_g=4) == EINVAL
    assert call(S=-1) == EINVAL and call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL and call(shift=5) == EINVAL
    for name in ("dsrc", "row_dot", "keys", "rows", "out", "g"):
        assert call(**{name: None}) == EINVAL, name
    S = 3 * chunk + 5
    need = lib.egnn_scatter_softmax_ws_bytes(S, 8)
    assert call(S=S, ws=None, ws_bytes=need) == EWORKSPACE and call(S=S, ws=base, ws_bytes=need - 1) == EWORKSPACE
    assert call(S=S, ws=base + 4, ws_bytes=need) == EALIGN
    assert call(keys=base + 4) == EALIGN and call(rows=base + 4) == EALIGN
    for name in ("dsrc", "row_dot", "out", "g"):
        assert call(**{name: base + 2}) == EALIGN, name


def test_composite_and_the_two_names_resolve_through_the_dropin_path():
    names = ("torch_geometric", "torch_scatter")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in names or k.startswith(tuple(n + "." for n in names))}
    sys.path.insert(0, DROPIN)
    try:
        import torch_scatter
        import torch_scatter.composite
        from torch_scatter.composite import scatter_log_softmax, scatter_softmax
        from torch_geometric.utils import softmax
        assert torch_scatter.composite.__file__.startswith(DROPIN)
        assert scatter_softmax is torch_scatter.scatter_softmax and scatter_log_softmax is torch_scatter.scatter_log_softmax
        assert softmax is utils.softmax
        src, index = torch.zeros(3, 2), torch.tensor([0, 1, 1])
        for fn in (scatter_softmax, scatter_log_softmax):
            with pytest.raises(NotImplementedError, match="dim"):
                fn(src, index, 1, dim_size=2)
            with pytest.raises(NotImplementedError, match="index"):
                fn(src, index.view(3, 1).expand(3, 2), 0, dim_size=2)
            with pytest.raises(_lib.HipExtensionError):
                fn(src, index, 0, dim_size=2)                                      # CPU tensors: no fallback
    finally:
        sys.path.remove(DROPIN)
        for k in [k for k in sys.modules if k in names or k.startswith(tuple(n + "." for n in names))]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_option_errors():
    x, index = torch.zeros(3, 2), torch.tensor([0, 1, 1])
    with pytest.raises(NotImplementedError, match="dim"):
        utils.softmax(x, index, dim=1)
    with pytest.raises(NotImplementedError, match="dim"):
        utils.softmax(x, index, dim=-1)
    with pytest.raises(ValueError, match="index"):
        utils.softmax(x)
    with pytest.raises(_lib.HipExtensionError):
        utils.softmax(x, index, num_nodes=2, dim=-2)                               # a valid spelling of the first axis; CPU tensors
    with pytest.raises(_lib.HipExtensionError):
        utils.softmax(x[:, 0], index, num_nodes=2)                                 # the 1-D path, as before
    with pytest.raises(_lib.HipExtensionError):
        ops.scatter_softmax(x, index, 2)
    plan = ops.RowsPlan(index, 2, 3)
    with pytest.raises(ValueError, match="plan was built for 2 rows"):
        ops.scatter_softmax(x, None, 4, plan=plan)
    sig = inspect.signature(ops.scatter_softmax).parameters
    assert list(sig) == ["src", "index", "dim_size", "plan", "eps", "log"]
    assert sig["plan"].default is None and sig["eps"].default == 0.0 and sig["log"].default is False
    sig = inspect.signature(utils.softmax).parameters
    assert list(sig) == ["src", "index", "ptr", "num_nodes", "dim"] and sig["dim"].default == 0
