"""Host checks of the device path for user-defined message-passing convs (csrc/scatter.hip, ``ops.scatter``, ``ops.rows_plan(check=
"deferred")``, ``nn.MessagePassing``, the ``torch_scatter`` shim): the C ABI additions against ``_lib.SIGNATURES``, the argument errors
that must come back before any launch, the drop-in imports and the option errors.  No GPU (the kernels themselves:
tests/test_gpu_message_passing.py)."""
import ctypes
import importlib
import inspect
import os
import re
import sys

import pytest
import torch

import efficient_gnns_amd as P
from efficient_gnns_amd import _lib, ops
from efficient_gnns_amd import nn as PN
from conftest import ROOT

EINVAL, EWORKSPACE, EALIGN = -1, -3, _lib.EGNN_EALIGN
NEW = ("egnn_rows_wrap_i64", "egnn_scatter_runs_ws_bytes", "egnn_scatter_runs_f32", "egnn_scatter_bwd_f32")
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
    assert "scatter.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "scatter.hip"))
    text = open(os.path.join(build.CSRC, "scatter.hip")).read()
    assert '#include "rows_runs.h"' in text and "atomic" not in text.split("namespace {", 1)[1]     # no atomics of any kind in the code
    runs = open(os.path.join(build.CSRC, "rows_runs.h")).read()
    assert '#include "rows_keys.h"' in runs and "atomic" not in runs and "CHUNK = EGNN_ROWS_SUM_CHUNK;" in runs
    # the cut, the slot rule and the size helpers are the shared header's
    for own in ("int64_t lower_bound", "int64_t part_slot", "int64_t part_pitch", "bool sizes_ok", "int64_t blocks_for", "EGNN_ROWS_SUM_CHUNK;"):
        assert own not in text and own in runs, own
    assert "egnn_rows_add_runs_f32(" in text                                      # sum / mean run the existing run-sum itself


def _buf():
    keep = (ctypes.c_float * 64)()                       # a 16-byte aligned stand-in: nothing is launched on these paths
    return (ctypes.addressof(keep) + 15) & ~15, keep


def test_scatter_workspace_sizes():
    lib, chunk = _lib.load(), _chunk()
    for red in range(4):
        assert lib.egnn_scatter_runs_ws_bytes(chunk, 256, red) == 0               # no run can be longer than one chunk
        assert lib.egnn_scatter_runs_ws_bytes(0, 256, red) == 0
    for S in (chunk + 1, 10 * chunk, 1_000_000):
        assert lib.egnn_scatter_runs_ws_bytes(S, 40, 0) == lib.egnn_scatter_runs_ws_bytes(S, 40, 1) == lib.egnn_rows_add_runs_ws_bytes(S, 40)
        # max / min keep a position (8 bytes) next to every partial value (4 bytes)
        assert lib.egnn_scatter_runs_ws_bytes(S, 40, 2) == lib.egnn_scatter_runs_ws_bytes(S, 40, 3) == 3 * lib.egnn_rows_add_runs_ws_bytes(S, 40)
    assert lib.egnn_scatter_runs_ws_bytes(10 * chunk, 40, 4) == 0                  # not a reduction


def test_scatter_forward_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    chunk = _chunk()

    def call(**kw):
        S = kw.get("S", 3)
        shift = kw.get("shift", max(1, (S - 1).bit_length()))
        return lib.egnn_scatter_runs_f32(kw.get("out", base), kw.get("ld_out", 8), kw.get("n_rows", 4), kw.get("count", base),
                                         kw.get("arg", None), kw.get("keys", base), S, shift, kw.get("src", base), kw.get("ld_src", 8),
                                         kw.get("C", 8), kw.get("reduce", 0), kw.get("ws", None), kw.get("ws_bytes", 0), None)
    for red in range(4):
        assert lib.egnn_scatter_runs_f32(None, 8, 4, None, None, None, 0, 0, None, 8, 8, red, None, 0, None) == 0   # S == 0, NULL operands
    assert call(reduce=4) == EINVAL and call(reduce=-1) == EINVAL
    assert call(ld_out=7) == EINVAL and call(ld_src=4) == EINVAL and call(C=0) == EINVAL
    assert call(out=None) == EINVAL and call(keys=None) == EINVAL and call(src=None) == EINVAL
    assert call(S=-1) == EINVAL and call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL and call(shift=5) == EINVAL
    assert call(reduce=1, count=None) == EINVAL                                    # mean needs the counts
    assert call(reduce=0, arg=base) == EINVAL                                      # arg belongs to max / min
    S = 3 * chunk + 5
    for red in range(4):
        need = lib.egnn_scatter_runs_ws_bytes(S, 8, red)
        assert need > 0
        assert call(S=S, reduce=red, ws=None, ws_bytes=need) == EWORKSPACE and call(S=S, reduce=red, ws=base, ws_bytes=need - 1) == EWORKSPACE
        assert call(S=S, reduce=red, ws=base + 4, ws_bytes=need) == EALIGN
    assert call(count=base + 2) == EALIGN and call(reduce=2, arg=base + 4) == EALIGN and call(keys=base + 4) == EALIGN


def test_scatter_backward_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()

    def call(**kw):
        return lib.egnn_scatter_bwd_f32(kw.get("dsrc", base), kw.get("ld_dsrc", 8), kw.get("S", 3), kw.get("index", base), kw.get("n_rows", 4),
                                        kw.get("g", base), kw.get("ld_g", 8), kw.get("C", 8), kw.get("reduce", 0), kw.get("count", None),
                                        kw.get("arg", None), None)
    for red in range(4):
        assert lib.egnn_scatter_bwd_f32(None, 8, 0, None, 4, None, 8, 8, red, None, None, None) == 0               # S == 0, NULL operands
    assert call(reduce=4) == EINVAL and call(reduce=-1) == EINVAL
    assert call(ld_dsrc=7) == EINVAL and call(ld_g=4) == EINVAL and call(C=0) == EINVAL and call(S=-1) == EINVAL
    assert call(dsrc=None) == EINVAL and call(index=None) == EINVAL and call(g=None) == EINVAL
    assert call(reduce=1) == EINVAL and call(reduce=2) == EINVAL and call(reduce=3) == EINVAL        # without count / arg
    assert call(index=base + 4) == EALIGN and call(reduce=1, count=base + 2) == EALIGN and call(reduce=2, arg=base + 4) == EALIGN
    assert lib.egnn_rows_wrap_i64(None, 0, 4, None, None) == 0
    assert lib.egnn_rows_wrap_i64(None, 3, 4, base, None) == EINVAL and lib.egnn_rows_wrap_i64(base + 4, 3, 4, base, None) == EALIGN


def test_message_passing_and_torch_scatter_resolve_through_the_dropin_path():
    names = ("torch_geometric", "torch_scatter")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in names or k.startswith(tuple(n + "." for n in names))}
    sys.path.insert(0, DROPIN)
    try:
        from torch_geometric.nn import MessagePassing
        import torch_scatter
        assert MessagePassing is PN.MessagePassing is P.MessagePassing
        assert torch_scatter.__file__.startswith(DROPIN)
        for fn in ("scatter", "scatter_add", "scatter_mean", "scatter_max", "scatter_min"):
            assert callable(getattr(torch_scatter, fn))
        src, index = torch.zeros(3, 2), torch.tensor([0, 1, 1])
        with pytest.raises(NotImplementedError, match="out"):
            torch_scatter.scatter_add(src, index, 0, out=torch.zeros(2, 2))
        with pytest.raises(NotImplementedError, match="dim"):
            torch_scatter.scatter(src, index, 1, dim_size=2)
        with pytest.raises(NotImplementedError, match="index"):
            torch_scatter.scatter_max(src, index.view(3, 1).expand(3, 2), 0, dim_size=2)
        with pytest.raises(_lib.HipExtensionError):
            torch_scatter.scatter_mean(src, index, 0, dim_size=2)                  # CPU tensors: no fallback
    finally:
        sys.path.remove(DROPIN)
        for k in [k for k in sys.modules if k in names or k.startswith(tuple(n + "." for n in names))]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_constructor_options():
    for aggr in ("add", "sum", "mean", "max", "min"):
        assert PN.MessagePassing(aggr=aggr).aggr == aggr
    with pytest.raises(ValueError, match="aggr"):
        PN.MessagePassing(aggr="median")
    with pytest.raises(ValueError, match="flow"):
        PN.MessagePassing(flow="sideways")
    with pytest.raises(NotImplementedError, match="node_dim"):
        PN.MessagePassing(node_dim=1)
    assert PN.MessagePassing(node_dim=0).node_dim == 0 and PN.MessagePassing(node_dim=-2).node_dim == -2
    assert PN.MessagePassing(flow="target_to_source").flow == "target_to_source"


class _Conv(PN.MessagePassing):
    def __init__(self, **kw):
        super().__init__(aggr="mean", **kw)

    def forward(self, x, edge_index, edge_type):
        return self.propagate(edge_index, x=x, edge_type=edge_type)

    def message(self, x_j, edge_type: int):
        return x_j * float(edge_type)

    def update(self, aggr_out, x):
        return aggr_out + x


def test_parameter_names_are_read_once_per_class():
    a, b = _Conv(), _Conv()
    assert a._mp_params() is b._mp_params()
    assert [n for n, _ in a._mp_params()["message"]] == ["x_j", "edge_type"]
    assert [n for n, _ in a._mp_params()["update"]] == ["x"]
    assert [n for n, _ in a._mp_params()["aggregate"]] == ["index", "ptr", "dim_size"]
    assert PN.MessagePassing()._mp_params() is not a._mp_params()                  # the base class has its own entry


def test_propagate_on_cpu_tensors_raises():
    x, ei = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(_lib.HipExtensionError):
        _Conv()(x, ei, 2)
    with pytest.raises(_lib.HipExtensionError):
        PN.MessagePassing().propagate(ei, x=x)
    with pytest.raises(TypeError, match="edge_index"):
        PN.MessagePassing().propagate(ei.to(torch.int32), x=x)
    with pytest.raises(_lib.HipExtensionError):
        ops.scatter(x[:3], ei[1], 4)
    with pytest.raises(ValueError, match="reduce"):
        ops.scatter(x[:3], ei[1], 4, reduce="median")
    with pytest.raises(ValueError, match="check"):
        ops.rows_plan(ei[1], 4, check="later")
    assert inspect.signature(ops.rows_plan).parameters["check"].default == "host"
