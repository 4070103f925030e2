"""Host checks of the fused gather-weight-aggregate path (csrc/gather_scatter.hip, ``ops.gather_scatter``, ``lazy.LazyWeightedRows``): the C
ABI additions against ``_lib.SIGNATURES``, the argument errors that must come back before any launch, and which multiplies of a
``lazy.LazyRows`` stay deferred.  No GPU (the kernels themselves: tests/test_gpu_gather_scatter.py)."""
import ctypes
import importlib
import os
import re

import pytest
import torch

from efficient_gnns_amd import _lib, lazy, ops
from efficient_gnns_amd import nn as PN
from conftest import ROOT

EINVAL, EWORKSPACE, EALIGN = -1, -3, _lib.EGNN_EALIGN
NEW = ("egnn_gather_scatter_ws_bytes", "egnn_gather_scatter_runs_f32", "egnn_edge_dot_f32")
CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}


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
    assert "gather_scatter.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gather_scatter.hip"))
    text = open(os.path.join(build.CSRC, "gather_scatter.hip")).read()
    code = text.split("namespace {", 1)[1]
    assert '#include "rows_runs.h"' in text and "atomic" not in code                # no atomics of any kind in the code
    for shared in ("chunk_start(", "chunk_is_long(", "part_slot(", "long_run_head(", "run_chunks(", "key_usable("):
        assert shared in code, shared                                              # the cut and the slots are the shared header's
    assert "int64_t lower_bound" not in text and "int64_t part_slot" not in text
    # the new prototypes are appended: nothing is declared after them
    names = re.findall(r"\b(?:int|size_t|int64_t)\s+(egnn_\w+)\s*\(", _header())
    assert tuple(names[-3:]) == NEW


def _buf():
    keep = (ctypes.c_float * 64)()                       # a 16-byte aligned stand-in: nothing is launched on these paths
    return (ctypes.addressof(keep) + 15) & ~15, keep


def test_workspace_size_is_the_run_sums():
    lib, chunk = _lib.load(), _chunk()
    assert lib.egnn_gather_scatter_ws_bytes(0, 256) == 0 and lib.egnn_gather_scatter_ws_bytes(chunk, 256) == 0
    for S in (chunk + 1, 10 * chunk, 1_000_000):
        for C in (1, 40, 260):
            assert lib.egnn_gather_scatter_ws_bytes(S, C) == lib.egnn_rows_add_runs_ws_bytes(S, C) > 0
    assert lib.egnn_gather_scatter_ws_bytes(10 * chunk, 0) == 0


def test_gather_scatter_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    chunk = _chunk()

    def call(**kw):
        S = kw.get("S", 3)
        shift = kw.get("shift", max(1, (S - 1).bit_length()))
        return lib.egnn_gather_scatter_runs_f32(kw.get("out", base), kw.get("ld_out", 8), kw.get("n_rows", 4), kw.get("count", base),
                                                kw.get("keys", base), S, shift, kw.get("frm", base), kw.get("x", base), kw.get("ld_x", 8),
                                                kw.get("n_x", 5), kw.get("from_count", None), kw.get("w", base), kw.get("ld_w", 2),
                                                kw.get("H", 2), kw.get("C", 8), kw.get("reduce", 0), kw.get("ws", None), kw.get("ws_bytes", 0),
                                                None)
    for red in (0, 1):
        assert lib.egnn_gather_scatter_runs_f32(None, 8, 4, None, None, 0, 0, None, None, 8, 5, None, None, 0, 1, 8, red, None, 0, None) == 0
    assert call(reduce=2) == EINVAL and call(reduce=3) == EINVAL and call(reduce=-1) == EINVAL       # max / min stay with egnn_scatter_runs_f32
    assert call(ld_out=7) == EINVAL and call(ld_x=4) == EINVAL and call(C=0) == EINVAL and call(n_x=-1) == EINVAL
    assert call(H=0) == EINVAL and call(H=3, ld_w=3) == EINVAL and call(ld_w=1) == EINVAL             # H divides C, the pitch holds H
    assert call(w=None, H=2) == EINVAL                                              # heads without weights
    assert lib.egnn_gather_scatter_runs_f32(None, 8, 4, None, None, 0, 0, None, None, 8, 5, None, None, 2, 2, 8, 0, None, 0, None) == 0   # no edge: no weight
    assert call(out=None) == EINVAL and call(keys=None) == EINVAL and call(frm=None) == EINVAL and call(x=None) == EINVAL
    assert call(S=-1) == EINVAL and call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL and call(shift=5) == EINVAL
    assert call(reduce=1, count=None) == EINVAL                                     # mean needs the counts
    S = 3 * chunk + 5
    need = lib.egnn_gather_scatter_ws_bytes(S, 8)
    assert need > 0
    assert call(S=S, ws=None, ws_bytes=need) == EWORKSPACE and call(S=S, ws=base, ws_bytes=need - 1) == EWORKSPACE
    assert call(S=S, ws=base + 4, ws_bytes=need) == EALIGN
    assert call(keys=base + 4) == EALIGN and call(frm=base + 4) == EALIGN and call(count=base + 2) == EALIGN
    assert call(from_count=base + 2) == EALIGN and call(x=base + 2) == EALIGN


def test_edge_dot_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()

    def call(**kw):
        return lib.egnn_edge_dot_f32(kw.get("dw", base), kw.get("ld_dw", 2), kw.get("S", 3), kw.get("H", 2), kw.get("C", 8),
                                     kw.get("a_rows", base), kw.get("A", base), kw.get("ld_a", 8), kw.get("n_a", 4), kw.get("b_rows", base),
                                     kw.get("B", base), kw.get("ld_b", 8), kw.get("n_b", 5), kw.get("a_count", None), None)
    assert lib.egnn_edge_dot_f32(None, 1, 0, 1, 8, None, None, 8, 4, None, None, 8, 5, None, None) == 0                   # S == 0
    assert call(S=-1) == EINVAL and call(C=0) == EINVAL and call(H=0) == EINVAL and call(H=3, ld_dw=3) == EINVAL
    assert call(ld_dw=1) == EINVAL and call(ld_a=7) == EINVAL and call(ld_b=7) == EINVAL and call(n_a=-1) == EINVAL
    assert call(dw=None) == EINVAL and call(a_rows=None) == EINVAL and call(b_rows=None) == EINVAL and call(A=None) == EINVAL
    assert call(a_rows=base + 4) == EALIGN and call(b_rows=base + 4) == EALIGN and call(a_count=base + 2) == EALIGN


# ------------------------------------------------------------------------------------------------
# ops.gather_scatter: what is refused before any plan is built or kernel called
# ------------------------------------------------------------------------------------------------
def _no_kernels(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a kernel path was reached")
    monkeypatch.setattr(ops._GatherScatter, "apply", boom)
    monkeypatch.setattr(ops, "_rows_plan_launch", boom)


def test_python_argument_errors_come_first(monkeypatch):
    _no_kernels(monkeypatch)
    x = torch.zeros(5, 8)
    src, dst = torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)
    for red in ("max", "min"):
        with pytest.raises(ValueError, match="ops.scatter"):
            ops.gather_scatter(x, src, dst, 4, reduce=red)
    with pytest.raises(ValueError, match="reduce"):
        ops.gather_scatter(x, src, dst, 4, reduce="prod")
    with pytest.raises(ValueError, match="heads"):
        ops.gather_scatter(x, src, dst, 4, weight=torch.zeros(6, 3))                # 3 does not divide 8
    with pytest.raises(ValueError, match="heads"):
        ops.gather_scatter(torch.zeros(5, 2, 4), src, dst, 4, weight=torch.zeros(6, 4))    # divides 8, but x has 2 heads
    with pytest.raises(ValueError, match="weights for 6 edges"):
        ops.gather_scatter(x, src, dst, 4, weight=torch.zeros(7))
    with pytest.raises(ValueError, match="weight"):
        ops.gather_scatter(x, src, dst, 4, weight=torch.zeros(6, 2, 2))
    with pytest.raises(TypeError):
        ops.gather_scatter(x.double(), src, dst, 4)
    with pytest.raises(ValueError, match="source ids"):
        ops.gather_scatter(x, src, dst[:5], 4)
    plan_src = ops.RowsPlan(src, 5, 6)
    plan_dst = ops.RowsPlan(dst, 4, 6)
    with pytest.raises(ValueError, match="built for 4 rows"):
        ops.gather_scatter(x, plan_src, plan_dst, 9)                                # plan / dim_size mismatch
    with pytest.raises(ValueError, match="built for 5 rows"):
        ops.gather_scatter(torch.zeros(7, 8), plan_src, plan_dst, 4)
    with pytest.raises(_lib.HipExtensionError):
        ops.gather_scatter(x, plan_src, plan_dst, 4)                                # everything fits: refused as a CPU tensor, no fallback


def test_running_end_plan_matches_either_endpoint():
    ei = torch.zeros(2, 3, dtype=torch.int64)
    call = PN._Propagation((ei[0], ei[1]), [None, None])
    call.plans = ["source plan", "target plan"]                                     # (built elsewhere: nothing is launched here)
    PN._MP_RUNNING.append((call, 1))
    try:
        ends = call.ends
        assert PN.running_end_plan(ends[0], 5, "src") == "source plan" and PN.running_end_plan(ends[1], 4, "dst") == "target plan"
        assert call.size == [5, 4]
        assert PN.running_end_plan(ei[0], 5) is None                                # another tensor object: identity, not value
        with pytest.raises(ValueError):
            PN.running_end_plan(ends[0], 6, "src")                                  # the call has settled on 5 nodes
        assert PN.running_plan(ends[0]) is None                                     # (the target-side helper is as it was)
    finally:
        PN._MP_RUNNING.pop()


# ------------------------------------------------------------------------------------------------
# lazy.LazyRows * weight
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    """CPU tensors stand in for the device's: the shape rules are what is under test."""
    monkeypatch.setattr(lazy, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ops, "FUSE_LAZY_ROWS", True)
    calls = []

    def gather_scatter(x, src, dst, dim_size, weight=None, reduce="sum"):
        calls.append((x, src, dst, dim_size, weight, reduce))
        return "fused"
    monkeypatch.setattr(ops, "gather_scatter", gather_scatter)
    return calls


def test_lazy_rows_times_a_per_edge_weight_stays_deferred(stubbed):
    E = 6
    idx = torch.tensor([0, 2, 2, 1, 4, 0])
    x2, x3 = torch.randn(5, 8), torch.randn(5, 2, 4)
    accepted = ((x2, torch.randn(E, 1)), (x2, torch.tensor(0.5)), (x2, 2.0), (x2, 3), (x3, torch.randn(E, 2, 1)), (x3, torch.randn(E, 1, 1)),
                (x3, torch.tensor(0.5)), (x2, torch.nn.Parameter(torch.randn(E, 1))))
    for base, w in accepted:
        for spell in (lambda r, w: r * w, lambda r, w: w * r, lambda r, w: torch.mul(r, w), lambda r, w: torch.mul(w, r)):
            rows = lazy.LazyRows(base, idx)
            try:
                got = spell(rows, w)
            except TypeError:
                assert not isinstance(w, torch.Tensor)                              # torch.mul(3, rows): torch refuses a number first
                continue
            assert isinstance(got, lazy.LazyWeightedRows) and rows._value is None, (base.shape, w)
            assert tuple(got.shape) == (E,) + tuple(base.shape[1:])
            assert torch.equal(lazy.materialise(got), base[idx] * w)               # every other consumer: exactly take_rows(...) * w
    rejected = ((x2, torch.randn(E)), (x2, torch.randn(E, 8)), (x2, torch.randn(1, 8)), (x2, torch.randn(E, 1).double()), (x3, torch.randn(E, 1)),
                (x3, torch.randn(E, 2, 4)), (x3, torch.randn(2, 1)), (x2, True))
    for base, w in rejected:
        rows = lazy.LazyRows(base, idx)
        try:
            got = rows * w
        except RuntimeError:
            got = None                                                              # shapes torch does not broadcast raise as torch does
        assert not isinstance(got, lazy._TensorLike) and rows._value is not None, (base.shape, getattr(w, "shape", w))
        if got is not None:
            assert torch.equal(got, base[idx] * w)
    formed = lazy.LazyRows(x2, idx)
    lazy.materialise(formed)
    assert isinstance(formed * torch.randn(E, 1), torch.Tensor)                     # rows that exist already
    twice = lazy.LazyRows(x2, idx) * torch.randn(E, 1)
    assert isinstance(twice * torch.randn(E, 1), torch.Tensor)                      # a second per-edge weight materialises
    assert isinstance(lazy.LazyRows(x2, idx) + torch.randn(E, 1), torch.Tensor)     # any other operator too


def test_scatter_hands_unformed_rows_to_gather_scatter(stubbed):
    E = 6
    idx, index = torch.tensor([0, 2, 2, 1, 4, 0]), torch.tensor([1, 1, 0, 3, 3, 3])
    x2, x3 = torch.randn(5, 8), torch.randn(5, 2, 4)
    plan = lambda: "the call's plan"                                                # noqa: E731
    w = torch.randn(E, 1)
    assert ops.scatter(lazy.LazyRows(x2, idx, plan=plan), index, 4, "mean") == "fused"
    assert stubbed[-1][0] is x2 and stubbed[-1][1:4] == ("the call's plan", index, 4) and stubbed[-1][4] is None and stubbed[-1][5] == "mean"
    assert ops.scatter(lazy.LazyRows(x2, idx) * w, index, 4, "add", plan="dst plan") == "fused"
    assert stubbed[-1][1] is idx and stubbed[-1][2] == "dst plan" and stubbed[-1][4] is w and stubbed[-1][5] == "add"
    w3 = torch.randn(E, 2, 1)
    assert ops.scatter(lazy.LazyRows(x3, idx) * w3, index, 4) == "fused" and stubbed[-1][4] is w3
    assert ops.scatter(lazy.LazyRows(x3, idx) * torch.ones(E, 1, 1), index, 4) == "fused" and tuple(stubbed[-1][4].shape) == (E,)
    assert ops.scatter(lazy.LazyRows(x2, idx) * 2.0, index, 4) == "fused" and torch.equal(stubbed[-1][4], torch.full((E,), 2.0))
    out, arg = ops.scatter(lazy.LazyRows(x2, idx), index, 4, return_arg=True)
    assert out == "fused" and arg is None
    n = len(stubbed)
    x2.add_(1.0)                                                                    # the base changed after the rows were asked for
    stale = lazy.LazyRows(x2, idx, base_version=x2._version - 1)
    with pytest.raises(RuntimeError, match="inplace"):
        ops.scatter(stale * w, index, 4)
    for red in ("max", "min"):                                                      # these materialise (and then need the device)
        with pytest.raises(_lib.HipExtensionError):
            ops.scatter(lazy.LazyRows(x2, idx) * w, index, 4, red)
    assert len(stubbed) == n
