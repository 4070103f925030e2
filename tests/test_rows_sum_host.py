"""Host checks of the run-sum behind row gathers with repeated ids (csrc/rows_sum.hip, ``ops.rows_plan``, ``duplicates="sum"``): the C ABI
additions against ``_lib.SIGNATURES``, the argument errors that must come back before any launch, the workspace bounds and the option
errors.  No GPU (the kernels themselves: tests/test_gpu_rows_sum.py)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from efficient_gnns_amd import _lib, ops
from conftest import ROOT

EINVAL, EWORKSPACE, EALIGN = -1, -3, _lib.EGNN_EALIGN
NEW = ("egnn_rows_plan_ws_bytes", "egnn_rows_plan_build_i64", "egnn_rows_add_runs_ws_bytes", "egnn_rows_add_runs_f32")
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
    build = __import__("importlib").import_module("efficient_gnns_amd.build")
    assert "rows_sum.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "rows_keys.h"))
    # the key / sort helpers live in the shared key header only, which a file reaches directly or through the run-cut header
    runs = open(os.path.join(build.CSRC, "rows_runs.h")).read()
    assert '#include "rows_keys.h"' in runs and "DeviceRadixSort" not in runs and "int bits_for" not in runs
    for f in ("adam_rows.hip", "rows_sum.hip"):
        text = open(os.path.join(build.CSRC, f)).read()
        assert '#include "rows_keys.h"' in text or '#include "rows_runs.h"' in text
        assert "DeviceRadixSort" not in text and "int bits_for" not in text


def test_the_run_cut_is_defined_in_rows_runs_h_only():
    build = __import__("importlib").import_module("efficient_gnns_amd.build")
    runs = open(os.path.join(build.CSRC, "rows_runs.h")).read()
    assert re.search(r"constexpr int64_t CHUNK = EGNN_ROWS_SUM_CHUNK;", runs)     # the chunk is the header's, not a number of its own
    assert "atomic" not in runs                                                   # nothing shared reads-modifies-writes memory
    shared = ("lower_bound", "row_has_run", "is_run_head", "chunk_start", "chunk_is_long", "chunk_limit", "long_run_head", "run_chunks",
              "part_slot", "part_slots", "part_pitch", "sizes_ok", "blocks_for", "key_usable", "fold_chunk4", "load_w", "store_w")
    defines = lambda name, text: re.search(r"^[^/\n]*[\w>&*]\s+" + name + r"\s*\([^;{]*\)\s*\{", text, flags=re.M)  # noqa: E731
    for name in shared:
        assert defines(name, runs), f"rows_runs.h does not define {name}"
    for f in ("rows_sum.hip", "scatter.hip", "scatter_softmax.hip", "adam_rows.hip"):
        text = open(os.path.join(build.CSRC, f)).read()
        assert '#include "rows_runs.h"' in text
        for name in shared:
            assert not defines(name, text), f"{f} defines {name} again"
        assert "EGNN_ROWS_SUM_CHUNK;" not in text and "% CHUNK" not in text and "sorted[j - 1]" not in text   # no cut written out again


def test_plan_workspace_is_monotone_in_the_list():
    lib = _lib.load()
    sizes = [lib.egnn_rows_plan_ws_bytes(S, 170_000) for S in (0, 1, 2, 1000, 65_536, 1_000_000, 2_500_000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] >= 8 * 2_500_000                                            # at least the unsorted key array
    chunk = _chunk()
    assert lib.egnn_rows_add_runs_ws_bytes(chunk, 256) == 0                      # no run can be longer than one chunk
    part = [lib.egnn_rows_add_runs_ws_bytes(S, 256) for S in (chunk + 1, 10 * chunk, 1_000_000)]
    assert all(a <= b for a, b in zip(part, part[1:])) and part[0] > 0
    assert part[-1] <= 1_000_000 * 256 * 4 // 32                                 # two partial rows per chunk of entries


def _buf():
    keep = (ctypes.c_float * 64)()                       # a 16-byte aligned stand-in: nothing is launched on these paths
    return (ctypes.addressof(keep) + 15) & ~15, keep


def test_plan_build_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    call = lambda **kw: lib.egnn_rows_plan_build_i64(kw.get("idx", base), kw.get("S", 3), kw.get("n_rows", 4), kw.get("keys", base),  # noqa: E731
                                                     kw.get("counters", base), kw.get("ws", base), kw.get("ws_bytes", 1 << 20), None)
    assert lib.egnn_rows_plan_build_i64(None, 0, 4, None, None, None, 0, None) == 0      # S == 0: nothing to enqueue
    assert call(idx=None) == EINVAL and call(keys=None) == EINVAL and call(counters=None) == EINVAL
    assert call(S=-1) == EINVAL and call(n_rows=-1) == EINVAL
    assert call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL   # row and position share one 64-bit key
    need = lib.egnn_rows_plan_ws_bytes(3, 4)
    assert call(ws=None, ws_bytes=need) == EWORKSPACE and call(ws_bytes=need - 1) == EWORKSPACE
    assert call(ws=base + 4, ws_bytes=need) == EALIGN


def test_add_runs_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    chunk = _chunk()

    def call(**kw):
        S = kw.get("S", 3)
        shift = kw.get("shift", max(1, (S - 1).bit_length()))
        return lib.egnn_rows_add_runs_f32(kw.get("dst", base), kw.get("ld_dst", 8), kw.get("n_rows", 4), kw.get("keys", base), S, shift,
                                          kw.get("src", base), kw.get("ld_src", 8), kw.get("C", 8), kw.get("accumulate", 1),
                                          kw.get("ws", None), kw.get("ws_bytes", 0), None)
    for acc in (0, 1):
        assert lib.egnn_rows_add_runs_f32(None, 8, 4, None, 0, 0, None, 8, 8, acc, None, 0, None) == 0   # S == 0 with null buffers
    assert call(dst=None) == EINVAL and call(keys=None) == EINVAL and call(src=None) == EINVAL
    assert call(C=0) == EINVAL and call(C=-4) == EINVAL
    assert call(ld_dst=4) == EINVAL and call(ld_src=7) == EINVAL
    assert call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL and call(S=-1) == EINVAL
    assert call(shift=5) == EINVAL and call(accumulate=2) == EINVAL
    S = 3 * chunk + 5                                                             # long enough for a run of several chunks
    need = lib.egnn_rows_add_runs_ws_bytes(S, 8)
    assert need > 0
    assert call(S=S, ws=None, ws_bytes=need) == EWORKSPACE and call(S=S, ws=base, ws_bytes=need - 1) == EWORKSPACE
    assert call(S=S, ws=base + 4, ws_bytes=need) == EALIGN


def test_duplicates_option_takes_the_two_values_only():
    x, idx = torch.zeros(4, 8), torch.tensor([0, 1])
    w = torch.zeros(3, 8)
    for bad in ("bogus", "", None, True):
        with pytest.raises(ValueError, match="duplicates"):
            ops.take_rows(x, idx, duplicates=bad)
        with pytest.raises(ValueError, match="duplicates"):
            ops.linear_rows(x, idx, w, duplicates=bad)
        with pytest.raises(ValueError, match="duplicates"):
            ops.gather_normalize(x, idx, duplicates=bad)
    for fn in (ops.take_rows, ops.linear_rows, ops.gather_normalize):
        assert inspect.signature(fn).parameters["duplicates"].default == "unique"


def test_a_plan_is_not_built_during_a_graph_capture(monkeypatch):
    """The plan reads its counters on the host: under a capture the builder raises before it enqueues or reads anything."""
    monkeypatch.setattr(torch.cuda.graphs, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
    idx = torch.tensor([0, 1, 1])
    before = len(ops._ROWS_PLANS)
    with pytest.raises(RuntimeError, match="captur"):
        ops.rows_plan(idx, 4)
    assert len(ops._ROWS_PLANS) == before
