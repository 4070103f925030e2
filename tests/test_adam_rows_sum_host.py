"""Host checks of the summing row step (egnn_adam_rows_step_sum_f32, csrc/adam_rows.hip) and ``LazyRowAdam(duplicates=...)``: the two
C ABI additions, the argument errors that must come back before any launch, the workspace bound and the option errors.  No GPU (the
kernel itself: tests/test_gpu_adam_rows_sum.py)."""
import ctypes
import os
import re

import pytest
import torch

import efficient_gnns_amd as E
from efficient_gnns_amd import _lib
from conftest import ROOT

EINVAL, EWORKSPACE = -1, -3


def _header():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_the_two_symbols_are_declared_exported_and_bound_and_the_abi_is_still_9():
    src = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+egnn_adam_rows_step_sum_ws_bytes\s*\(\s*int64_t\s+n\s*,\s*int64_t\s+n_rows\s*\)\s*;", src)
    args = re.search(r"\bint\s+egnn_adam_rows_step_sum_f32\s*\(([^;{]*)\)\s*;", src).group(1).split(",")
    assert len(args) == 11 and re.fullmatch(r"\s*const\s+egnn_adam_rows_t\s*\*\s*\w+\s*", args[0])
    assert re.fullmatch(r"\s*float\s+scale\s*", args[7])
    for s, res, n_args in (("egnn_adam_rows_step_sum_ws_bytes", ctypes.c_size_t, 2), ("egnn_adam_rows_step_sum_f32", ctypes.c_int, 11)):
        assert hasattr(lib, s), f"{s} is not exported"
        assert _lib.SIGNATURES[s][0] is res and len(_lib.SIGNATURES[s][1]) == n_args
    assert _lib.SIGNATURES["egnn_adam_rows_step_sum_f32"][1][7] is ctypes.c_float
    assert re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", src)
    assert _lib.load().egnn_abi_version() == 9
    assert int(re.search(r"#define\s+EGNN_EWORKSPACE\s+\((-?\d+)\)", src).group(1)) == EWORKSPACE


def _descriptor():
    buf = (ctypes.c_float * 64)()                       # 16-byte aligned stand-ins: nothing is launched on these paths
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.AdamRows()
    d.p = d.m = d.v = d.last = d.dup_count = base
    d.n_rows, d.D, d.ld = 4, 8, 8
    d.step, d.flushed = 70, 6
    return d, base, buf


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    call = lib.egnn_adam_rows_step_sum_f32
    assert call(None, 0, None, None, 0, None, 0, 1.0, None, 0, None) == EINVAL
    d, base, keep = _descriptor()
    ok = lambda **kw: call(ctypes.byref(d), 0, None, kw.get("idx", base), kw.get("n", 0), kw.get("g", base), kw.get("ldg", 8), 1.0,  # noqa: E731
                           kw.get("ws", None), kw.get("ws_bytes", 0), None)
    assert ok() == 0                                                            # n == 0: nothing to enqueue, no workspace needed
    assert ok(idx=None) == EINVAL and ok(g=None) == EINVAL and ok(n=-1) == EINVAL and ok(ldg=4) == EINVAL
    assert ok(g=base + 4) == _lib.EGNN_EALIGN and ok(ldg=10) == _lib.EGNN_EALIGN
    assert ok(n=2 ** 31) == EINVAL                                              # row and entry share one 64-bit key
    need = lib.egnn_adam_rows_step_sum_ws_bytes(3, 4)
    assert ok(n=3, ws=None, ws_bytes=need) == EWORKSPACE                        # a workspace that is missing or too small
    assert ok(n=3, ws=base, ws_bytes=need - 1) == EWORKSPACE
    assert ok(n=3, ws=base + 4, ws_bytes=need) == _lib.EGNN_EALIGN
    d.D = 6                                                                     # D % 4 != 0
    assert ok() == EINVAL
    d.D, d.ld = 8, 10                                                           # ld % 4 != 0
    assert ok() == _lib.EGNN_EALIGN
    d.ld, d.p = 8, base + 4                                                     # a misaligned table
    assert ok() == _lib.EGNN_EALIGN
    d.p, d.step = base, 0                                                       # a step needs step >= 1
    assert ok() == EINVAL
    d.step, d.flushed = 70, 5                                                   # older than the ring
    assert ok() == EINVAL


@pytest.mark.parametrize("n", [0, 1, 55_000, 500_000])
def test_workspace_is_linear_in_the_list_and_independent_of_the_table(n):
    """Two arrays of n 64-bit keys and the radix sort's temporary storage (a third key array, histograms): at most 32 bytes per entry
    plus 1 MiB; the table (1.2 M x 128: 588 MiB) does not enter."""
    lib = _lib.load()
    got = lib.egnn_adam_rows_step_sum_ws_bytes(n, 1_200_000)
    assert 16 * n <= got <= 32 * n + (1 << 20), got
    assert got < 1_200_000 * 128 * 4 // 8


def test_duplicates_option_takes_the_two_values_only():
    w = torch.nn.Parameter(torch.zeros(4, 8))
    for bad in ("add", "", None, True):
        with pytest.raises(ValueError, match="duplicates"):
            E.LazyRowAdam([w], duplicates=bad)
    import inspect
    import efficient_gnns_amd.models as PM
    assert inspect.signature(E.LazyRowAdam.__init__).parameters["duplicates"].default == "refuse"
    assert inspect.signature(PM.mag_optimizer).parameters["duplicates"].default == "refuse"
