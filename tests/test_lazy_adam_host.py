"""Host checks of the row-lazy Adam (efficient-gnns_amd/optim.py, csrc/adam_rows.hip): the C ABI additions, the option errors and the
host rings of per-step scalars.  No GPU (the kernels themselves: tests/test_gpu_lazy_adam.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import efficient_gnns_amd as E
from efficient_gnns_amd import _lib, optim
from conftest import ROOT

NEW_SYMBOLS = ("egnn_group_input_f32", "egnn_adam_rows_catchup_f32", "egnn_adam_rows_flush_f32", "egnn_adam_rows_step_f32")


def _header():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_is_still_9():
    src = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), f"{s} is not declared in include/egnn_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES and _lib.SIGNATURES[s][0] is ctypes.c_int
    assert re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", src)
    assert _lib.load().egnn_abi_version() == 9
    assert "adam_rows.hip" in __import__("importlib").import_module("efficient_gnns_amd.build").SOURCES
    assert E.LazyRowAdam is optim.LazyRowAdam


def test_adam_rows_descriptor_matches_the_header_field_by_field():
    """egnn_adam_rows_t against _lib.AdamRows: same fields, same order, same kinds; the two rings are float[EGNN_ADAM_MAX_LAG]; every
    taker receives it first, as ``const egnn_adam_rows_t*``."""
    src = _header()
    assert int(re.search(r"#define\s+EGNN_ADAM_MAX_LAG\s+(\d+)", src).group(1)) == _lib.ADAM_MAX_LAG == optim.MAX_LAG == 64
    body = re.search(r"typedef\s+struct\s+egnn_adam_rows\s*\{([^}]*)\}\s*egnn_adam_rows_t\s*;", src).group(1)
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int, "float": ctypes.c_float}
    want = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        m = re.fullmatch(r"(.*?)(\w+)(\[EGNN_ADAM_MAX_LAG\])?", decl, flags=re.S)
        ctype, name, ring = m.group(1).replace("const", "").strip(), m.group(2), m.group(3)
        t = ctypes.c_void_p if ctype.endswith("*") else kinds[ctype]
        want.append((name, t * 64 if ring else t))
    got = list(_lib.AdamRows._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is b or (a._type_ is b._type_ and a._length_ == b._length_)), n
    for s in NEW_SYMBOLS[1:]:
        args = re.search(r"\bint\s+%s\s*\(([^;{]*)\)\s*;" % s, src).group(1).split(",")
        assert re.fullmatch(r"\s*const\s+egnn_adam_rows_t\s*\*\s*\w+\s*", args[0]), s
        assert _lib.SIGNATURES[s][1][0] is ctypes.c_void_p


def test_argument_errors_are_reported_before_any_launch():
    """NULL descriptors / operands and a step that has left the ring are EGNN_EINVAL without a device."""
    lib = _lib.load()
    assert lib.egnn_adam_rows_flush_f32(None, None) == -1
    assert lib.egnn_adam_rows_catchup_f32(None, 0, None, None, 0, None) == -1
    assert lib.egnn_adam_rows_step_f32(None, 0, None, None, 0, None, 0, None) == -1
    assert lib.egnn_group_input_f32(None, None, 1, None, None, 0, 4, None, 4, None, None) == -1
    buf = (ctypes.c_float * 64)()                       # 16-byte aligned stand-ins: nothing is launched on these paths
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.AdamRows()
    d.p = d.m = d.v = d.last = d.dup_count = base
    d.n_rows, d.D, d.ld = 0, 8, 8
    d.step, d.flushed = 70, 6
    assert lib.egnn_adam_rows_flush_f32(ctypes.byref(d), None) == 0             # no rows: nothing to enqueue
    d.flushed = 5                                                               # 65 steps behind: older than the ring
    assert lib.egnn_adam_rows_flush_f32(ctypes.byref(d), None) == -1
    d.flushed, d.D = 6, 6                                                       # D % 4 != 0
    assert lib.egnn_adam_rows_flush_f32(ctypes.byref(d), None) == -1
    d.D, d.ld = 8, 10                                                           # ld % 4 != 0
    assert lib.egnn_adam_rows_flush_f32(ctypes.byref(d), None) == _lib.EGNN_EALIGN


def test_unsupported_options_raise():
    w = torch.nn.Parameter(torch.zeros(4, 8))
    for kw in ({"weight_decay": 0.1}, {"amsgrad": True}, {"maximize": True}, {"capturable": True}):
        with pytest.raises(NotImplementedError):
            E.LazyRowAdam([w], **kw)
    with pytest.raises(NotImplementedError):
        E.LazyRowAdam([{"params": [w], "weight_decay": 0.01}])
    with pytest.raises(ValueError):
        E.LazyRowAdam([w], lazy=[torch.nn.Parameter(torch.zeros(4, 8))])


def test_cpu_parameter_raises():
    w = torch.nn.Parameter(torch.zeros(4, 8))
    with pytest.raises(_lib.HipExtensionError):
        E.LazyRowAdam([w], lazy=[w])
    assert not hasattr(w, "_egnn_rows")
    with pytest.raises(_lib.HipExtensionError):         # a non-lazy CPU parameter too: the inner fused Adam never sees it
        E.LazyRowAdam([w])
    with pytest.raises(_lib.HipExtensionError):
        E._lib.require_gpu(w)
    from efficient_gnns_amd import ops
    with pytest.raises(_lib.HipExtensionError):
        ops.group_input({0: w}, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 8)


def test_ring_entries_are_the_double_scalars_rounded_to_fp32():
    """t = 1..130 with lr 5e-3, then 1e-3 from t = 30: slot t % 64 holds fp32(lr_t / (1 - beta1^t)) and fp32(sqrt(1 - beta2^t)) as
    formed in Python double; a slot is overwritten only 64 steps later."""
    b1, b2 = 0.9, 0.999
    ring = optim.AdamRing(b1, b2)
    want_ss, want_bc = {}, {}
    for t in range(1, 131):
        lr = 5e-3 if t < 30 else 1e-3
        ring.fill(t, lr)
        want_ss[t] = np.float32(lr / (1.0 - b1 ** t))
        want_bc[t] = np.float32(math.sqrt(1.0 - b2 ** t))
        for tau in range(max(1, t - 63), t + 1):
            assert np.float32(ring.step_size[tau % 64]) == want_ss[tau], (t, tau)
            assert np.float32(ring.bc2_sqrt[tau % 64]) == want_bc[tau], (t, tau)
    assert want_ss[29] != want_ss[30] and float(want_ss[130]) == pytest.approx(1e-3, rel=1e-5)
