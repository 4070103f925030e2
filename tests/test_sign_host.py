"""CPU-side checks of the SIGN student: the C ABI additions (prototypes + egnn_sign_seg_t against their ctypes mirrors), the model's
state_dict against the reference's (tests/golden/sign.npz), argument handling, and the golden generator's reproducibility."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import efficient_gnns_amd.models as M
from efficient_gnns_amd import _lib, build, ops
from conftest import GOLDEN, ROOT

REFERENCE = "/root/reference"
NEW = ("egnn_sign_gather_drop_f32", "egnn_prelu_drop_fwd_f32", "egnn_prelu_drop_ws_floats", "egnn_prelu_drop_bwd_f32")
KINDS = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "uint64_t": C.c_uint64, "size_t": C.c_size_t}


@pytest.fixture(scope="module")
def golden_sign():
    return np.load(os.path.join(GOLDEN, "sign.npz"), allow_pickle=False)


def header():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def ctype_of(decl):
    """The ctypes class of one C parameter / field declaration: any pointer is c_void_p, scalars by name."""
    d = decl.strip()
    if "*" in d:
        return C.c_void_p
    return KINDS[re.sub(r"\bconst\b", "", d).split()[0]]


def test_new_prototypes_match_the_ctypes_table_argument_by_argument():
    src = header()
    for name in NEW:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^;{]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/egnn_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is {"int": C.c_int, "size_t": C.c_size_t}[m.group(1)], name
        assert [ctype_of(a) for a in m.group(2).split(",")] == list(argtypes), name
        if name != "egnn_prelu_drop_ws_floats":
            first = m.group(2).split(",")[0]
            assert re.fullmatch(r"\s*const\s+egnn_sign_seg_t\s*\*\s*\w+\s*", first), f"{name}: {first}"
    assert "sign.hip" in build.SOURCES


def test_sign_descriptor_matches_the_header_field_by_field():
    body = re.search(r"typedef\s+struct\s+egnn_sign_seg\s*\{([^}]*)\}\s*egnn_sign_seg_t\s*;", header()).group(1)
    want = []
    for d in (d.strip() for d in body.split(";")):
        if d:
            m = re.match(r"(.*?)(\w+)$", d, flags=re.S)
            want.append((m.group(2), ctype_of(m.group(1))))
    assert want == list(_lib.SignSeg._fields_)
    assert all(t in (C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_uint64) for _, t in want)


def test_abi_version_is_still_9():
    assert re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", open(os.path.join(ROOT, "include", "egnn_hip.h")).read())
    assert _lib.load().egnn_abi_version() == 9


def test_too_many_segments_is_an_argument_error_on_the_host():
    """H = 17 is refused by the entry points before anything touches a device (no GPU needed: no launch happens)."""
    lib = _lib.load()
    d = _lib.SignSeg()
    d.B, d.Cs, d.H, d.p = 4, 4, 17, 0.0
    one = C.c_float(0.25)
    slopes = (C.c_void_p * 17)(*[C.addressof(one)] * 17)
    d.slope = C.addressof(slopes)
    buf = (C.c_float * 4 * 68)()
    assert lib.egnn_prelu_drop_fwd_f32(C.byref(d), C.addressof(buf), 68, C.addressof(buf), 68, None) == -1
    assert lib.egnn_prelu_drop_ws_floats(4, 4, 17) == 0
    assert lib.egnn_prelu_drop_fwd_f32(None, C.addressof(buf), 68, C.addressof(buf), 68, None) == -1


@pytest.mark.parametrize("L", [1, 2, 3])
def test_state_dict_equals_the_reference(golden_sign, L):
    G = golden_sign
    torch.manual_seed(40 + L)
    model = M.SIGN(12, 16, 5, 3, L, 0.5, 0.1)
    pre = f"L{L}__init__"
    want = {k[len(pre):]: G[k] for k in G.files if k.startswith(pre)}
    sd = model.state_dict()
    assert list(sd.keys()) == [k for k in sd.keys() if k in want] and set(sd.keys()) == set(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k].shape, k
        assert np.array_equal(v.numpy(), want[k]), k
    assert ("prelu.weight" in sd) and (("project.prelu.weight" in sd) == (L > 1))
    assert float(sd["prelu.weight"]) == 0.25


def test_projection_heads_equal_the_reference(golden_sign):
    G = golden_sign
    torch.manual_seed(40 + 10 + 5)            # the nce epoch of the generator: model, then the two heads
    M.SIGN(12, 16, 5, 3, 2, 0.5, 0.1)
    sp, tp = M.make_sign_projections(16, 3, 8, teacher_dim=17)
    for name, head in (("sproj", sp), ("tproj", tp)):
        for k, v in head.state_dict().items():
            assert np.array_equal(v.numpy(), G[f"kda_nce__init__{name}.{k}"]), (name, k)


def test_unknown_mode_is_rejected():
    model = M.SIGN(12, 16, 5, 3, 2, 0.5, 0.1)
    with pytest.raises(NotImplementedError, match="lpw"):
        M.sign_train_epoch(model, [torch.zeros(4, 12)] * 3, torch.zeros(4, dtype=torch.int64), None, [], "lpw", {})


def test_out_keyword_defaults():
    for fn in (ops.gemm_raw, ops.matmul, ops.linear):
        assert inspect.signature(fn).parameters["out"].default is None


def test_host_tensors_are_refused():
    model = M.SIGN(12, 16, 5, 3, 2, 0.5, 0.1)
    with pytest.raises(_lib.HipExtensionError):
        model([torch.zeros(4, 12)] * 3)
    with pytest.raises(_lib.HipExtensionError):
        ops.prelu_drop(torch.zeros(4, 8), [torch.zeros(1)], 8, 0.0, False)
    with pytest.raises(_lib.HipExtensionError):
        ops.sign_gather_drop([torch.zeros(4, 8)], torch.zeros(2, dtype=torch.int64), 0.0, False)


def test_golden_generator_reproduces_sign_npz_bit_for_bit(tmp_path):
    if not os.path.isdir(REFERENCE):
        pytest.skip("the reference checkout is not on this machine")
    script = os.path.join(GOLDEN, "make_golden_sign.py")
    subprocess.run([sys.executable, script, "--out", str(tmp_path)], check=True, capture_output=True, timeout=300)
    assert open(tmp_path / "sign.npz", "rb").read() == open(os.path.join(GOLDEN, "sign.npz"), "rb").read()
