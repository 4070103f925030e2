"""CPU-side checks of kernel (RBF) CKA (efficient-gnns_amd/similarity.py, csrc/similarity.hip): the four C ABI additions are declared,
exported and bound; the workspace sizes and their O(N) bound; the entry points' argument checks, which need no GPU; the public
functions refuse CPU tensors; the default ``representation_similarity`` keeps its three keys."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import efficient_gnns_amd as E
import efficient_gnns_amd.models as M
import efficient_gnns_amd.similarity as S
from efficient_gnns_amd import _lib
from conftest import ROOT

NEW = ("egnn_sqdist_median_ws_bytes", "egnn_sqdist_median_f32", "egnn_rbf_cka_ws_bytes", "egnn_rbf_cka_f32")
KINDS = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}
HIST = 3 * 2 * 2048 * 8          # three passes, two selections, 2048 64-bit bins
SIZES = (2, 128, 129, 641, 29_799, 169_343)


def header(strip_comments=True):
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S) if strip_comments else src


def ctype_of(decl):
    d = decl.strip()
    return C.c_void_p if "*" in d else KINDS[re.sub(r"\bconst\b", "", d).split()[0]]


def tiles(N):
    T = (N + 127) // 128
    return T * (T + 1) // 2


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_is_9():
    src, lib = header(), _lib.load()
    for name in NEW:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^;{]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/egnn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is {"int": C.c_int, "size_t": C.c_size_t}[m.group(1)], name
        assert [ctype_of(a) for a in m.group(2).split(",")] == list(argtypes), name
    assert lib.egnn_abi_version() == 9 and re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", src)
    whole = header(strip_comments=False)
    for cite in ("correlation.py:41-53", ":70-75", "correlation.py:45-46"):
        assert cite in whole, f"the header cites the reference lines ({cite})"


@pytest.mark.parametrize("N", SIZES)
def test_workspace_sizes(N):
    lib = _lib.load()
    assert lib.egnn_sqdist_median_ws_bytes(N) == HIST + 24 + (4 * N + 7) // 8 * 8
    chunks = min((N + 127) // 128, 16)
    doubles = 2 * chunks * N + 2 * N + 2 + 2 * ((N + 255) // 256) + 3 * tiles(N)      # row-sum slabs, means, their sums, partials
    assert lib.egnn_rbf_cka_ws_bytes(N) == 8 * doubles + 8 * N                        # ... and two fp32 norm vectors
    assert lib.egnn_sqdist_median_ws_bytes(0) == 0 and lib.egnn_rbf_cka_ws_bytes(0) == 0


@pytest.mark.parametrize("N", [29_799, 169_343])
def test_workspace_is_linear_in_n_at_full_size(N):
    """No per-tile row vector, let alone an N x N object: O(N) doubles with a small constant, three doubles per upper tile."""
    lib = _lib.load()
    cap = 64 * N * 8 + tiles(N) * 3 * 8 + HIST
    assert lib.egnn_rbf_cka_ws_bytes(N) < cap
    assert lib.egnn_sqdist_median_ws_bytes(N) < cap
    assert lib.egnn_rbf_cka_ws_bytes(N) + 2 * lib.egnn_sqdist_median_ws_bytes(N) < N * N * 4


def test_entry_points_reject_bad_arguments_before_any_launch():
    """Negative codes for N < 2, a leading dimension below the width, null pointers, a short workspace and misaligned float64
    arguments; callable without a GPU (nothing is launched and no pointer is followed)."""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    big = 1 << 24
    med, cka = lib.egnn_sqdist_median_f32, lib.egnn_rbf_cka_f32
    assert med(p, 8, 8, 1, p, p, big, None) == -1
    assert med(p, 7, 8, 4, p, p, big, None) == -1
    assert med(p, 8, 0, 4, p, p, big, None) == -1
    assert med(None, 8, 8, 4, p, p, big, None) == -1
    assert med(p, 8, 8, 4, None, p, big, None) == -1
    assert med(p, 8, 8, 4, p, None, big, None) == -1
    assert med(p, 8, 8, 4, p, p, lib.egnn_sqdist_median_ws_bytes(4) - 1, None) == -3
    assert med(p, 8, 8, 4, p + 4, p, big, None) == -1
    assert med(p, 8, 8, 4, p, p + 4, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 1, p, p, p, big, None) == -1
    assert cka(p, 7, 8, p, 8, 8, 4, p, p, p, big, None) == -1
    assert cka(p, 8, 8, p, 7, 8, 4, p, p, p, big, None) == -1
    assert cka(None, 8, 8, p, 8, 8, 4, p, p, p, big, None) == -1
    assert cka(p, 8, 8, None, 8, 8, 4, p, p, p, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 4, None, p, p, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 4, p, None, p, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 4, p, p, None, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 4, p, p, p, lib.egnn_rbf_cka_ws_bytes(4) - 1, None) == -3
    assert cka(p, 8, 8, p, 8, 8, 129, p, p, p, lib.egnn_rbf_cka_ws_bytes(128), None) == -3
    assert cka(p, 8, 8, p, 8, 8, 4, p + 4, p, p, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 4, p, p + 4, p, big, None) == -1
    assert cka(p, 8, 8, p, 8, 8, 4, p, p, p + 4, big, None) == -1


def test_public_functions_exist_and_refuse_cpu_tensors():
    for name in ("kernel_cka", "rbf_bandwidth"):
        assert getattr(E, name) is getattr(S, name), name
    g = torch.Generator().manual_seed(0)
    x, t = torch.randn(6, 4, generator=g), torch.randn(6, 5, generator=g)
    idx = torch.tensor([0, 2, 5])
    for kw in ({}, {"normalize": False}, {"idx": idx}):
        with pytest.raises(_lib.HipExtensionError):
            E.rbf_bandwidth(x, **kw)
    for kw in ({}, {"normalize": False}, {"idx": idx}, {"sigma": 0.5}, {"sigma": (0.5, 0.7)}):
        with pytest.raises(_lib.HipExtensionError):
            E.kernel_cka(x, t, **kw)
    with pytest.raises(_lib.HipExtensionError):
        E.representation_similarity(x, t, idx, None, kernel_cka=True)


def test_the_default_signature_keeps_the_three_keys():
    sig = inspect.signature(S.representation_similarity)
    assert list(sig.parameters) == ["feat", "teacher_feat", "idx", "edge_index", "kernel_cka"]
    assert sig.parameters["kernel_cka"].default is False
    assert inspect.signature(M.student_similarity).parameters["kernel_cka"].default is False
    # the metrics replaced from the outside: what the function assembles, without a GPU
    x = torch.zeros(4, 3)
    saved = {n: getattr(S, n) for n in ("_check_pair", "_unit_rows", "_global_r", "_cka", "_kcka")}
    try:
        S._check_pair = lambda *a: None
        S._unit_rows = lambda t, idx: t
        S._global_r = lambda a, b: 0.25
        S._cka = lambda a, b: 0.5
        S._kcka = lambda a, b, sigma: 0.75
        assert S.representation_similarity(x, x, None) == dict(global_=0.25, local=None, cka=0.5)
        assert S.representation_similarity(x, x, None, kernel_cka=False) == dict(global_=0.25, local=None, cka=0.5)
        assert S.representation_similarity(x, x, None, kernel_cka=True) == dict(global_=0.25, local=None, cka=0.5, kcka=0.75)
    finally:
        for n, f in saved.items():
            setattr(S, n, f)
