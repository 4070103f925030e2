"""CPU-side checks of the structure-preservation metrics (efficient-gnns_amd/similarity.py, csrc/similarity.hip): the four C ABI
additions are declared, exported and bound; the public functions exist and refuse CPU tensors; ``pearson_from_moments`` against
``scipy.stats.pearsonr`` on float64 moments; the entry points' argument checks that need no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.stats import pearsonr

import efficient_gnns_amd as E
import efficient_gnns_amd.models as M
import efficient_gnns_amd.similarity as S
from efficient_gnns_amd import _lib, build
from conftest import ROOT

NEW = ("egnn_pair_moments_ws_bytes", "egnn_pair_moments_f32", "egnn_pearson_moments_ws_bytes", "egnn_pearson_moments_f32")
KINDS = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}


def header(strip_comments=True):
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S) if strip_comments else src


def ctype_of(decl):
    d = decl.strip()
    return C.c_void_p if "*" in d else KINDS[re.sub(r"\bconst\b", "", d).split()[0]]


def moments(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return [float(a.size), a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()]


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
    assert "similarity.hip" in build.SOURCES
    whole = header(strip_comments=False)
    assert "correlation.py:178-181" in whole, "the header cites the reference lines the moments stand for"


def test_workspace_sizes():
    lib = _lib.load()
    for N, tiles in ((2, 1), (128, 1), (129, 3), (257, 6), (641, 21), (29799, 233 * 234 // 2), (169343, 1323 * 1324 // 2)):
        assert lib.egnn_pair_moments_ws_bytes(N) == tiles * 6 * 8, N
    assert lib.egnn_pearson_moments_ws_bytes(1) == 48
    assert lib.egnn_pearson_moments_ws_bytes(257) == 2 * 48
    assert lib.egnn_pearson_moments_ws_bytes(10 ** 7) == 1024 * 48


def test_entry_points_reject_bad_arguments_before_any_launch():
    """Negative codes for N < 2, a leading dimension below the width, a short workspace and null pointers; callable without a GPU
    (nothing is launched and no pointer is followed)."""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    big = 1 << 20
    assert lib.egnn_pair_moments_f32(p, 8, 8, p, 8, 8, 1, p, p, big, None) == -1
    assert lib.egnn_pair_moments_f32(p, 7, 8, p, 8, 8, 4, p, p, big, None) == -1
    assert lib.egnn_pair_moments_f32(p, 8, 8, p, 7, 8, 4, p, p, big, None) == -1
    assert lib.egnn_pair_moments_f32(None, 8, 8, p, 8, 8, 4, p, p, big, None) == -1
    assert lib.egnn_pair_moments_f32(p, 8, 8, p, 8, 8, 4, p, p, 47, None) == -3
    assert lib.egnn_pair_moments_f32(p, 8, 8, p, 8, 8, 129, p, p, 3 * 48 - 1, None) == -3
    assert lib.egnn_pearson_moments_f32(p, p, 0, p, p, big, None) == -1
    assert lib.egnn_pearson_moments_f32(p, None, 4, p, p, big, None) == -1
    assert lib.egnn_pearson_moments_f32(p, p, 4, p, p, 47, None) == -3


def test_public_functions_exist_and_refuse_cpu_tensors():
    for name in ("structural_correlation", "local_structural_correlation", "linear_cka", "representation_similarity", "pair_moments",
                 "pearson_from_moments"):
        assert getattr(E, name) is getattr(S, name), name
    assert callable(M.student_similarity)
    g = torch.Generator().manual_seed(0)
    x, t = torch.randn(6, 4, generator=g), torch.randn(6, 5, generator=g)
    idx = torch.tensor([0, 2, 5])
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(_lib.HipExtensionError):
        E.structural_correlation(x, t)
    with pytest.raises(_lib.HipExtensionError):
        E.structural_correlation(x, t, idx)
    with pytest.raises(_lib.HipExtensionError):
        E.local_structural_correlation(x, t, ei)
    with pytest.raises(_lib.HipExtensionError):
        E.linear_cka(x, t)
    with pytest.raises(_lib.HipExtensionError):
        E.linear_cka(x, t, normalize=False)
    with pytest.raises(_lib.HipExtensionError):
        E.representation_similarity(x, t, idx, ei)
    with pytest.raises(_lib.HipExtensionError):
        E.pair_moments(x, t)
    with pytest.raises(_lib.HipExtensionError):
        S.vector_moments(x[:, 0], t[:, 0])


@pytest.mark.parametrize("n,rho", [(2, 0.5), (3, -0.9), (1000, 0.3), (1000, -0.7), (100000, 0.0), (100000, 0.999)])
def test_pearson_from_moments_matches_scipy(n, rho):
    rs = np.random.RandomState(n + int(1000 * abs(rho)))
    z = rs.randn(n)
    a = 0.4 + 0.2 * z                                           # cosine-like: a mean well away from 0
    b = -0.1 + 0.3 * (rho * z + math.sqrt(1 - rho * rho) * rs.randn(n))
    want = pearsonr(a, b)[0]
    got = S.pearson_from_moments(moments(a, b))
    # the moment form loses mean^2 / var of the float64 digits: a few 1e-14 here, 1e-12 leaves two orders of room
    assert abs(got - want) <= 1e-12, (got, want)
    assert S.pearson_from_moments(torch.tensor(moments(a, b), dtype=torch.float64)) == got
    # r is invariant under a -> 1 - a on both sides: similarities stand for the reference's distances
    assert abs(S.pearson_from_moments(moments(1 - a, 1 - b)) - want) <= 1e-12


def test_pearson_from_moments_edge_values():
    a = np.array([0.25, 0.5, 0.75, 1.0])
    assert S.pearson_from_moments(moments(a, a)) == 1.0
    assert S.pearson_from_moments(moments(a, -a)) == -1.0
    assert S.pearson_from_moments(moments(a, 3.0 * a + 2.0)) == pytest.approx(1.0, abs=1e-15)
    const = np.full(4, 0.3)
    assert math.isnan(S.pearson_from_moments(moments(a, const)))
    assert math.isnan(S.pearson_from_moments(moments(const, a)))
    assert math.isnan(S.pearson_from_moments(moments(const, const)))
    assert math.isnan(S.pearson_from_moments(moments(np.zeros(5), a[[0, 1, 2, 3, 0]])))
    assert math.isnan(S.pearson_from_moments(moments(np.full(1000, 0.1), np.linspace(0, 1, 1000))))   # 0.1 is inexact in binary
