"""The dropout gate arithmetic of the fused BatchNorm kernels (run with ``-m gpu``), csrc/bn_common.h ``bn_gate`` / ``bn_keep4_hash``.

The kernels read seed + *seed_dev once, scale a kept element by a 1 / (1 - p) formed once, and below 2^32 elements form the hash's
element index in 32 bits and leave out the term of its (zero) upper half.  None of that may change one bit of any mask: every kernel
that draws or re-draws the mask is compared here with the host restatement of the hash (oracle/dropout.py), to EQUALITY of the gate
pattern, and the forward values to equality with (undropped output) * (oracle mask).

  * streaming kernels (bn_act_fwd_kernel, bn_act_bwd_reduce_kernel, bn_act_bwd_apply_kernel): (n, C) = (1, 4) a single element
    quartet; (5, 256) one workgroup; (33, 256) several workgroups; (130, 260) two column chunks, the second with one live lane;
    (1031, 1024) the widest row; ld = C and C + 4; p = 0.1 and 0.5; a seed with a non-zero upper half, with and without seed_dev;
    and (32 773, 256), chosen from the launchers' grid caps: bn_act_bwd_reduce_kernel runs at most 512 workgroups (a sweep of 2048
    rows) and takes four rows per iteration while row + 3 * 2048 < n, then single rows; the forward and apply kernels run at most
    2048 workgroups (8192 rows per sweep, 1024 / 4096 with column sums) and take single rows.  With n = 4 * 8192 + 5 the wave that
    starts at row r < 5 of the reduce pass runs its four-row body four times (rows r .. r + 30 720) and then the one-row remainder loop
    once (row r + 32 768); every other wave runs only the body; every wave of the forward and apply passes takes four to nine single rows.
    The benchmark's 169 343 rows take the same two loops.  (Two (p, seed_dev) pairs there: its host restatement takes a second each.);
  * the tail (BatchNorm + ReLU + dropout feeding a narrow Linear, Ks = 40): n = 1, 31, 32, 33, 3000 in the tile form (C = 256:
    tail_fwd_tile_kernel / tail_bwd_tile_kernel) and in the MFMA-layout form the host takes for other widths (C = 128:
    skinny_dx_bn_kernel), with and without the row-compact addend.

The index path for more than 2^32 elements (``BnParams::wide``, chosen in ``bn_unpack`` alone) is the arithmetic the kernels had
before; it needs a 16 GiB tensor and is not run here.
"""
import ctypes
import functools

import pytest
import torch

from efficient_gnns_amd import _lib
from oracle.dropout import counter_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda"
MASK64 = (1 << 64) - 1
SEED = 0x9E3779B97F4A7C15          # non-zero upper half
SEED_DEV = 0x0123456789ABCDEF
EPS = 1e-5

N_BOTH_LOOPS = 4 * 8192 + 5        # see the module docstring
STREAM_SHAPES = [(1, 4), (5, 256), (33, 256), (130, 260), (1031, 1024), (N_BOTH_LOOPS, 256)]
COMBOS = [(0.1, False), (0.1, True), (0.5, False), (0.5, True)]     # (p, with seed_dev)


@functools.lru_cache(maxsize=None)
def oracle_uniform(seed, n, C):
    return torch.from_numpy(counter_uniform(seed, n, C))


def oracle_mask(seed, n, C, p):
    """oracle.dropout.counter_mask from the cached uniforms: 1 / (1 - p) where u >= p, else 0 (float32 arithmetic)."""
    u = oracle_uniform(seed & MASK64, n, C)
    pf = torch.tensor(p, dtype=torch.float32)
    return torch.where(u >= pf, torch.tensor(1.0) / (torch.tensor(1.0) - pf), torch.tensor(0.0))


class Case:
    """One BatchNorm call over x [n, C] with pitch ld: statistics of x itself, random affine parameters, ReLU, dropout p."""

    def __init__(self, n, C, ld, p, with_seed_dev, gen_seed=0):
        g = torch.Generator().manual_seed(1000 * gen_seed + n + C)
        self.n, self.C, self.ld, self.p = n, C, ld, p
        self.x = (torch.randn(n, ld, generator=g) * 1.5 + 0.3).to(DEV)[:, :C]
        self.mean = self.x.mean(0).contiguous()
        self.var = self.x.var(0, unbiased=False).contiguous() if n > 1 else torch.ones(C, device=DEV)
        self.gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
        self.beta = (torch.randn(C, generator=g) * 0.3).to(DEV)
        self.dy = (torch.randn(n, ld, generator=g).abs() + 0.5).to(DEV)[:, :C]      # never zero: d != 0 exactly where the gate is
        self.seed_dev = torch.tensor([SEED_DEV], dtype=torch.int64, device=DEV) if with_seed_dev else None
        self.total_seed = (SEED + (SEED_DEV if with_seed_dev else 0)) & MASK64

    def desc(self, p=None):
        return ctypes.byref(_lib.BnAct(_lib.ptr(self.x), self.ld, self.n, self.C, _lib.ptr(self.mean), _lib.ptr(self.var), EPS,
                                       _lib.ptr(self.gamma), _lib.ptr(self.beta), 1, self.p if p is None else p, SEED,
                                       _lib.ptr(self.seed_dev), None, 0))

    def forward(self, p=None):
        y = torch.empty(self.n, self.ld, device=DEV)[:, :self.C]
        _lib.check(_lib.load().egnn_bn_act_fwd_f32(self.desc(p), _lib.ptr(y), self.ld, _lib.stream()), "fwd")
        return y

    def backward(self, batch_stats):
        """egnn_bn_act_bwd_f32 (reduce + apply with the column sums of dx): dx, dgamma, dbeta, colsum."""
        lib = _lib.load()
        C = self.C
        nws = lib.egnn_bn_ws_floats(C)
        ws = torch.empty(nws, device=DEV)
        dx = torch.empty(self.n, self.ld, device=DEV)[:, :C]
        dg, db, cs = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        _lib.check(lib.egnn_bn_act_bwd_f32(self.desc(), _lib.ptr(self.dy), self.ld, batch_stats, _lib.ptr(dg), _lib.ptr(db), _lib.ptr(dx),
                                           self.ld, _lib.ptr(cs), _lib.ptr(ws), nws, _lib.stream()), "bwd")
        return dx, dg, db, cs


@pytest.mark.parametrize("pad", [0, 4], ids=["ld=C", "ld=C+4"])
@pytest.mark.parametrize("n,C", STREAM_SHAPES)
def test_streaming_kernels_draw_the_host_restatements_mask(n, C, pad):
    for p, with_dev in ([(0.1, False), (0.5, True)] if n == N_BOTH_LOOPS else COMBOS):
        case = Case(n, C, C + pad, p, with_dev)
        tag = f"n={n} C={C} ld={C + pad} p={p} seed_dev={with_dev}"
        want = oracle_mask(case.total_seed, n, C, p).to(DEV)
        y, y_nodrop = case.forward(), case.forward(p=0.0)
        # forward: the kept elements are scaled by exactly 1 / (1 - p), the others are zero
        assert torch.equal(y, y_nodrop * want), tag
        gate = (y_nodrop > 0) & (want != 0)                      # ReLU sign and dropout decision
        # backward with running statistics (no mean / variance terms): dx = gamma rstd dy gate, zero exactly where the gate is
        dx, dg, db, cs = case.backward(0)
        assert torch.equal(dx != 0, gate), tag + ": apply pass"
        d = case.dy.double() * gate * want.double()
        rstd = (case.var.double() + EPS).rsqrt()
        assert torch.allclose(dx.double(), case.gamma.double() * rstd * d, rtol=1e-5, atol=1e-6), tag
        # the reduce pass: sum d and sum d xhat over the same gate against float64; bound of an fp32 sum of n terms in any order:
        # (n + 2) eps sum |term| (eps = 2^-23; + 2: the rounding of d and of xhat)
        xhat = (case.x.double() - case.mean.double()) * rstd
        bound = (n + 2) * 2.0 ** -23
        assert bool(((db.double() - d.sum(0)).abs() <= bound * d.abs().sum(0) + 1e-30).all()), tag + ": reduce pass (dbeta)"
        assert bool(((dg.double() - (d * xhat).sum(0)).abs() <= bound * (d * xhat).abs().sum(0) + 1e-30).all()), tag + ": reduce pass (dgamma)"
        # training backward (batch statistics: the mean / variance terms of the apply pass, the form the benchmark runs) against
        # float64: dx = gamma rstd (d - (sum d + xhat sum d xhat) / n).  Bound per element: the two sums carry the summation bound
        # above, every other operand a few roundings (8 eps of the magnitudes added, rsqrtf's 2 ulp included)
        dx1, dg1, db1, cs1 = case.backward(1)
        assert torch.equal(dg1, dg) and torch.equal(db1, db), tag + ": the reduce pass does not depend on batch_stats"
        S1, S2 = d.sum(0), (d * xhat).sum(0)
        A1, A2 = d.abs().sum(0), (d * xhat).abs().sum(0)
        gr = (case.gamma.double() * rstd).abs()
        ref = case.gamma.double() * rstd * (d - (S1 + xhat * S2) / n)
        tol = gr * (bound * (A1 + xhat.abs() * A2) / n + 8 * 2.0 ** -23 * (d.abs() + (S1.abs() + xhat.abs() * S2.abs()) / n)) + 1e-30
        assert bool(((dx1.double() - ref).abs() <= tol).all()), tag + ": apply pass with batch statistics"
        assert bool(((cs1.double() - ref.sum(0)).abs() <= bound * ref.abs().sum(0) + tol.sum(0)).all()), tag + ": column sums of dx"
        # a dropped element contributes nothing: with dy = +-big on the dropped elements only, both sums stay exactly zero
        case.dy[:] = torch.where(gate, torch.zeros_like(want), torch.full_like(want, 1e30))
        dx0, dg0, db0, _ = case.backward(0)
        assert float(db0.abs().max()) == 0.0 and float(dg0.abs().max()) == 0.0 and float(dx0.abs().max()) == 0.0, tag


def tail_backward(case, W, G, rows=None, inv=None):
    """egnn_skinny_dx_bn_bwd_reduce_f32: d = dh * gate (left in dx), dgamma, dbeta."""
    lib = _lib.load()
    n, C, Ks = case.n, case.C, W.shape[1]
    nws = lib.egnn_skinny_dx_bn_ws_floats(n, C)
    ws = torch.empty(nws, device=DEV)
    dx = torch.empty(n, C, device=DEV)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    _lib.check(lib.egnn_skinny_dx_bn_bwd_reduce_f32(_lib.ptr(G), G.stride(0), _lib.ptr(W), W.stride(0), 0, Ks, 1.0, None, 0, _lib.ptr(rows),
                                                    0 if rows is None else rows.stride(0), _lib.ptr(inv), case.desc(), _lib.ptr(dg),
                                                    _lib.ptr(db), _lib.ptr(dx), C, _lib.ptr(ws), nws, _lib.stream()), "tail reduce")
    return dx, dg, db


@pytest.mark.parametrize("with_rows", [False, True], ids=["plain", "add_rows"])
@pytest.mark.parametrize("C", [256, 128], ids=["tile", "mfma-layout"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 3000])
def test_tail_kernels_draw_the_host_restatements_mask(n, C, with_rows):
    """C = 256 takes tail_fwd_tile_kernel / tail_bwd_tile_kernel, C = 128 bn_act_fwd_kernel / skinny_dx_bn_kernel (the host's choice:
    tail_tile_form needs C == 256); Ks = 40 as in the model of record."""
    lib = _lib.load()
    Ks, p = 40, 0.5
    case = Case(n, C, C, p, True, gen_seed=7)
    g = torch.Generator().manual_seed(n + C)
    W = (torch.randn(C, Ks, generator=g) * 0.1).to(DEV)
    G = torch.randn(n, Ks, generator=g).to(DEV)
    rows = inv = None
    dh = G.double() @ W.double().t()
    if with_rows:
        ids = torch.randperm(n, generator=g)[:max(1, n // 3)]
        rows = torch.randn(ids.numel(), C, generator=g).to(DEV)
        inv = torch.full((n,), -1, dtype=torch.int32)
        inv[ids] = torch.arange(ids.numel(), dtype=torch.int32)
        inv = inv.to(DEV)
        dh[ids.to(DEV)] += rows.double()
    want = oracle_mask(case.total_seed, n, C, p).to(DEV)
    y_nodrop = case.forward(p=0.0)
    if C == 256:
        h, xw = torch.empty(n, C, device=DEV), torch.empty(n, Ks, device=DEV)
        _lib.check(lib.egnn_bn_act_linear_fwd_f32(case.desc(), _lib.ptr(W), Ks, 0, Ks, _lib.ptr(h), C, _lib.ptr(xw), Ks, _lib.stream()),
                   "linear fwd")
        assert torch.equal(h, y_nodrop * want), "h of the tile form"
        assert torch.equal(h, case.forward()), "h of the tile form is bn_act_fwd_kernel's h"
        assert torch.allclose(xw.double(), h.double() @ W.double(), rtol=1e-4, atol=1e-4)
    gate = (y_nodrop > 0) & (want != 0)
    d, dg, db = tail_backward(case, W, G, rows, inv)
    assert torch.equal(d != 0, gate & (dh != 0)), f"n={n} C={C} rows={with_rows}: gate pattern of d"
    ref = dh * gate * want.double()
    assert torch.allclose(d.double(), ref, rtol=1e-4, atol=1e-5)
    # (fp32 sum of n terms in any order: (n + 2) eps sum |term|, the terms themselves within 1e-4 of the float64 ones)
    assert bool(((db.double() - ref.sum(0)).abs() <= ((n + 2) * 2.0 ** -23 + 1e-4) * ref.abs().sum(0) + 1e-5).all())
