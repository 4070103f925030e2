"""Softmax over the groups of an unsorted index on the GPU (csrc/scatter_softmax.hip, ``ops.scatter_softmax``, the multi-dimensional
``utils.softmax``, the ``torch_scatter`` composite shim, an attention conv through ``nn.MessagePassing``) against float64 torch on
the CPU.  The references are written here with ``index_add_`` and ``scatter_reduce(amax, include_self=False)``.

Bars: forward rtol 1e-5, atol 1e-6 max|ref|; gradients rtol 1e-4, atol 1e-5 max|ref| (the project's bar for this operation on sorted
segments).  Shapes: 37 rows, E in {0, 1, 700} with one hub named 300 times (three chunks of EGNN_ROWS_SUM_CHUNK = 128), and a second
index whose runs are exactly 1, 2, 127, 128, 129, 256 and 257 long; every third id is negative, the order is shuffled, some rows are
never named."""
import ctypes
import functools
import importlib.util
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from efficient_gnns_amd import _lib, ops, utils
from efficient_gnns_amd import nn as PN
from conftest import ROOT

pytestmark = pytest.mark.gpu

N_ROWS, HUB, EMPTY = 37, 7, (0, 1, 2, 3, 4, 36)
RUN_LENGTHS = (1, 2, 127, 128, 129, 256, 257)
CASES = ("E0", "E1", "E700", "runs")
CS = (1, 3, 4, 12)
DROPIN = os.path.join(ROOT, "efficient-gnns_amd", "dropin")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def close(got, ref, what):
    """|got - ref| <= atol + rtol |ref| with the bars of the module docstring."""
    rtol, scale = {"fwd": (1e-5, 1e-6), "grad": (1e-4, 1e-5)}[what]
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return
    atol = scale * float(ref.abs().max())
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {ref.numel()} off, worst |err| {float(err.max()):.3e} (atol {atol:.3e}, rtol {rtol})"


@functools.lru_cache(maxsize=None)
def make_index(case):
    """(rows, raw): [E] int64 on the CPU, already wrapped, and the form handed to the kernels (every third id negative)."""
    g = torch.Generator().manual_seed(2000 + len(case) + sum(map(ord, case)))
    if case == "E0":
        rows = torch.zeros(0, dtype=torch.int64)
    elif case == "E1":
        rows = torch.tensor([N_ROWS - 3])
    elif case == "E700":
        allowed = torch.tensor([r for r in range(N_ROWS) if r not in EMPTY and r != HUB])
        rows = torch.cat([torch.full((300,), HUB, dtype=torch.int64), allowed[torch.randint(0, allowed.numel(), (400,), generator=g)]])
        rows = rows[torch.randperm(700, generator=g)]
    else:   # row 10 + 3 i is named exactly RUN_LENGTHS[i] times
        rows = torch.cat([torch.full((n,), 10 + 3 * i, dtype=torch.int64) for i, n in enumerate(RUN_LENGTHS)])
        rows = rows[torch.randperm(rows.numel(), generator=g)]
    raw = rows.clone()
    raw[::3] -= N_ROWS
    return rows, raw


@functools.lru_cache(maxsize=None)
def gpu_index(case):
    return make_index(case)[1].to(dev())


def reference(x, rows, g, eps, log, n=N_ROWS):
    """float64 CPU: (out, dsrc) for ``rows`` already wrapped; a row id outside [0, n) marks a dropped position (0 in both)."""
    x = x.double().cpu()
    E, tail = x.shape[0], x.shape[1:]
    C = 1
    for d in tail:
        C *= d
    s = x.reshape(E, C).clone().requires_grad_(True)
    live = (rows >= 0) & (rows < n)
    r, sl = rows[live], s[live]
    M = torch.zeros(n, C, dtype=torch.float64).scatter_reduce(0, r.view(-1, 1).expand(-1, C), sl.detach(), "amax", include_self=False)
    e = sl - M[r]
    Z = torch.zeros(n, C, dtype=torch.float64).index_add_(0, r, e.exp())
    val = e - (Z[r] + eps).log() if log else e.exp() / (Z[r] + eps)
    out = torch.zeros(E, C, dtype=torch.float64).index_put((live.nonzero().view(-1),), val)
    if E and C:
        (dsrc,) = torch.autograd.grad(out, s, g.double().cpu().reshape(E, C))
    else:
        dsrc = torch.zeros(E, C, dtype=torch.float64)
    return out.detach().reshape((E,) + tail), dsrc.reshape((E,) + tail)


@functools.lru_cache(maxsize=None)
def make_values(case, tail, spread):
    """src = 3 randn and an upstream gradient (float32 CPU).  ``spread``: +100 on some positions and -100 on others INSIDE the same
    runs, and the hub's / the longest run's largest value placed once in its first chunk and once in its last -- without the max shift
    exp(100) overflows fp32, and a chunk merge that rescales wrongly shows at once."""
    rows, _ = make_index(case)
    E = rows.numel()
    gen = torch.Generator().manual_seed(31 * E + 7 * sum(tail) + len(tail) + (1 if spread else 0))
    x = 3 * torch.randn((E,) + tail, generator=gen)
    g = torch.randn((E,) + tail, generator=gen)
    if spread and E > 1:
        pos = torch.arange(E)
        x[pos % 5 == 0] += 100.0
        x[pos % 5 == 1] -= 100.0
        big = HUB if case == "E700" else 10 + 3 * (len(RUN_LENGTHS) - 1)
        at = (rows == big).nonzero().view(-1)               # ascending position = the order of the run
        assert at.numel() > 256
        x[at[3]] = 150.0
        x[at[-2]] = 150.0
    return x, g


def run(x, g, index, eps, log, plan=None, n=N_ROWS):
    src = x.to(dev()).requires_grad_(True)
    out = ops.scatter_softmax(src, index, n, plan=plan, eps=eps, log=log)
    (dsrc,) = torch.autograd.grad(out, src, g.to(dev())) if out.numel() else (torch.zeros_like(src),)
    return out.detach(), dsrc


# ------------------------------------------------------------------------------------------------
# values and gradients
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("case", CASES)
def test_values_and_gradients_both_forms_both_eps(case, C):
    rows, _ = make_index(case)
    x, g = make_values(case, (C,), False)
    for log in (False, True):
        for eps in (0.0, 1e-16):
            out, dsrc = run(x, g, gpu_index(case), eps, log)
            ref_out, ref_dsrc = reference(x, rows, g, eps, log)
            assert out.shape == x.shape and dsrc.shape == x.shape
            close(out, ref_out, "fwd")
            close(dsrc, ref_dsrc, "grad")


@pytest.mark.parametrize("C", (1, 4))
@pytest.mark.parametrize("case", ("E700", "runs"))
def test_values_a_hundred_apart_inside_one_run(case, C):
    rows, _ = make_index(case)
    x, g = make_values(case, (C,), True)
    for log in (False, True):
        for eps in (0.0, 1e-16):
            out, dsrc = run(x, g, gpu_index(case), eps, log)
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dsrc).all())
            ref_out, ref_dsrc = reference(x, rows, g, eps, log)
            close(out, ref_out, "fwd")
            close(dsrc, ref_dsrc, "grad")


def test_trailing_dimensions_are_flattened():
    rows, _ = make_index("E700")
    x, g = make_values("E700", (3, 4), False)
    out, dsrc = run(x, g, gpu_index("E700"), 0.0, False)
    ref_out, ref_dsrc = reference(x, rows, g, 0.0, False)
    assert out.shape == (700, 3, 4) and dsrc.shape == (700, 3, 4)
    close(out, ref_out, "fwd")
    close(dsrc, ref_dsrc, "grad")
    flat, _ = run(x.reshape(700, 12), g.reshape(700, 12), gpu_index("E700"), 0.0, False)
    assert torch.equal(out.reshape(700, 12), flat)
    # no column, no row: empty results of the right shape without a launch
    assert ops.scatter_softmax(torch.zeros(700, 0, 4, device=dev()), gpu_index("E700"), N_ROWS).shape == (700, 0, 4)
    assert ops.scatter_softmax(torch.zeros(0, 3, device=dev()), gpu_index("E0"), N_ROWS).shape == (0, 3)
    assert ops.scatter_softmax(torch.zeros(0, 3, device=dev()), gpu_index("E0"), 0).shape == (0, 3)


@pytest.mark.parametrize("case", ("E1", "E700", "runs"))
def test_the_probabilities_of_every_named_row_sum_to_one(case):
    rows, _ = make_index(case)
    for spread in (False, True):
        x, g = make_values(case, (3,), spread)
        out, _ = run(x, g, gpu_index(case), 0.0, False)
        total = torch.zeros(N_ROWS, 3, dtype=torch.float64).index_add_(0, rows, out.double().cpu())
        named = torch.zeros(N_ROWS, dtype=torch.bool).index_fill_(0, rows, True)
        assert float((total[named] - 1).abs().max()) <= 1e-5
        assert float(total[~named].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------
# bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("E700", "runs"))
def test_two_calls_are_bit_equal_and_the_columns_are_independent(case):
    for C in (3, 4, 12):
        x, g = make_values(case, (C,), False)
        for log in (False, True):
            a, da = run(x, g, gpu_index(case), 1e-16, log)
            b, db = run(x, g, gpu_index(case), 1e-16, log)
            assert torch.equal(a, b) and torch.equal(da, db)
            for c in range(C):
                one, done = run(x[:, c:c + 1].contiguous(), g[:, c:c + 1].contiguous(), gpu_index(case), 1e-16, log)
                assert torch.equal(a[:, c:c + 1], one), (C, c, log)
                assert torch.equal(da[:, c:c + 1], done), (C, c, log)


def raw_call(plan, x, g, pitch, offset, eps, form):
    """Both entry points through ctypes on operands laid out with ``pitch`` floats per row, starting ``offset`` floats into a
    256-byte aligned buffer: (out, dsrc) as contiguous tensors."""
    lib, d = _lib.load(), dev()
    S, C = x.shape

    def lay(t=None):
        buf = torch.full((S * pitch + offset + 4,), float("nan"), device=d)
        view = buf[offset:offset + S * pitch].view(S, pitch)[:, :C]
        if t is not None:
            view.copy_(t)
        assert view.data_ptr() % 16 == (4 * offset) % 16
        return view
    src, out, gg, dsrc = lay(x.to(d)), lay(), lay(g.to(d)), lay()
    stats = torch.empty(3, N_ROWS, C, device=d)
    nws = lib.egnn_scatter_softmax_ws_bytes(S, C)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=d)
    common = (_lib.ptr(plan.all_keys), S, plan.shift, _lib.ptr(plan.rows))
    _lib.check(lib.egnn_scatter_softmax_fwd_f32(_lib.ptr(out), pitch, _lib.ptr(stats[0]), _lib.ptr(stats[1]), N_ROWS, *common, _lib.ptr(src),
                                                pitch, C, eps, form, _lib.ptr(ws), nws, _lib.stream()), "egnn_scatter_softmax_fwd_f32")
    _lib.check(lib.egnn_scatter_softmax_bwd_f32(_lib.ptr(dsrc), pitch, _lib.ptr(stats[2]), N_ROWS, *common, _lib.ptr(out), pitch, _lib.ptr(gg),
                                                pitch, C, form, _lib.ptr(ws), nws, _lib.stream()), "egnn_scatter_softmax_bwd_f32")
    return out.contiguous(), dsrc.contiguous(), stats


@pytest.mark.parametrize("C", CS)
def test_a_padded_pitch_and_a_misaligned_base_give_the_contiguous_bits(C):
    plan = ops.rows_plan(gpu_index("E700"), N_ROWS)
    x, g = make_values("E700", (C,), False)
    for form in (0, 1):
        want, dwant = run(x, g, gpu_index("E700"), 1e-16, bool(form))
        # (pitch, offset in floats): contiguous; padded by 4 (16 bytes per lane stays possible when C % 4 == 0); padded by 1; base off by 4 bytes
        for pitch, offset in ((C, 0), (C + 4, 0), (C + 1, 0), (C, 1), (C + 4, 3)):
            out, dsrc, stats = raw_call(plan, x, g, pitch, offset, 1e-16, form)
            assert torch.equal(out, want), (C, form, pitch, offset)
            assert torch.equal(dsrc, dwant), (C, form, pitch, offset)
            assert bool(torch.isfinite(stats).all())                               # every row of the per-row buffers was written
            assert float(stats[:, list(EMPTY)].abs().max()) == 0.0                 # ... with 0 for a row that no key names


# ------------------------------------------------------------------------------------------------
# a deferred plan with ids out of range
# ------------------------------------------------------------------------------------------------
def test_a_deferred_plan_drops_and_counts_ids_out_of_range():
    rows, raw = make_index("E700")
    bad = torch.arange(5, 700, 41)
    raw, rows = raw.clone(), rows.clone()
    raw[bad[::2]] = N_ROWS + 3
    raw[bad[1::2]] = -N_ROWS - 2
    rows[bad] = -1                                                                 # the reference is computed without them
    ops.rows_oob(dev())
    plan = ops.rows_plan(raw.to(dev()), N_ROWS, check="deferred")
    for C in (3, 4):
        x, g = make_values("E700", (C,), False)
        for log in (False, True):
            out, dsrc = run(x, g, None, 0.0, log, plan=plan)
            assert float(out[bad.to(dev())].abs().max()) == 0.0 and float(dsrc[bad.to(dev())].abs().max()) == 0.0
            ref_out, ref_dsrc = reference(x, rows, g, 0.0, log)
            close(out, ref_out, "fwd")
            close(dsrc, ref_dsrc, "grad")
    assert ops.rows_oob(dev()) == bad.numel()


# ------------------------------------------------------------------------------------------------
# the public spellings
# ------------------------------------------------------------------------------------------------
def test_one_column_agrees_with_the_one_dimensional_path():
    for case in ("E700", "runs"):
        rows, _ = make_index(case)
        x, g = make_values(case, (), False)
        one_d = utils.softmax(x.to(dev()), rows.to(dev()), num_nodes=N_ROWS)
        assert one_d.shape == x.shape
        two_d = ops.scatter_softmax(x.to(dev())[:, None], rows.to(dev()), N_ROWS, eps=1e-16)
        close(two_d[:, 0], one_d, "fwd")
        close(one_d, reference(x[:, None], rows, g[:, None], 1e-16, False)[0][:, 0], "fwd")


def test_utils_softmax_on_head_scores(monkeypatch):
    rows, raw = make_index("E700")
    x, g = make_values("E700", (3,), False)
    ref_out, ref_dsrc = reference(x, rows, g, 1e-16, False)
    built = []
    real = ops._rows_plan_launch
    monkeypatch.setattr(ops, "_rows_plan_launch", lambda ids, n: built.append(n) or real(ids, n))
    for index, kw in ((raw.to(dev()), {"num_nodes": N_ROWS}), (rows.to(dev()), {}), (rows.to(dev()), {"num_nodes": N_ROWS, "dim": -2})):
        src = x.to(dev()).requires_grad_(True)
        out = utils.softmax(src, index, **kw)
        (dsrc,) = torch.autograd.grad(out, src, g.to(dev()))
        close(out, ref_out, "fwd")
        close(dsrc, ref_dsrc, "grad")
    assert built == [N_ROWS, int(rows.max()) + 1, N_ROWS]
    # ptr in place of index: consecutive groups
    order = torch.argsort(rows, stable=True)
    ptr = torch.zeros(N_ROWS + 1, dtype=torch.int64)
    ptr[1:] = torch.bincount(rows, minlength=N_ROWS).cumsum(0)
    out = utils.softmax(x[order].to(dev()), None, ptr.to(dev()))
    close(out, ref_out[order], "fwd")
    with pytest.raises(NotImplementedError, match="dim"):
        utils.softmax(x.to(dev()), rows.to(dev()), dim=1)


def test_torch_scatter_composite_functions():
    names = ("torch_scatter",)
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in names or k.startswith("torch_scatter.")}
    sys.path.insert(0, DROPIN)
    try:
        from torch_scatter.composite import scatter_log_softmax, scatter_softmax
        rows, raw = make_index("E700")
        x, g = make_values("E700", (3, 4), False)
        for fn, log in ((scatter_softmax, False), (scatter_log_softmax, True)):
            ref_out, ref_dsrc = reference(x, rows, g, 0.0, log)
            for index, kw in ((raw.to(dev()), {"dim": 0, "dim_size": N_ROWS}), (rows.to(dev()), {"dim": -3})):
                src = x.to(dev()).requires_grad_(True)
                out = fn(src, index, **kw)
                (dsrc,) = torch.autograd.grad(out, src, g.to(dev()))
                close(out, ref_out, "fwd")
                close(dsrc, ref_dsrc, "grad")
    finally:
        sys.path.remove(DROPIN)
        for k in [k for k in sys.modules if k in names or k.startswith("torch_scatter.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ------------------------------------------------------------------------------------------------
# end to end: a multi-head attention conv in PyG's idiom
# ------------------------------------------------------------------------------------------------
class AttConv(PN.MessagePassing):
    def __init__(self, c_in, heads, c_head):
        super().__init__(aggr="add", node_dim=0)
        self.heads, self.c_head = heads, c_head
        self.lin = torch.nn.Linear(c_in, heads * c_head, bias=False)
        self.att_l = torch.nn.Parameter(torch.empty(1, heads, c_head))
        self.att_r = torch.nn.Parameter(torch.empty(1, heads, c_head))

    def forward(self, x, edge_index):
        h = self.lin(x).view(-1, self.heads, self.c_head)
        alpha_l, alpha_r = (h * self.att_l).sum(-1), (h * self.att_r).sum(-1)
        out = self.propagate(edge_index, x=h, alpha=(alpha_l, alpha_r))
        return out.reshape(-1, self.heads * self.c_head)

    def message(self, x_j, alpha_j, alpha_i, index, ptr, size_i):
        alpha = F.leaky_relu(alpha_j + alpha_i, 0.2)
        alpha = utils.softmax(alpha, index, ptr, size_i)
        return x_j * alpha.unsqueeze(-1)


def att_reference(x, w, att_l, att_r, ei, g, heads, c_head, n):
    """The conv restated in float64 on the CPU: (out, [dx, dw, datt_l, datt_r])."""
    x, w, att_l, att_r = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, att_l, att_r))
    j, i = ei[0].cpu(), ei[1].cpu()
    h = (x @ w.t()).view(-1, heads, c_head)
    al, ar = (h * att_l).sum(-1), (h * att_r).sum(-1)
    s = F.leaky_relu(al[j] + ar[i], 0.2)
    M = torch.zeros(n, heads, dtype=torch.float64).scatter_reduce(0, i.view(-1, 1).expand(-1, heads), s.detach(), "amax", include_self=False)
    e = (s - M[i]).exp()
    Z = torch.zeros(n, heads, dtype=torch.float64).index_add_(0, i, e)
    alpha = e / (Z[i] + 1e-16)
    out = torch.zeros(n, heads, c_head, dtype=torch.float64).index_add_(0, i, h[j] * alpha.unsqueeze(-1)).reshape(n, heads * c_head)
    grads = torch.autograd.grad(out, (x, w, att_l, att_r), g.double().cpu())
    return out.detach(), grads


def load_accel():
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_ssm", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    return accel


@pytest.mark.parametrize("under_accel", (False, True))
def test_attention_conv_shares_one_plan_per_endpoint(under_accel, monkeypatch):
    N, H, F_, C_IN = N_ROWS, 3, 4, 6
    gen = torch.Generator().manual_seed(99)
    rows, _ = make_index("E700")
    full = torch.stack([torch.randint(0, N, (900,), generator=gen), torch.cat([rows, torch.randint(0, N, (200,), generator=gen)])])
    mask = torch.zeros(900, dtype=torch.bool)
    mask[:700] = True                                                              # the 700 edges whose targets are the hub index
    conv = AttConv(C_IN, H, F_)
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.7)
    x = torch.randn(N, C_IN, generator=gen)
    g = torch.randn(N, H * F_, generator=gen)
    ref_out, ref_grads = att_reference(x, conv.lin.weight, conv.att_l, conv.att_r, full[:, mask], g, H, F_, N)

    conv = conv.to(dev())
    xg = x.to(dev()).requires_grad_(True)
    built = []
    real = ops._rows_plan_launch
    monkeypatch.setattr(ops, "_rows_plan_launch", lambda ids, n: built.append(n) or real(ids, n))

    def step():
        out = conv(xg, full.to(dev())[:, mask.to(dev())])                          # a fresh edge_index[:, mask]
        return out, torch.autograd.grad(out, (xg, conv.lin.weight, conv.att_l, conv.att_r), g.to(dev()))
    if under_accel:
        accel = load_accel()
        with accel.scope():
            out, grads = step()
    else:
        out, grads = step()
    assert len(built) <= 2, built                                                  # one plan per endpoint: the softmax shares the aggregation's
    assert not PN._MP_RUNNING
    close(out, ref_out, "fwd")
    for a, b in zip(grads, ref_grads):
        close(a, b, "grad")
