"""The fused gather-weight-aggregate on the device (csrc/gather_scatter.hip, ``ops.gather_scatter``), its two backward kernels, and the
routes that reach it (``nn.MessagePassing``'s default message, ``lazy.LazyWeightedRows`` under ``accel``).

The defining property is BIT-EQUALITY with the existing composition ``ops.scatter(ops.take_rows(x, plan_src) * weight, None, dim_size,
reduce, plan=plan_dst)`` -- value and every gradient except the weights' -- asserted with ``torch.equal``.  Against float64 on the CPU
(``index_add_``, division by counts) the bars are those of tests/test_gpu_message_passing.py for the same kind of sums: forward rtol 1e-5,
atol 1e-5 * max|ref|; gradients (dx, dweight) rtol 1e-4, atol 1e-4 * max|ref|.  Small-integer inputs are exact.

Index design, on both endpoints independently: 37 target rows and 23 source rows, a hub named 300 times on each side (over two
EGNN_ROWS_SUM_CHUNKs: the workspace merge runs), rows never named, every third id negative, E in 0 | 1 | 700 in random order."""
import functools
import importlib.util
import os

import pytest
import torch

from efficient_gnns_amd import lazy, ops, utils
from efficient_gnns_amd import nn as PN
from conftest import ROOT

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 37, 23
SIDES = {"dst": (N_DST, 7, (0, 1, 2, 3, 4, 36), 0), "src": (N_SRC, 4, (0, 9, 22), 1)}    # rows, hub, never named, first negative position
ES = (0, 1, 700)
# (C, H, weight form): None, [E] and [E, H]; C = 40 / H = 5 has 8 columns per head, C = 260 / H = 5 has 52
SHAPES = [(C, 1, form) for C in (1, 3, 4, 40, 260) for form in (None, "E")] + [(4, 2, "EH"), (40, 2, "EH"), (260, 2, "EH"), (40, 5, "EH"),
                                                                               (260, 5, "EH"), (3, 1, "EH")]
REDUCES = ("sum", "mean")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def close(got, ref, rtol):
    ref = ref.detach().double().cpu()
    atol = rtol * float(ref.abs().max()) if ref.numel() else 0.0
    torch.testing.assert_close(got.detach().double().cpu(), ref, rtol=rtol, atol=atol)


@functools.lru_cache(maxsize=None)
def make_ends(E):
    """{side: (rows, raw)}: [E] int64 on the CPU, wrapped (`rows`) and as handed to the kernels (`raw`: every third id negative)."""
    g = torch.Generator().manual_seed(2000 + E)
    ends = {}
    for side, (n, hub, empty, first_neg) in SIDES.items():
        allowed = torch.tensor([r for r in range(n) if r not in empty and r != hub])
        if E == 0:
            rows = torch.zeros(0, dtype=torch.int64)
        elif E == 1:
            rows = torch.tensor([n - 3])
        else:
            rows = torch.cat([torch.full((300,), hub, dtype=torch.int64), allowed[torch.randint(0, allowed.numel(), (E - 300,), generator=g)]])
            rows = rows[torch.randperm(E, generator=g)]
        raw = rows.clone()
        raw[first_neg::3] -= n
        ends[side] = (rows, raw)
    return ends


def reference(x, w, g, src_rows, dst_rows, H, red, n_dst=N_DST):
    """float64 on the CPU: (out, dx, dw or None).  A row id of -1 marks a dropped edge end: a dropped source reads row 0 without a
    gradient, a dropped target takes no part."""
    E, C = src_rows.numel(), x.shape[1]
    xr = x.clone().requires_grad_(True)
    wr = None if w is None else w.clone().requires_grad_(True)
    msg = xr[src_rows.clamp(min=0)] * (src_rows >= 0).double().view(-1, 1) + (xr.detach()[0] * (src_rows < 0).double().view(-1, 1))
    if wr is not None:
        msg = (msg.view(E, H, C // H) * wr.view(E, H, 1)).reshape(E, C)
    live = dst_rows >= 0
    out = torch.zeros(n_dst, C, dtype=torch.float64).index_add_(0, dst_rows[live], msg[live])
    if red == "mean":
        out = out / torch.bincount(dst_rows[live], minlength=n_dst).clamp(min=1).double().view(-1, 1)
    grads = torch.autograd.grad(out, [xr] + ([] if wr is None else [wr]), g, allow_unused=True)
    dx = grads[0] if grads[0] is not None else torch.zeros_like(x)
    dw = None if wr is None else (grads[1] if grads[1] is not None else torch.zeros_like(w))
    return out.detach(), dx, dw


@functools.lru_cache(maxsize=None)
def make_case(E, C, H, form, integer):
    """x [N_SRC, C], w (None, [E] or [E, H]), g [N_DST, C] in float64 on the CPU and {reduce: reference}."""
    gen = torch.Generator().manual_seed(13 * E + 7 * C + H + (1 if integer else 0))
    if integer:   # small integers: every product and sum is exact in fp32
        x = torch.randint(-3, 4, (N_SRC, C), generator=gen).double()
        w = torch.randint(-2, 3, (E, H), generator=gen).double()
        g = torch.randint(-4, 5, (N_DST, C), generator=gen).double()
    else:
        x = torch.randn(N_SRC, C, generator=gen, dtype=torch.float64)
        w = torch.randn(E, H, generator=gen, dtype=torch.float64)
        g = torch.randn(N_DST, C, generator=gen, dtype=torch.float64)
    x, w, g = x.float().double(), w.float().double(), g.float().double()            # the reference sees the fp32 inputs
    if form is None:
        w = None
    elif form == "E":
        w = w.view(E)
    ends = make_ends(E)
    refs = {red: reference(x, w, g, ends["src"][0], ends["dst"][0], H, red) for red in REDUCES}
    return x, w, g, refs


def on_gpu(t, slice_pitch=False):
    if t is None:
        return None
    t = t.float()
    if slice_pitch and t.dim() == 2:   # a column slice: the pitch (C + 3) is no multiple of 4 and the base is 4 bytes off 16
        big = torch.zeros(t.shape[0], t.shape[1] + 3)
        big[:, 1:1 + t.shape[1]] = t
        return big.to(dev())[:, 1:1 + t.shape[1]]
    return t.to(dev())


def composed(x, src, dst, dim_size, weight, red, H=1):
    """The existing three steps: lift, multiply, aggregate."""
    plan_src = src if isinstance(src, ops.RowsPlan) else ops.rows_plan(src, x.shape[0])
    plan_dst = dst if isinstance(dst, ops.RowsPlan) else ops.rows_plan(dst, dim_size)
    msg = ops.take_rows(x, plan_src)
    if weight is not None:
        E, C = msg.shape
        msg = (msg.view(E, H, C // H) * weight.view(E, H, 1)).view(E, C)
    return ops.scatter(msg, None, dim_size, red, plan=plan_dst)


def run(fn, x, w, g, src, dst, red, H=1, n_dst=N_DST):
    """(out, dx, dw or None) of ``fn`` in {ops.gather_scatter, composed} on operands that keep their strides."""
    x = x.detach().requires_grad_(True)
    w = None if w is None else w.detach().requires_grad_(True)
    if fn is composed:
        out = composed(x, src, dst, n_dst, w, red, H)
    else:
        out = ops.gather_scatter(x, src, dst, n_dst, w, red)
    grads = torch.autograd.grad(out, [x] + ([] if w is None else [w]), g)
    return out.detach(), grads[0], (None if w is None else grads[1])


# ------------------------------------------------------------------------------------------------
# 1 + 2: the composition bit for bit, float64 within the bars
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,form", SHAPES)
def test_value_and_dx_equal_the_composition_and_float64(C, H, form):
    for E in ES:
        ends = make_ends(E)
        src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
        x64, w64, g64, refs = make_case(E, C, H, form, False)
        x, w, g = on_gpu(x64), on_gpu(w64), on_gpu(g64)
        for red in REDUCES:
            out, dx, dw = run(ops.gather_scatter, x, w, g, src, dst, red, H)
            c_out, c_dx, c_dw = run(composed, x, w, g, src, dst, red, H)
            assert out.shape == (N_DST, C) and dx.shape == (N_SRC, C)
            assert torch.equal(out, c_out), (E, red)
            assert torch.equal(dx, c_dx), (E, red)
            ref_out, ref_dx, ref_dw = refs[red]
            close(out, ref_out, 1e-5)
            close(dx, ref_dx, 1e-4)
            if w is not None:
                assert dw.shape == w.shape
                close(dw, ref_dw, 1e-4)
                close(c_dw, ref_dw, 1e-4)
            empty = torch.tensor(SIDES["dst"][2] if E else range(N_DST), device=dev())
            assert float(out[empty].abs().sum()) == 0.0                             # every row is written: a row no id names is 0


@pytest.mark.parametrize("C,H,form", [(4, 2, "EH"), (40, 5, "EH"), (260, 1, "E"), (3, 1, None)])
def test_small_integers_are_exact(C, H, form):
    ends = make_ends(700)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, w64, g64, refs = make_case(700, C, H, form, True)
    out, dx, dw = run(ops.gather_scatter, on_gpu(x64), on_gpu(w64), on_gpu(g64), src, dst, "sum", H)
    ref_out, ref_dx, ref_dw = refs["sum"]
    assert torch.equal(out.cpu().double(), ref_out) and torch.equal(dx.cpu().double(), ref_dx)
    if form is not None:
        assert torch.equal(dw.cpu().double(), ref_dw)
    # mean: one correctly rounded division of an exact sum by an exact count (53 >= 2 * 24 + 2 bits: rounding the float64 quotient
    # to fp32 is that division)
    out, _, _ = run(ops.gather_scatter, on_gpu(x64), on_gpu(w64), on_gpu(g64), src, dst, "mean", H)
    assert torch.equal(out.cpu(), refs["mean"][0].float())


def test_trailing_dimensions_and_the_three_dimensional_weight():
    E, Hh, D = 700, 2, 20
    ends = make_ends(E)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, w64, g64, refs = make_case(E, Hh * D, Hh, "EH", False)
    x, w, g = on_gpu(x64), on_gpu(w64), on_gpu(g64)
    flat = run(ops.gather_scatter, x, w, g, src, dst, "sum", Hh)
    x3 = x.view(N_SRC, Hh, D).detach().requires_grad_(True)
    w3 = w.view(E, Hh, 1).detach().requires_grad_(True)
    out = ops.gather_scatter(x3, src, dst, N_DST, w3, "add")
    dx, dw = torch.autograd.grad(out, (x3, w3), g.view(N_DST, Hh, D))
    assert out.shape == (N_DST, Hh, D) and dx.shape == x3.shape and dw.shape == w3.shape
    assert torch.equal(out.view(N_DST, -1), flat[0]) and torch.equal(dx.view(N_SRC, -1), flat[1]) and torch.equal(dw.view(E, Hh), flat[2])
    only_w = ops.gather_scatter(x.detach(), src, dst, N_DST, w3, "add")            # x outside autograd: only the weights get a gradient
    assert torch.equal(torch.autograd.grad(only_w, w3, g)[0], dw)


# ------------------------------------------------------------------------------------------------
# 3: the weights' gradient: two calls, one head against its column block, pitch and alignment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H", [(4, 2), (40, 5), (260, 5), (260, 2)])
def test_dweight_is_a_function_of_the_columns_and_heads_only(C, H):
    E, D = 700, C // H
    ends = make_ends(E)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, w64, g64, _ = make_case(E, C, H, "EH", False)
    x, w, g = on_gpu(x64), on_gpu(w64), on_gpu(g64)
    for red in REDUCES:
        out, dx, dw = run(ops.gather_scatter, x, w, g, src, dst, red, H)
        again = run(ops.gather_scatter, x, w, g, src, dst, red, H)
        assert torch.equal(dw, again[2]) and torch.equal(out, again[0]) and torch.equal(dx, again[1])
        for h in range(H):
            block = slice(h * D, (h + 1) * D)
            o1, dx1, dw1 = run(ops.gather_scatter, x[:, block], w[:, h], g[:, block], src, dst, red)
            assert torch.equal(dw1, dw[:, h]), (red, h)
            assert torch.equal(o1, out[:, block]) and torch.equal(dx1, dx[:, block])


@pytest.mark.parametrize("C,H,form", [(40, 5, "EH"), (260, 2, "EH"), (4, 1, "E"), (3, 1, "E")])
def test_a_pitched_and_misaligned_operand_gives_the_contiguous_bits(C, H, form):
    E = 700
    ends = make_ends(E)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, w64, g64, _ = make_case(E, C, H, form, False)
    for red in REDUCES:
        flat = run(ops.gather_scatter, on_gpu(x64), on_gpu(w64), on_gpu(g64), src, dst, red, H)
        xs, ws, gs = on_gpu(x64, True), on_gpu(w64, True), on_gpu(g64, True)
        assert xs.stride(0) % 4 != 0 and gs.stride(0) % 4 != 0 and not xs.is_contiguous()
        got = run(ops.gather_scatter, xs, ws, gs, src, dst, red, H)
        for a, b in zip(got, flat):
            assert torch.equal(a, b), red
        comp = run(composed, xs, ws, gs, src, dst, red, H)
        assert torch.equal(got[0], comp[0]) and torch.equal(got[1], comp[1])


# ------------------------------------------------------------------------------------------------
# 4: deferred plans, ids out of range on either side, no host read
# ------------------------------------------------------------------------------------------------
def host_read_spy(mp):
    reads = []
    for name in ("tolist", "item", "cpu"):
        real = getattr(torch.Tensor, name)
        mp.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **k: (reads.append(_name), _real(self, *a, **k))[1])
    return reads


def test_deferred_plans_drop_and_count_ids_out_of_range_without_a_host_read(monkeypatch):
    E, C, H = 700, 40, 5
    ends = make_ends(E)
    x64, w64, g64, _ = make_case(E, C, H, "EH", False)
    bad_src, bad_dst = torch.tensor([3, 200, 698]), torch.tensor([5, 200, 333, 699])     # (position 200: both ends are out of range)
    raw_s, raw_d = ends["src"][1].clone(), ends["dst"][1].clone()
    raw_s[bad_src] = torch.tensor([N_SRC, -N_SRC - 1, 10 ** 6])
    raw_d[bad_dst] = torch.tensor([N_DST, N_DST + 13, -N_DST - 2, 10 ** 6])
    rows_s, rows_d = ends["src"][0].clone(), ends["dst"][0].clone()
    rows_s[bad_src], rows_d[bad_dst] = -1, -1
    ops.rows_oob(dev())
    with pytest.raises(IndexError):
        ops.gather_scatter(on_gpu(x64), raw_s.to(dev()), ends["dst"][1].to(dev()), N_DST)      # host-checked plans raise, as before
    x, w, g = on_gpu(x64), on_gpu(w64), on_gpu(g64)
    ids_s, ids_d = raw_s.to(dev()), raw_d.to(dev())
    ops.rows_oob_counter(dev())
    torch.cuda.synchronize()
    results = {}
    with monkeypatch.context() as mp:
        reads = host_read_spy(mp)
        plan_s = ops.rows_plan(ids_s, N_SRC, check="deferred")
        plan_d = ops.rows_plan(ids_d, N_DST, check="deferred")
        for red in REDUCES:
            results[red] = (run(ops.gather_scatter, x, w, g, plan_s, plan_d, red, H), run(composed, x, w, g, plan_s, plan_d, red, H))
        assert reads == []
    for red in REDUCES:
        (out, dx, dw), (c_out, c_dx, c_dw) = results[red]
        assert torch.equal(out, c_out) and torch.equal(dx, c_dx)
        ref_out, ref_dx, ref_dw = reference(x64, w64, g64, rows_s, rows_d, H, red)
        close(out, ref_out, 1e-5)
        close(dx, ref_dx, 1e-4)
        close(dw, ref_dw, 1e-4)
        close(c_dw, ref_dw, 1e-4)
        assert float(dw[bad_dst.to(dev())].abs().max()) == 0.0                       # a dropped target: its weights get gradient 0
    assert ops.rows_oob(dev()) == bad_src.numel() + bad_dst.numel() and ops.rows_oob(dev()) == 0


# ------------------------------------------------------------------------------------------------
# 5: nn.MessagePassing
# ------------------------------------------------------------------------------------------------
def conv_edges():
    """[2, 700] over 37 nodes: the source and target columns of make_ends (wrapped)."""
    ends = make_ends(700)
    return torch.stack([ends["src"][0], ends["dst"][0]])


def count_plans(monkeypatch):
    built = []
    real = ops._rows_plan_launch
    monkeypatch.setattr(ops, "_rows_plan_launch", lambda ids, n: built.append(n) or real(ids, n))
    return built


@pytest.mark.parametrize("flow", ("source_to_target", "target_to_source"))
@pytest.mark.parametrize("aggr", ("add", "mean"))
def test_default_message_skips_the_lift(aggr, flow, monkeypatch):
    N, C = N_DST, 12
    ei = conv_edges().to(dev())
    j, i = (0, 1) if flow == "source_to_target" else (1, 0)
    gen = torch.Generator().manual_seed(21)
    x64, g64 = torch.randn(N, C, generator=gen, dtype=torch.float64), torch.randn(N, C, generator=gen, dtype=torch.float64)
    x, g = on_gpu(x64).requires_grad_(True), on_gpu(g64)
    plan_j, plan_i = ops.rows_plan(ei[j].contiguous(), N, check="deferred"), ops.rows_plan(ei[i].contiguous(), N, check="deferred")
    want = ops.scatter(ops.take_rows(x, plan_j), None, N, aggr, plan=plan_i)
    (want_dx,) = torch.autograd.grad(want, x, g)

    def refuse(*a, **k):
        raise AssertionError("the default message must not lift x_j")
    monkeypatch.setattr(ops._TakeRows, "apply", refuse)
    built = count_plans(monkeypatch)
    out = PN.MessagePassing(aggr=aggr, flow=flow).propagate(ei, x=x)
    (dx,) = torch.autograd.grad(out, x, g)
    assert len(built) == 2, built
    assert torch.equal(out, want) and torch.equal(dx, want_dx)
    ref_out, ref_dx, _ = reference(x64.float().double(), None, g64.float().double(), ei[j].cpu(), ei[i].cpu(), 1, "sum" if aggr == "add" else aggr,
                                   n_dst=N)
    close(out, ref_out, 1e-5)
    close(dx, ref_dx, 1e-4)
    assert not PN._MP_RUNNING


class GCNStyle(PN.MessagePassing):
    """PyG's own ``GCNConv.message``."""

    def __init__(self, aggr="add", bias=None):
        super().__init__(aggr=aggr)
        self.shift = bias

    def forward(self, x, edge_index, edge_weight):
        return self.propagate(edge_index, x=x, edge_weight=edge_weight)

    def message(self, x_j, edge_weight):
        msg = edge_weight.view(-1, 1) * x_j
        return msg if self.shift is None else msg + self.shift


class TwoHeadAttention(PN.MessagePassing):
    """PyG's ``GATConv.message`` on given scores: a softmax over the target's edges per head, then the weighted lift."""

    def __init__(self):
        super().__init__(aggr="add", node_dim=0)

    def forward(self, x, edge_index, alpha):
        return self.propagate(edge_index, x=x.view(-1, 2, 20), alpha=alpha).reshape(-1, 40)

    def message(self, x_j, alpha, index, ptr, size_i):
        alpha = utils.softmax(alpha, index, ptr, size_i)
        return x_j * alpha.unsqueeze(-1)


def load_accel():
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_gs", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    return accel


def conv_inputs(kind):
    N, E = N_DST, 700
    gen = torch.Generator().manual_seed(31)
    x64 = torch.randn(N, 40, generator=gen, dtype=torch.float64).float().double()
    e64 = torch.randn(E, 1 if kind == "gcn" else 2, generator=gen, dtype=torch.float64).float().double()
    g64 = torch.randn(N, 40, generator=gen, dtype=torch.float64).float().double()
    return x64, (e64.view(E) if kind == "gcn" else e64), g64


def conv_reference(kind, x64, e64, g64, ei, aggr="add"):
    """The two convs restated in float64 on the CPU: (out, dx, d edge tensor)."""
    N, E = x64.shape[0], ei.shape[1]
    x, e = x64.clone().requires_grad_(True), e64.clone().requires_grad_(True)
    if kind == "gcn":
        msg = e.view(-1, 1) * x[ei[0]]
    else:
        M = torch.zeros(N, 2, dtype=torch.float64).scatter_reduce(0, ei[1].view(-1, 1).expand(-1, 2), e.detach(), "amax", include_self=False)
        ex = (e - M[ei[1]]).exp()
        alpha = ex / (torch.zeros(N, 2, dtype=torch.float64).index_add_(0, ei[1], ex)[ei[1]] + 1e-16)
        msg = (x.view(N, 2, 20)[ei[0]] * alpha.unsqueeze(-1)).reshape(E, 40)
    out = torch.zeros(N, 40, dtype=torch.float64).index_add_(0, ei[1], msg)
    if aggr == "mean":
        out = out / torch.bincount(ei[1], minlength=N).clamp(min=1).double().view(-1, 1)
    dx, de = torch.autograd.grad(out, (x, e), g64)
    return out.detach(), dx, de


def conv_step(conv, x64, e64, g64, ei):
    x, e = on_gpu(x64).requires_grad_(True), on_gpu(e64).requires_grad_(True)
    out = conv(x, ei, e)
    dx, de = torch.autograd.grad(out, (x, e), on_gpu(g64))
    return out.detach(), dx, de


@pytest.mark.parametrize("kind,aggr", [("gcn", "add"), ("gcn", "mean"), ("attention", "add")])
def test_under_accel_no_edge_tensor_is_formed(kind, aggr, monkeypatch):
    ei = conv_edges()
    x64, e64, g64 = conv_inputs(kind)
    conv = GCNStyle(aggr) if kind == "gcn" else TwoHeadAttention()
    plain = conv_step(conv, x64, e64, g64, ei.to(dev()))
    ref = conv_reference(kind, x64, e64, g64, ei, aggr)
    close(plain[0], ref[0], 1e-5)
    accel = load_accel()

    def refuse(*a, **k):
        raise AssertionError("an [E, C] message tensor was aggregated")
    with monkeypatch.context() as mp:
        mp.setattr(ops._Scatter, "apply", refuse)
        mp.setattr(ops._TakeRows, "apply", refuse)
        built = count_plans(mp)
        with accel.scope():
            fused = conv_step(conv, x64, e64, g64, ei.to(dev()))
        assert len(built) <= 2, built
    assert not lazy.ACCEL_ACTIVE and not PN._MP_RUNNING
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])      # out and dx: bit for bit
    close(fused[0], ref[0], 1e-5)
    close(fused[1], ref[1], 1e-4)
    close(fused[2], ref[2], 1e-4)                                                   # dweight / dalpha: the float64 bar
    close(plain[2], ref[2], 1e-4)


@pytest.mark.parametrize("conv", ("max", "bias"))
def test_under_accel_other_messages_and_aggregations_materialise(conv):
    ei = conv_edges().to(dev())
    x64, e64, g64 = conv_inputs("gcn")
    conv = GCNStyle("max") if conv == "max" else GCNStyle("add", bias=0.25)
    plain = conv_step(conv, x64, e64, g64, ei)
    accel = load_accel()
    with accel.scope():
        under = conv_step(conv, x64, e64, g64, ei)
    for a, b in zip(under, plain):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# 6: a captured step
# ------------------------------------------------------------------------------------------------
def test_a_captured_step_of_the_gcn_style_conv_replays_to_the_eager_result():
    ei = conv_edges().to(dev())
    x64, e64, g64 = conv_inputs("gcn")
    x, w = on_gpu(x64), on_gpu(e64)
    conv = GCNStyle("mean")
    accel = load_accel()
    ops.rows_oob(dev())
    with accel.scope(), torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            conv(x, ei, w)                                                          # warm-up
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = conv(x, ei, w)                                                      # builds its deferred plans inside the capture
        x.copy_(torch.randn(x.shape, device=dev()))
        w.copy_(torch.randn(w.shape, device=dev()))
        graph.replay()
        torch.cuda.synchronize()
        eager = conv(x, ei, w)
    assert torch.equal(y, eager)
    assert torch.equal(eager, conv(x, ei, w))                                       # and outside accel: the composition
    close(y, conv_reference("gcn", x.double().cpu(), w.double().cpu(), g64, ei.cpu(), "mean")[0], 1e-5)
    assert ops.rows_oob(dev()) == 0
