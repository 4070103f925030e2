"""The fused gather-add-activate-aggregate on the device (csrc/gather_edge_scatter.hip, ``ops.gather_add_scatter``), its two backward
kernels, and what is built on it: ``nn.GINConv`` / ``nn.GINEConv``, ``lazy.LazyEdgeRows`` under ``accel``, the graph-level pools,
``Batch.from_data_list`` and a ``models.MolGNN`` training step.

The defining property is BIT-EQUALITY with the existing composition ``ops.scatter(torch.relu(ops.take_rows(x, plan_src) + edge), None,
dim_size, reduce, plan=plan_dst)`` -- value, dx and dedge -- asserted with ``torch.equal``.  Against float64 on the CPU (``index_add_``,
division by counts, torch's relu) the bars are those of tests/test_gpu_gather_scatter.py for the same kind of sums: forward rtol 1e-5,
atol 1e-5 * max|ref|; gradients rtol 1e-4, atol 1e-4 * max|ref|.  Small-integer inputs are exact.  The gate needs no excluded cases: the
fp32 sum of two fp32 numbers has the sign of the exact sum and is zero only when the exact sum is, so fp32 and float64 agree on every
mask; positions with ``edge[p] == -x[src[p]]`` exactly (pre-activation 0) pin relu'(0) = 0.

Index design, on both endpoints independently: 41 target rows and 29 source rows; a hub named 300 times on each side (over two
EGNN_ROWS_SUM_CHUNKs of 128: the workspace merge runs), runs of exactly 127, 128 and 129, rows never named, every third id negative,
E in 0 | 1 | 700 in random order."""
import functools
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from efficient_gnns_amd import data, lazy, models, ops, saint
from efficient_gnns_amd import nn as PN
from conftest import ROOT

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 41, 29
# rows, hub, (row with a run of 127, of 128, of 129), never named, first negative position
SIDES = {"dst": (N_DST, 7, (11, 12, 13), (0, 1, 2, 3, 4, 40), 0), "src": (N_SRC, 4, (20, 5, 17), (0, 9, 28), 1)}
ES = (0, 1, 700)
CS = (1, 3, 4, 40, 260, 300)
ACTS = ("relu", None)
REDUCES = ("sum", "mean")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def close(got, ref, rtol, scale=None):
    ref = ref.detach().double().cpu()
    atol = rtol * float((ref if scale is None else scale).abs().max()) if ref.numel() else 0.0
    torch.testing.assert_close(got.detach().double().cpu(), ref, rtol=rtol, atol=atol)


@functools.lru_cache(maxsize=None)
def make_ends(E):
    """{side: (rows, raw)}: [E] int64 on the CPU, wrapped (`rows`) and as handed to the kernels (`raw`: every third id negative)."""
    g = torch.Generator().manual_seed(4000 + E)
    ends = {}
    for side, (n, hub, runs, empty, first_neg) in SIDES.items():
        allowed = torch.tensor([r for r in range(n) if r not in empty and r != hub and r not in runs])
        if E == 0:
            rows = torch.zeros(0, dtype=torch.int64)
        elif E == 1:
            rows = torch.tensor([n - 3])
        else:
            fixed = [torch.full((300,), hub, dtype=torch.int64)] + [torch.full((k,), r, dtype=torch.int64) for r, k in zip(runs, (127, 128, 129))]
            rest = E - sum(t.numel() for t in fixed)
            rows = torch.cat(fixed + [allowed[torch.randint(0, allowed.numel(), (rest,), generator=g)]])
            rows = rows[torch.randperm(E, generator=g)]
        raw = rows.clone()
        raw[first_neg::3] -= n
        ends[side] = (rows, raw)
    return ends


def reference(x, e, g, src_rows, dst_rows, act, red, n_dst=N_DST):
    """float64 on the CPU: (out, dx, dedge).  A row id of -1 marks a dropped edge end: a dropped source reads row 0 without a gradient
    for x (the edge row keeps its own), a dropped target takes no part."""
    xr, er = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    kept = (src_rows >= 0).double().view(-1, 1)
    msg = xr[src_rows.clamp(min=0)] * kept + xr.detach()[:1] * (1 - kept) + er if x.shape[0] else er * 1
    if act == "relu":
        msg = torch.relu(msg)
    live = dst_rows >= 0
    out = torch.zeros(n_dst, x.shape[1], dtype=torch.float64).index_add_(0, dst_rows[live], msg[live])
    if red == "mean":
        out = out / torch.bincount(dst_rows[live], minlength=n_dst).clamp(min=1).double().view(-1, 1)
    dx, de = torch.autograd.grad(out, (xr, er), g, allow_unused=True)
    return out.detach(), (dx if dx is not None else torch.zeros_like(x)), (de if de is not None else torch.zeros_like(e))


@functools.lru_cache(maxsize=None)
def make_case(E, C, integer):
    """x [N_SRC, C], e [E, C], g [N_DST, C] in float64 on the CPU (fp32 values) and {(act, reduce): reference}.  Every seventh position
    has e[p] = -x[src[p]] exactly: pre-activation 0."""
    gen = torch.Generator().manual_seed(17 * E + 5 * C + (1 if integer else 0))
    if integer:   # small integers: every sum is exact in fp32
        x = torch.randint(-3, 4, (N_SRC, C), generator=gen).double()
        e = torch.randint(-3, 4, (E, C), generator=gen).double()
        g = torch.randint(-4, 5, (N_DST, C), generator=gen).double()
    else:
        x = torch.randn(N_SRC, C, generator=gen, dtype=torch.float64)
        e = torch.randn(E, C, generator=gen, dtype=torch.float64)
        g = torch.randn(N_DST, C, generator=gen, dtype=torch.float64)
    x, e, g = x.float().double(), e.float().double(), g.float().double()            # the reference sees the fp32 inputs
    ends = make_ends(E)
    if E:
        e[::7] = -x[ends["src"][0][::7]]
    refs = {(act, red): reference(x, e, g, ends["src"][0], ends["dst"][0], act, red) for act in ACTS for red in REDUCES}
    return x, e, g, refs


def on_gpu(t, slice_pitch=False):
    t = t.float()
    if slice_pitch and t.dim() == 2:   # a column slice: the pitch (C + 3) is no multiple of 4 and the base is 4 bytes off 16
        big = torch.zeros(t.shape[0], t.shape[1] + 3)
        big[:, 1:1 + t.shape[1]] = t
        return big.to(dev())[:, 1:1 + t.shape[1]]
    return t.to(dev())


def composed(x, src, dst, dim_size, edge, act, red):
    """The existing four steps: lift, add, activate, aggregate."""
    plan_src = src if isinstance(src, ops.RowsPlan) else ops.rows_plan(src, x.shape[0])
    plan_dst = dst if isinstance(dst, ops.RowsPlan) else ops.rows_plan(dst, dim_size)
    msg = ops.take_rows(x, plan_src) + edge
    return ops.scatter(torch.relu(msg) if act == "relu" else msg, None, dim_size, red, plan=plan_dst)


def run(fn, x, e, g, src, dst, act, red, n_dst=N_DST):
    """(out, dx, dedge) of ``fn`` in {ops.gather_add_scatter, composed} on operands that keep their strides."""
    x, e = x.detach().requires_grad_(True), e.detach().requires_grad_(True)
    out = composed(x, src, dst, n_dst, e, act, red) if fn is composed else ops.gather_add_scatter(x, src, dst, n_dst, e, act, red)
    dx, de = torch.autograd.grad(out, (x, e), g)
    return out.detach(), dx, de


# ------------------------------------------------------------------------------------------------
# 1 + 2: the composition bit for bit, float64 within the bars
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_value_dx_and_dedge_equal_the_composition_and_float64(C):
    for E in ES:
        ends = make_ends(E)
        src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
        x64, e64, g64, refs = make_case(E, C, False)
        x, e, g = on_gpu(x64), on_gpu(e64), on_gpu(g64)
        for act in ACTS:
            for red in REDUCES:
                out, dx, de = run(ops.gather_add_scatter, x, e, g, src, dst, act, red)
                c_out, c_dx, c_de = run(composed, x, e, g, src, dst, act, red)
                assert out.shape == (N_DST, C) and dx.shape == (N_SRC, C) and de.shape == (E, C)
                assert torch.equal(out, c_out), (E, act, red)
                assert torch.equal(dx, c_dx), (E, act, red)
                assert torch.equal(de, c_de), (E, act, red)
                again = run(ops.gather_add_scatter, x, e, g, src, dst, act, red)
                assert all(torch.equal(a, b) for a, b in zip(again, (out, dx, de))), (E, act, red)    # two calls are bit-equal
                ref_out, ref_dx, ref_de = refs[(act, red)]
                close(out, ref_out, 1e-5)
                close(dx, ref_dx, 1e-4)
                close(de, ref_de, 1e-4)
                if E and act == "relu":
                    assert float(de[::7].abs().max()) == 0.0                        # pre-activation 0: relu'(0) = 0
                empty = torch.tensor(SIDES["dst"][3] if E else range(N_DST), device=dev())
                assert float(out[empty].abs().sum()) == 0.0                         # every row is written: a row no id names is 0


@pytest.mark.parametrize("C", (3, 4, 260))
def test_small_integers_are_exact(C):
    ends = make_ends(700)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, e64, g64, refs = make_case(700, C, True)
    for act in ACTS:
        out, dx, de = run(ops.gather_add_scatter, on_gpu(x64), on_gpu(e64), on_gpu(g64), src, dst, act, "sum")
        ref_out, ref_dx, ref_de = refs[(act, "sum")]
        assert torch.equal(out.cpu().double(), ref_out) and torch.equal(dx.cpu().double(), ref_dx) and torch.equal(de.cpu().double(), ref_de)
        # mean: one correctly rounded division of an exact sum by an exact count (rounding the float64 quotient to fp32 is that division)
        out, _, _ = run(ops.gather_add_scatter, on_gpu(x64), on_gpu(e64), on_gpu(g64), src, dst, act, "mean")
        assert torch.equal(out.cpu(), refs[(act, "mean")][0].float())


@pytest.mark.parametrize("C", (3, 4, 40))
def test_a_pitched_and_misaligned_operand_gives_the_contiguous_bits(C):
    E = 700
    ends = make_ends(E)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, e64, g64, _ = make_case(E, C, False)
    for act in ACTS:
        for red in REDUCES:
            flat = run(ops.gather_add_scatter, on_gpu(x64), on_gpu(e64), on_gpu(g64), src, dst, act, red)
            xs, es, gs = on_gpu(x64, True), on_gpu(e64, True), on_gpu(g64, True)
            assert xs.stride(0) % 4 != 0 and es.stride(0) % 4 != 0 and not xs.is_contiguous()
            got = run(ops.gather_add_scatter, xs, es, gs, src, dst, act, red)
            for a, b in zip(got, flat):
                assert torch.equal(a, b), (act, red)
            only_edge = run(ops.gather_add_scatter, on_gpu(x64), es, on_gpu(g64), src, dst, act, red)     # one scalar operand decides the path
            for a, b in zip(only_edge, flat):
                assert torch.equal(a, b), (act, red)


def test_the_switch_off_runs_the_composition(monkeypatch):
    ends = make_ends(700)
    src, dst = ends["src"][1].to(dev()), ends["dst"][1].to(dev())
    x64, e64, g64, _ = make_case(700, 40, False)
    x, e, g = on_gpu(x64), on_gpu(e64), on_gpu(g64)
    fused = run(ops.gather_add_scatter, x, e, g, src, dst, "relu", "mean")

    def refuse(*a, **k):
        raise AssertionError("FUSE_EDGE_ROWS is off: the fused walk must not run")
    monkeypatch.setattr(ops, "FUSE_EDGE_ROWS", False)
    monkeypatch.setattr(ops._GatherAddScatter, "apply", refuse)
    off = run(ops.gather_add_scatter, x, e, g, src, dst, "relu", "mean")
    assert all(torch.equal(a, b) for a, b in zip(fused, off))


def test_cpu_tensors_are_refused():
    from efficient_gnns_amd._lib import HipExtensionError
    with pytest.raises(HipExtensionError):
        ops.gather_add_scatter(torch.zeros(5, 8), torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int64), 4, torch.zeros(6, 8))


# ------------------------------------------------------------------------------------------------
# 3: deferred plans, ids out of range on either side
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (40, 3))
def test_deferred_plans_drop_and_count_ids_out_of_range(C):
    E = 700
    ends = make_ends(E)
    x64, e64, g64, _ = make_case(E, C, False)
    bad_src, bad_dst = torch.tensor([3, 200, 698]), torch.tensor([5, 200, 333, 699])     # (position 200: both ends are out of range)
    raw_s, raw_d = ends["src"][1].clone(), ends["dst"][1].clone()
    raw_s[bad_src] = torch.tensor([N_SRC, -N_SRC - 1, 10 ** 6])
    raw_d[bad_dst] = torch.tensor([N_DST, N_DST + 13, -N_DST - 2, 10 ** 6])
    rows_s, rows_d = ends["src"][0].clone(), ends["dst"][0].clone()
    rows_s[bad_src], rows_d[bad_dst] = -1, -1
    e64 = e64.clone()
    e64[bad_src] = -x64[0]                                                            # a dropped source reads row 0: pre-activation 0 there too
    ops.rows_oob(dev())
    with pytest.raises(IndexError):
        ops.gather_add_scatter(on_gpu(x64), raw_s.to(dev()), ends["dst"][1].to(dev()), N_DST, on_gpu(e64))    # host-checked plans raise
    x, e, g = on_gpu(x64), on_gpu(e64), on_gpu(g64)
    plan_s = ops.rows_plan(raw_s.to(dev()), N_SRC, check="deferred")
    plan_d = ops.rows_plan(raw_d.to(dev()), N_DST, check="deferred")
    for act in ACTS:
        for red in REDUCES:
            out, dx, de = run(ops.gather_add_scatter, x, e, g, plan_s, plan_d, act, red)
            c_out, c_dx, c_de = run(composed, x, e, g, plan_s, plan_d, act, red)
            assert torch.equal(out, c_out) and torch.equal(dx, c_dx) and torch.equal(de, c_de), (act, red)
            ref_out, ref_dx, ref_de = reference(x64, e64, g64, rows_s, rows_d, act, red)
            close(out, ref_out, 1e-5)
            close(dx, ref_dx, 1e-4)
            close(de, ref_de, 1e-4)
            assert float(de[bad_dst.to(dev())].abs().max()) == 0.0                   # a dropped target: its edge row gets gradient 0
    assert ops.rows_oob(dev()) == bad_src.numel() + bad_dst.numel() and ops.rows_oob(dev()) == 0


# ------------------------------------------------------------------------------------------------
# 4: nn.GINConv / nn.GINEConv and the routes that reach the fused walk
# ------------------------------------------------------------------------------------------------
def conv_edges():
    """[2, 700] over 41 nodes: the source and target columns of make_ends (wrapped)."""
    ends = make_ends(700)
    return torch.stack([ends["src"][0], ends["dst"][0]])


def count_calls(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)
    monkeypatch.setattr(owner, name, lambda *a, **k: calls.append(name) or real(*a, **k))
    return calls


def mlp(C, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(C, 2 * C), torch.nn.ReLU(), torch.nn.Linear(2 * C, C)).to(dev())


def gin_reference(conv, x64, e64, g64, ei, eps_grad):
    """The conv restated in float64 on the CPU: (out, [dx, dedge?, deps?, *dparams of nn])."""
    x = x64.clone().requires_grad_(True)
    e = None if e64 is None else e64.clone().requires_grad_(True)
    eps = conv.eps.detach().double().cpu().requires_grad_(eps_grad)
    params = [p.detach().double().cpu().requires_grad_(True) for p in conv.nn.parameters()]
    msg = x[ei[0]] if e is None else torch.relu(x[ei[0]] + e)
    h = (1 + eps) * x + torch.zeros_like(x).index_add_(0, ei[1], msg)
    out = F.linear(torch.relu(F.linear(h, params[0], params[1])), params[2], params[3])
    wrt = [x] + ([] if e is None else [e]) + ([eps] if eps_grad else []) + params
    return out.detach(), torch.autograd.grad(out, wrt, g64)


@pytest.mark.parametrize("kind", ("gin", "gine"))
@pytest.mark.parametrize("train_eps", (False, True))
def test_gin_and_gine_forward_and_backward_against_float64(kind, train_eps, monkeypatch):
    N, C = N_DST, 40
    ei = conv_edges()
    gen = torch.Generator().manual_seed(51)
    x64 = torch.randn(N, C, generator=gen, dtype=torch.float64).float().double()
    e64 = torch.randn(700, C, generator=gen, dtype=torch.float64).float().double() if kind == "gine" else None
    g64 = torch.randn(N, C, generator=gen, dtype=torch.float64).float().double()
    conv = (PN.GINEConv if kind == "gine" else PN.GINConv)(mlp(C, 3), eps=0.25, train_eps=train_eps).to(dev())
    assert isinstance(conv.eps, torch.nn.Parameter) == train_eps
    x = on_gpu(x64).requires_grad_(True)
    e = None if e64 is None else on_gpu(e64).requires_grad_(True)
    built = count_calls(monkeypatch, ops, "_rows_plan_launch")
    fused = count_calls(monkeypatch, ops, "gather_add_scatter" if kind == "gine" else "gather_scatter")
    out = conv(x, ei.to(dev())) if e is None else conv(x, ei.to(dev()), e)
    assert fused and len(built) == 2, (fused, built)
    wrt = [x] + ([] if e is None else [e]) + ([conv.eps] if train_eps else []) + list(conv.nn.parameters())
    grads = torch.autograd.grad(out, wrt, on_gpu(g64))
    ref_out, ref_grads = gin_reference(conv, x64, e64, g64, ei, train_eps)
    close(out, ref_out, 1e-5)
    for got, ref in zip(grads, ref_grads):
        close(got, ref, 1e-4)
    assert not PN._MP_RUNNING
    pair = conv((x, x), ei.to(dev())) if e is None else conv((x, x), ei.to(dev()), e)
    assert torch.equal(pair, out)


class OwnMessage(PN.GINEConv):
    def message(self, x_j, edge_attr):
        return torch.relu(x_j + edge_attr)


def test_a_subclass_overriding_message_takes_the_general_path(monkeypatch):
    N, C = N_DST, 40
    ei = conv_edges().to(dev())
    gen = torch.Generator().manual_seed(52)
    x = torch.randn(N, C, generator=gen).to(dev()).requires_grad_(True)
    e = torch.randn(700, C, generator=gen).to(dev()).requires_grad_(True)
    g = torch.randn(N, C, generator=gen).to(dev())
    want = PN.GINEConv(mlp(C, 4)).to(dev())(x, ei, e)
    want_grads = torch.autograd.grad(want, (x, e), g)
    calls = count_calls(monkeypatch, ops, "gather_add_scatter")
    out = OwnMessage(mlp(C, 4)).to(dev())(x, ei, e)
    grads = torch.autograd.grad(out, (x, e), g)
    assert not calls
    assert torch.equal(out, want) and all(torch.equal(a, b) for a, b in zip(grads, want_grads))
    with pytest.raises(ValueError, match="widths"):
        PN.GINEConv(mlp(C, 4)).to(dev())(x, ei, e[:, :8])


class UserEdgeConv(PN.MessagePassing):
    """A user's own edge-feature conv, spelled as PyG documents it."""

    def forward(self, x, edge_index, edge_attr):
        return self.propagate(edge_index, x=x, edge_attr=edge_attr)

    def message(self, x_j, edge_attr):
        return F.relu(x_j + edge_attr)


def load_accel():
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_gine", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    return accel


@pytest.mark.parametrize("aggr", ("add", "mean"))
def test_under_accel_a_user_conv_is_the_fused_walk_and_forms_no_edge_tensor(aggr, monkeypatch):
    N, E, C = 3000, 20000, 64                                                       # E C 4 = 5 MB: far above the plans and workspaces
    gen = torch.Generator().manual_seed(53)
    ei = torch.randint(0, N, (2, E), generator=gen).to(dev())
    x = torch.randn(N, C, generator=gen).to(dev()).requires_grad_(True)
    e = torch.randn(E, C, generator=gen).to(dev()).requires_grad_(True)
    g = torch.randn(N, C, generator=gen).to(dev())
    conv = UserEdgeConv(aggr=aggr)
    plain = conv(x, ei, e)
    plain_grads = torch.autograd.grad(plain, (x, e), g)
    gine = PN.GINEConv(torch.nn.Identity(), aggr=aggr)._fused(x, x, ei, e, None)    # GINEConv's aggregation
    gine_grads = torch.autograd.grad(gine, (x, e), g)
    accel = load_accel()
    calls = count_calls(monkeypatch, ops, "gather_add_scatter")
    with accel.scope():
        conv(x, ei, e)                                                              # (warm-up: the allocator's pools, the counters)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = conv(x, ei, e)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        grads = torch.autograd.grad(out, (x, e), g)
    assert len(calls) == 2 and not lazy.ACCEL_ACTIVE and not PN._MP_RUNNING
    assert peak < E * C * 4, (peak, E * C * 4)                                      # no [E, C] tensor in the forward
    assert torch.equal(out, gine) and all(torch.equal(a, b) for a, b in zip(grads, gine_grads))
    assert torch.equal(out, plain) and all(torch.equal(a, b) for a, b in zip(grads, plain_grads))


# ------------------------------------------------------------------------------------------------
# 5: pools and batches
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("add", "mean", "max"))
def test_global_pools_against_float64(name):
    pool = {"add": PN.global_add_pool, "mean": PN.global_mean_pool, "max": PN.global_max_pool}[name]
    sizes = [5, 1, 0, 130, 7]                                                       # graph 2 owns no node
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    gen = torch.Generator().manual_seed(61)
    x64 = torch.randn(batch.numel(), 33, generator=gen, dtype=torch.float64).float().double()
    g64 = torch.randn(len(sizes), 33, generator=gen, dtype=torch.float64).float().double()
    xr = x64.clone().requires_grad_(True)
    ref = torch.zeros(len(sizes), 33, dtype=torch.float64)
    for k, n in enumerate(sizes):
        rows = xr[batch == k]
        if n:
            ref = ref + F.one_hot(torch.tensor(k), len(sizes)).double().view(-1, 1) * {"add": rows.sum(0), "mean": rows.mean(0), "max": rows.max(0)[0]}[name]
    (ref_dx,) = torch.autograd.grad(ref, xr, g64)
    for size in (len(sizes), None):
        x = on_gpu(x64).requires_grad_(True)
        out = pool(x, batch.to(dev()), size)
        (dx,) = torch.autograd.grad(out, x, on_gpu(g64))
        assert out.shape == (len(sizes), 33) and float(out[2].detach().abs().sum()) == 0.0
        close(out, ref, 1e-5)
        close(dx, ref_dx, 1e-4)
    assert pool(on_gpu(x64), batch.to(dev()), 7).shape == (7, 33)


def test_batch_from_device_graphs_equals_the_cpu_result():
    graphs = data.molhiv_like(6, seed=3)
    graphs.insert(2, saint.Data(x=torch.zeros(0, 9, dtype=torch.int64), edge_index=torch.zeros(2, 0, dtype=torch.int64),
                                edge_attr=torch.zeros(0, 3, dtype=torch.int64), y=torch.zeros(1, 1), num_nodes=0))
    cpu = saint.Batch.from_data_list(graphs)
    gpu = saint.Batch.from_data_list([saint.Data(**{k: v for k, v in vars(g).items()}).to(dev()) for g in graphs])
    for key in ("x", "edge_index", "edge_attr", "y", "batch", "ptr"):
        assert getattr(gpu, key).is_cuda and torch.equal(getattr(gpu, key).cpu(), getattr(cpu, key)), key
    assert gpu.num_graphs == cpu.num_graphs == 7


# ------------------------------------------------------------------------------------------------
# 6: a MolGNN training step
# ------------------------------------------------------------------------------------------------
def molgnn_float64(model, batch, mode, hp, teacher_logits):
    """The model restated in float64 on the CPU (training-mode BatchNorm, dropout 0): (loss, {parameter name: gradient})."""
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters()}
    B = {k: v.detach().double().cpu() for k, v in model.named_buffers()}

    def enc(prefix, attr):
        return sum(P[f"{prefix}.embeddings.{k}.weight"][attr[:, k]] for k in range(attr.shape[1]))

    def bn(prefix, h):
        return F.batch_norm(h, None, None, P[prefix + ".weight"], P[prefix + ".bias"], True, 0.0, 1e-5)
    ei, L = batch.edge_index, model.num_layers
    h = enc("atom_encoder", batch.x)
    for l in range(L):
        msg = torch.relu(h[ei[0]] + enc(f"bond_encoders.{l}", batch.edge_attr)) if model.conv == "gine" else h[ei[0]]
        eps = B[f"convs.{l}.eps"]
        z = torch.zeros_like(h).index_add_(0, ei[1], msg) + (1 + eps) * h
        z = F.linear(z, P[f"convs.{l}.nn.0.weight"], P[f"convs.{l}.nn.0.bias"])
        z = torch.relu(bn(f"convs.{l}.nn.1", z))
        h = bn(f"bns.{l}", F.linear(z, P[f"convs.{l}.nn.3.weight"], P[f"convs.{l}.nn.3.bias"]))
        if l != L - 1:
            h = torch.relu(h)
    G = batch.num_graphs
    pooled = torch.zeros(G, h.shape[1], dtype=torch.float64).index_add_(0, batch.batch, h)
    pooled = pooled / torch.bincount(batch.batch, minlength=G).clamp(min=1).double().view(-1, 1)
    out = F.linear(pooled, P["graph_pred_linear.weight"], P["graph_pred_linear.bias"])
    y = batch.y.double().view(out.shape)
    cls = F.binary_cross_entropy_with_logits(out, y)
    if mode == "supervised":
        loss = cls
    else:    # the multi-label KD of the PPI scripts: BCE against the teacher's probabilities, the temperature only scales the term
        kd = F.binary_cross_entropy_with_logits(out, torch.sigmoid(teacher_logits.double().view(out.shape)))
        loss = kd * (hp["alpha"] * hp["kd_T"] * hp["kd_T"]) + cls * (1 - hp["alpha"])
    names = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in names])
    return loss.detach(), dict(zip(names, grads))


@functools.lru_cache(maxsize=None)
def mol_batch():
    return saint.Batch.from_data_list(data.molhiv_like(24, seed=1))


@pytest.mark.parametrize("conv", ("gin", "gine"))
@pytest.mark.parametrize("mode", ("supervised", "kd"))
def test_molgnn_training_step_against_float64(conv, mode):
    cpu = mol_batch()
    batch = saint.Batch.from_data_list(data.molhiv_like(24, seed=1)).to(dev())
    batch.num_graphs = cpu.num_graphs
    hp = {"alpha": 0.5, "kd_T": 2.0}
    teacher = torch.randn(cpu.num_graphs, 1, generator=torch.Generator().manual_seed(71))
    torch.manual_seed(72)
    model = models.MolGNN(conv, num_layers=2, emb_dim=32, dropout=0.0).to(dev()).train()

    def step():
        model.zero_grad()
        loss, loss_cls, loss_aux = models.mol_batch_loss(model, batch, mode, hp, teacher.to(dev()) if mode == "kd" else None)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}
    loss, grads = step()
    ref_loss, ref_grads = molgnn_float64(model, cpu, mode, hp, teacher)
    assert model.out_feat.shape == (cpu.num_graphs, 32)
    close(loss, ref_loss, 1e-4)
    assert set(grads) == set(ref_grads)
    for k in grads:
        assert torch.isfinite(grads[k]).all(), k
        # A Linear bias in front of a BatchNorm has gradient 0 in exact arithmetic (the columns of the BatchNorm's input gradient sum
        # to 0), so max|ref| is rounding noise and no scale: such a bias is the column sum of the same dZ whose product with the layer
        # input is the weight's gradient, and is held to the bar at the weight gradient's scale.
        before_bn = k.endswith((".nn.0.bias", ".nn.3.bias"))
        close(grads[k], ref_grads[k], 1e-4, scale=ref_grads[k[:-4] + "weight"] if before_bn else None)
    loss2, grads2 = step()
    assert torch.equal(loss, loss2) and all(torch.equal(grads[k], grads2[k]) for k in grads)     # two runs are bit-equal
    # with dropout: finite, and reproducible under the same seed
    model.dropout = 0.5
    torch.manual_seed(5)
    a = step()
    torch.manual_seed(5)
    b = step()
    assert torch.isfinite(a[0]) and all(torch.isfinite(v).all() for v in a[1].values())
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    with pytest.raises(NotImplementedError):
        models.mol_batch_loss(model, batch, "fitnet", hp)


# ------------------------------------------------------------------------------------------------
# 7: under accel the convs are fed DEFERRED activations (BatchNorm1d -> relu -> dropout hands out a lazy.LazyBnAct)
# ------------------------------------------------------------------------------------------------
def spy_node_inputs(monkeypatch):
    """The types of what reaches GINConv / GINEConv as `x`."""
    seen = []
    real = PN._GINBase._node_pair
    monkeypatch.setattr(PN._GINBase, "_node_pair", staticmethod(lambda x, who: seen.append(type(x)) or real(x, who)))
    return seen


@pytest.mark.parametrize("kind", ("gin", "gine"))
def test_under_accel_a_deferred_activation_feeds_the_convs(kind, monkeypatch):
    N, C = N_DST, 40
    ei = conv_edges().to(dev())
    gen = torch.Generator().manual_seed(81)
    x = torch.randn(N, C, generator=gen).to(dev()).requires_grad_(True)
    e = torch.randn(700, C, generator=gen).to(dev()).requires_grad_(True)
    g = torch.randn(N, C, generator=gen).to(dev())
    bn = torch.nn.BatchNorm1d(C).to(dev()).train()
    conv = (PN.GINEConv if kind == "gine" else PN.GINConv)(mlp(C, 6), eps=0.25).to(dev())
    wrt = (x, e) if kind == "gine" else (x,)

    def layer(form):
        h = F.dropout(F.relu(bn(x)), p=0.5, training=False)
        h = form(h)
        out = conv(h, ei, e) if kind == "gine" else conv(h, ei)
        return out, torch.autograd.grad(out, wrt, g)
    plain = layer(lambda h: h)                                                      # outside accel: torch's BatchNorm, real tensors
    accel = load_accel()
    seen = spy_node_inputs(monkeypatch)
    with accel.scope():
        deferred = layer(lambda h: h)
        formed = layer(lazy.materialise)                                            # the same activation, formed before the conv sees it
    assert seen == [lazy.LazyBnAct, torch.Tensor], seen                             # (the spy starts after the plain run)
    assert torch.equal(deferred[0], formed[0]) and all(torch.equal(a, b) for a, b in zip(deferred[1], formed[1]))
    # against the run outside accel: another fp32 BatchNorm (fused statistics + apply) under the same two Linear layers -- the
    # gradient bar's order for values and gradients alike
    close(deferred[0], plain[0], 1e-4)
    for a, b in zip(deferred[1], plain[1]):
        close(a, b, 1e-4)
    assert float((deferred[0] - deferred[0][1]).detach().abs().max()) > 0                    # (not one row repeated for every node)


@pytest.mark.parametrize("conv", ("gin", "gine"))
def test_under_accel_a_two_layer_molgnn_meets_the_float64_bars(conv, monkeypatch):
    cpu = mol_batch()
    batch = saint.Batch.from_data_list(data.molhiv_like(24, seed=1)).to(dev())
    hp = {"alpha": 0.5, "kd_T": 2.0}
    torch.manual_seed(72)
    model = models.MolGNN(conv, num_layers=2, emb_dim=32, dropout=0.0).to(dev()).train()
    ref_loss, ref_grads = molgnn_float64(model, cpu, "supervised", hp, None)
    accel = load_accel()
    seen = spy_node_inputs(monkeypatch)
    with accel.scope():
        model.zero_grad()
        loss = models.mol_batch_loss(model, batch, "supervised", hp)[0]
        loss.backward()
    assert seen == [torch.Tensor, lazy.LazyBnAct], seen                             # layer 2 is fed the deferred BatchNorm -> relu -> dropout
    assert not lazy.ACCEL_ACTIVE and not PN._MP_RUNNING
    close(loss, ref_loss, 1e-4)
    for k, p in model.named_parameters():
        assert torch.isfinite(p.grad).all(), k
        before_bn = k.endswith((".nn.0.bias", ".nn.3.bias"))                        # (exact gradient 0: see the test above)
        close(p.grad, ref_grads[k], 1e-4, scale=ref_grads[k[:-4] + "weight"] if before_bn else None)
