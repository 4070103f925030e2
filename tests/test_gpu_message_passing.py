"""User-defined message-passing convs on the device: the aggregation kernels of csrc/scatter.hip (``ops.scatter``) and their backward,
plans built without a host read (``ops.rows_plan(check="deferred")``), and ``nn.MessagePassing`` -- against float64 torch on the CPU
(``index_add_``, ``scatter_reduce(..., include_self=False)``) and against the package's own restatements (``ops.spmm``, ``nn.RGCNConv``).

Bars.  Row sums / means: rtol 1e-5, atol 1e-5 * max|ref| (the project's bar for row sums).  Gradients of the composed
layers: rtol 1e-4, atol 1e-4 * max|ref| (a gradient element is a sum over up to E products formed in fp32 by two different orders of
the same terms).  max / min, their arg and their gradients: exact."""
import functools
import importlib.util
import os

import pytest
import torch

from efficient_gnns_amd import _lib, ops
from efficient_gnns_amd import nn as PN
from efficient_gnns_amd.sparse import SparseTensor
from conftest import ROOT

pytestmark = pytest.mark.gpu

N_ROWS, HUB, EMPTY = 37, 7, (0, 1, 2, 3, 4, 36)
CS, ES = (1, 3, 4, 40, 260), (0, 1, 700)
REDUCES = ("sum", "mean", "max", "min")
TORCH_REDUCE = {"sum": "sum", "mean": "mean", "max": "amax", "min": "amin"}


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def close(got, ref, rtol):
    ref = ref.detach().double().cpu()
    atol = rtol * float(ref.abs().max()) if ref.numel() else 0.0
    torch.testing.assert_close(got.detach().double().cpu(), ref, rtol=rtol, atol=atol)


@functools.lru_cache(maxsize=None)
def make_index(E):
    """[E] int64 on the CPU, already wrapped (`rows`), and the form handed to the kernels (`raw`: every third id negative).  E = 700:
    the hub row 300 times (over two EGNN_ROWS_SUM_CHUNKs), six rows never named, the rest spread in no order."""
    g = torch.Generator().manual_seed(1000 + E)
    allowed = torch.tensor([r for r in range(N_ROWS) if r not in EMPTY and r != HUB])
    if E == 0:
        rows = torch.zeros(0, dtype=torch.int64)
    elif E == 1:
        rows = torch.tensor([N_ROWS - 3])
    else:
        rows = torch.cat([torch.full((300,), HUB, dtype=torch.int64), allowed[torch.randint(0, allowed.numel(), (E - 300,), generator=g)]])
        rows = rows[torch.randperm(E, generator=g)]
    raw = rows.clone()
    raw[::3] -= N_ROWS
    return rows, raw


@functools.lru_cache(maxsize=None)
def make_case(E, C, integer):
    """src, g (float64 CPU) and per reduce the float64 reference (out, arg or None, dsrc)."""
    gen = torch.Generator().manual_seed(7 * E + C + (1 if integer else 0))
    rows, raw = make_index(E)
    if integer:   # small integers: exact in fp32, with exact ties
        src = torch.randint(-3, 4, (E, C), generator=gen).double()
        g = torch.randint(-4, 5, (N_ROWS, C), generator=gen).double()
    else:
        src = torch.randn(E, C, generator=gen, dtype=torch.float64)
        g = torch.randn(N_ROWS, C, generator=gen, dtype=torch.float64)
    refs = {}
    for red in REDUCES:
        s = src.clone().requires_grad_(True)
        if red == "sum":
            out = torch.zeros(N_ROWS, C, dtype=torch.float64).index_add_(0, rows, s)
        else:
            out = torch.zeros(N_ROWS, C, dtype=torch.float64).scatter_reduce(0, rows.view(-1, 1).expand(E, C), s, TORCH_REDUCE[red], include_self=False)
        arg = None
        if red in ("max", "min"):
            # the smallest position attaining the extreme (E for a row no id names); the gradient lands there only
            arg = torch.full((N_ROWS, C), E, dtype=torch.int64)
            for p in range(E - 1, -1, -1):
                r = int(rows[p])
                arg[r][src[p] == out[r].detach()] = p
            dsrc = torch.zeros(E, C, dtype=torch.float64)
            live = arg < E
            cols = torch.arange(C).expand(N_ROWS, C)
            dsrc[arg[live], cols[live]] = g[live]
        else:
            (dsrc,) = torch.autograd.grad(out, s, g) if E else (torch.zeros(0, C, dtype=torch.float64),)
        refs[red] = (out.detach(), arg, dsrc)
    return src, g, refs


def on_gpu(t, slice_pitch=False):
    t = t.float()
    if slice_pitch:   # a column slice: the pitch (C + 3) differs from C and is no multiple of 4 -> the scalar path
        big = torch.zeros(t.shape[0], t.shape[1] + 3)
        big[:, 1:1 + t.shape[1]] = t
        return big.to(dev())[:, 1:1 + t.shape[1]]
    return t.to(dev())


# ------------------------------------------------------------------------------------------------
# scatter forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("C", CS)
def test_scatter_sum_and_mean_forward(E, C):
    src64, _, refs = make_case(E, C, False)
    _, raw = make_index(E)
    idx, src = raw.to(dev()), on_gpu(src64)
    for red in ("sum", "mean"):
        out = ops.scatter(src, idx, N_ROWS, red)
        assert out.shape == (N_ROWS, C)
        close(out, refs[red][0], 1e-5)
        assert torch.equal(out, ops.scatter(src, idx, N_ROWS, red))                # two calls are bit-equal
        assert torch.equal(out[list(EMPTY)], torch.zeros(len(EMPTY), C, device=dev()))
    # sum IS the existing run-sum: bit-equal to the backward of the row gather by the same ids
    x = torch.zeros(N_ROWS, C, device=dev(), requires_grad=True)
    (want,) = torch.autograd.grad(ops.take_rows(x, idx, "sum"), x, src)
    assert torch.equal(ops.scatter(src, idx, N_ROWS, "sum"), want)
    assert torch.equal(ops.scatter(src, idx, N_ROWS, "add"), want)


@pytest.mark.parametrize("red", ("sum", "mean", "max", "min"))
def test_scatter_forward_from_a_column_slice(red):
    E, C = 700, 4
    src64, _, refs = make_case(E, C, True)
    _, raw = make_index(E)
    src = on_gpu(src64, slice_pitch=True)
    assert src.stride(0) == C + 3 and not src.is_contiguous()
    out, arg = ops.scatter(src, raw.to(dev()), N_ROWS, red, return_arg=True)
    if red in ("max", "min"):
        assert torch.equal(out.cpu().double(), refs[red][0]) and torch.equal(arg.cpu(), refs[red][1])
    else:
        assert arg is None
        close(out, refs[red][0], 1e-5)
        assert torch.equal(out, ops.scatter(src.contiguous(), raw.to(dev()), N_ROWS, red))   # the scalar path adds in the same order


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("C", CS)
def test_scatter_max_and_min_forward_are_exact(E, C):
    src64, _, refs = make_case(E, C, True)
    _, raw = make_index(E)
    idx, src = raw.to(dev()), on_gpu(src64)
    for red in ("max", "min"):
        out, arg = ops.scatter(src, idx, N_ROWS, red, return_arg=True)
        ref_out, ref_arg, _ = refs[red]
        assert torch.equal(out.cpu().double(), ref_out)
        assert arg.dtype == torch.int64 and torch.equal(arg.cpu(), ref_arg)        # the smallest position; E for an empty row
        assert bool((arg[list(EMPTY)] == E).all()) and bool((out[list(EMPTY)] == 0).all())
        again = ops.scatter(src, idx, N_ROWS, red, return_arg=True)
        assert torch.equal(out, again[0]) and torch.equal(arg, again[1])


def test_scatter_flattens_trailing_dimensions():
    src64, _, refs = make_case(700, 40, False)
    _, raw = make_index(700)
    out = ops.scatter(on_gpu(src64).view(700, 4, 10), raw.to(dev()), N_ROWS, "mean")
    assert out.shape == (N_ROWS, 4, 10)
    close(out.view(N_ROWS, 40), refs["mean"][0], 1e-5)


# ------------------------------------------------------------------------------------------------
# scatter backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("C", CS)
def test_scatter_backward(E, C):
    _, raw = make_index(E)
    idx = raw.to(dev())
    for red in REDUCES:
        exact = red in ("max", "min")
        src64, g64, refs = make_case(E, C, exact)
        src, g = on_gpu(src64).requires_grad_(True), on_gpu(g64)
        out, _ = ops._Scatter.apply(src, ops.rows_plan(idx, N_ROWS), ops._SCATTER_REDUCE[red])     # (ops.scatter without its final view)
        (dsrc,) = torch.autograd.grad(out, src, g)
        assert dsrc.shape == (E, C)
        if exact:
            assert torch.equal(dsrc.cpu().double(), refs[red][2])                  # the gradient lands on the arg position only
        else:
            close(dsrc, refs[red][2], 1e-5)
        # the kernel writes every element: the same values into a buffer the test filled with NaN
        fn = out.grad_fn
        into = torch.full((E, C), float("nan"), device=dev())
        rc = _lib.load().egnn_scatter_bwd_f32(_lib.ptr(into), C, E, _lib.ptr(fn.plan.rows), N_ROWS, _lib.ptr(g), g.stride(0), C, fn.red,
                                              _lib.ptr(fn.count), _lib.ptr(fn.arg), _lib.stream())
        assert rc == 0
        assert torch.equal(into, dsrc) and not bool(torch.isnan(into).any())


def test_scatter_backward_into_a_pitched_gradient_from_a_column_slice():
    E, C = 700, 3
    src64, g64, refs = make_case(E, C, False)
    _, raw = make_index(E)
    src = on_gpu(src64, slice_pitch=True).requires_grad_(True)
    (dsrc,) = torch.autograd.grad(ops.scatter(src, raw.to(dev()), N_ROWS, "mean"), src, on_gpu(g64, slice_pitch=True))
    close(dsrc, refs["mean"][2], 1e-5)


# ------------------------------------------------------------------------------------------------
# plans without a host read
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("C", CS)
def test_deferred_plan_gives_the_host_checked_results(E, C):
    _, raw = make_index(E)
    idx = raw.to(dev())
    ops.rows_oob(dev())
    host, plan = ops.rows_plan(idx, N_ROWS), ops.rows_plan(idx, N_ROWS, check="deferred")
    assert plan.deferred and plan.dups is None and not host.deferred and plan.S == E
    assert torch.equal(plan.idx, host.idx) and torch.equal(plan.rows, host.idx)
    if E:                                                                          # the keys are kept whether or not an id repeats
        assert plan.keys is plan.all_keys and torch.equal(plan.all_keys, host.all_keys)
    assert ops.rows_plan(idx, N_ROWS, check="deferred") is not plan                # not kept in the identity cache
    before = len(ops._ROWS_PLANS)
    ops.rows_plan(idx.clone(), N_ROWS, check="deferred")
    assert len(ops._ROWS_PLANS) == before
    for red in REDUCES:
        src64, g64, _ = make_case(E, C, red in ("max", "min"))
        a, b = on_gpu(src64).requires_grad_(True), on_gpu(src64).requires_grad_(True)
        out_h, arg_h = ops.scatter(a, idx, N_ROWS, red, return_arg=True)
        out_d, arg_d = ops.scatter(b, None, N_ROWS, red, plan=plan, return_arg=True)
        assert torch.equal(out_h, out_d) and (arg_h is None or torch.equal(arg_h, arg_d))
        g = on_gpu(g64)
        assert torch.equal(torch.autograd.grad(out_h, a, g)[0], torch.autograd.grad(out_d, b, g)[0])
    # the same plan serves the gather and its backward
    x64 = make_case(E, C, False)[1]
    xa, xb = on_gpu(x64).requires_grad_(True), on_gpu(x64).requires_grad_(True)
    ya, yb = ops.take_rows(xa, idx, "sum"), ops.take_rows(xb, plan)
    assert torch.equal(ya, yb) and torch.equal(ya, xa.detach()[host.idx])
    gy = torch.randn_like(ya)
    assert torch.equal(torch.autograd.grad(ya, xa, gy)[0], torch.autograd.grad(yb, xb, gy)[0])
    w = torch.randn(5, C, device=dev())
    assert torch.equal(ops.linear_rows(xa, idx, w, duplicates="sum"), ops.linear_rows(xb, plan, w))
    assert ops.rows_oob(dev()) == 0


def test_deferred_plan_drops_and_counts_ids_out_of_range():
    E, C = 700, 12
    src64, g64, _ = make_case(E, C, False)
    rows, raw = make_index(E)
    bad = raw.clone()
    where = torch.tensor([5, 333, 699])
    bad[where] = torch.tensor([N_ROWS, N_ROWS + 13, 10 ** 6])
    keep = torch.ones(E, dtype=torch.bool)
    keep[where] = False
    ops.rows_oob(dev())
    with pytest.raises(IndexError):
        ops.rows_plan(bad.to(dev()), N_ROWS)                                       # the host-checked plan raises, as before
    plan = ops.rows_plan(bad.to(dev()), N_ROWS, check="deferred")
    src = on_gpu(src64).requires_grad_(True)
    for red in REDUCES:
        out = ops.scatter(src, None, N_ROWS, red, plan=plan)
        if red == "sum":
            ref = torch.zeros(N_ROWS, C, dtype=torch.float64).index_add_(0, rows[keep], src64[keep])
        else:
            ref = torch.zeros(N_ROWS, C, dtype=torch.float64).scatter_reduce(0, rows[keep].view(-1, 1).expand(-1, C), src64[keep],
                                                                             TORCH_REDUCE[red], include_self=False)
        close(out, ref, 1e-5)
        (dsrc,) = torch.autograd.grad(out, src, on_gpu(g64))
        assert bool((dsrc[where.to(dev())] == 0).all())                            # a dropped entry gets a zero gradient row
    x = on_gpu(g64).requires_grad_(True)
    y = ops.take_rows(x, plan)                                                     # a dropped id reads row 0 and gets no gradient
    assert torch.equal(y[keep.to(dev())], x.detach()[rows[keep].to(dev())])
    (gx,) = torch.autograd.grad(y, x, torch.ones_like(y))
    counts = torch.bincount(rows[keep], minlength=N_ROWS).double().view(-1, 1).expand(-1, C)
    assert torch.equal(gx.cpu().double(), counts)
    assert ops.rows_oob(dev()) == 3 and ops.rows_oob(dev()) == 0
    with pytest.raises(IndexError):
        ops.rows_plan(bad.to(dev()), 0, check="deferred")                          # no row at all: known without a read


def graph_data(n=50, E=400, seed=3):
    """E edges over nodes 0 .. n - 11 (the last ten are isolated), with repeated edges and repeated endpoints."""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n - 10, (2, E), generator=g)
    ei[:, 50:60] = ei[:, 40:50]
    ei[1, 100:160] = 5
    return ei


def reference_aggregate(x_src, ei, aggr, flow, n_out):
    """float64: out[t] = aggr of x_src[s] over the edges (s -> t)."""
    j, i = (0, 1) if flow == "source_to_target" else (1, 0)
    C = x_src.shape[1]
    msgs = x_src[ei[j]]
    if aggr in ("add", "sum"):
        return torch.zeros(n_out, C, dtype=torch.float64).index_add_(0, ei[i], msgs)
    return torch.zeros(n_out, C, dtype=torch.float64).scatter_reduce(0, ei[i].view(-1, 1).expand(-1, C), msgs, TORCH_REDUCE[aggr],
                                                                     include_self=False)


def test_a_captured_propagate_step_replays_to_the_eager_result():
    N, C = 50, 12
    ei = graph_data(N).to(dev())
    conv = PN.MessagePassing(aggr="mean")
    x = torch.randn(N, C, device=dev())
    ops.rows_oob(dev())
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            conv.propagate(ei, x=x)                                                # warm-up
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = conv.propagate(ei, x=x)                                            # builds its deferred plans inside the capture
        x.copy_(torch.randn(N, C, device=dev()))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, conv.propagate(ei, x=x))
    close(y, reference_aggregate(x.double().cpu(), ei.cpu(), "mean", "source_to_target", N), 1e-5)
    assert ops.rows_oob(dev()) == 0


# ------------------------------------------------------------------------------------------------
# nn.MessagePassing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", ("source_to_target", "target_to_source"))
@pytest.mark.parametrize("aggr", ("add", "sum", "mean", "max", "min"))
def test_default_message_each_aggregation_both_flows(aggr, flow):
    N, C = 50, 12
    ei = graph_data(N)
    x64 = torch.randn(N, C, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    out = PN.MessagePassing(aggr=aggr, flow=flow).propagate(ei.to(dev()), x=x64.float().to(dev()))
    ref = reference_aggregate(x64.float().double(), ei, aggr, flow, N)
    if aggr in ("max", "min"):
        assert torch.equal(out.cpu().double(), ref)
    else:
        close(out, ref, 1e-5)
    assert bool((out[N - 10:] == 0).all())                                         # isolated nodes
    if aggr == "mean" and flow == "source_to_target":
        adj = SparseTensor(row=ei[1].to(dev()), col=ei[0].to(dev()), sparse_sizes=(N, N))
        close(ops.spmm(adj, x64.float().to(dev()), "mean"), ref, 1e-5)
        close(out, ops.spmm(adj, x64.float().to(dev()), "mean"), 1e-5)


class MixConv(PN.MessagePassing):
    """Both ends and a per-edge tensor in the message, the input again in the update."""

    def __init__(self, aggr):
        super().__init__(aggr=aggr)

    def forward(self, x, edge_index, edge_weight):
        return self.propagate(edge_index, x=x, edge_weight=edge_weight)

    def message(self, x_i, x_j, edge_weight):
        return edge_weight.view(-1, 1) * (x_j - 0.5 * x_i)

    def update(self, aggr_out, x):
        return aggr_out + x


@pytest.mark.parametrize("aggr", ("add", "mean", "max"))
def test_message_of_both_ends_and_an_edge_tensor_with_gradients(aggr):
    N, C, E = 50, 12, 400
    gen = torch.Generator().manual_seed(5)
    ei = graph_data(N)
    x64 = torch.randn(N, C, generator=gen).double().requires_grad_(True)
    w64 = (torch.rand(E, generator=gen) + 0.5).double().requires_grad_(True)
    g64 = torch.randn(N, C, generator=gen).double()
    msgs = w64.view(-1, 1) * (x64[ei[0]] - 0.5 * x64[ei[1]])
    if aggr == "add":
        ref = torch.zeros(N, C, dtype=torch.float64).index_add_(0, ei[1], msgs) + x64
    else:
        ref = torch.zeros(N, C, dtype=torch.float64).scatter_reduce(0, ei[1].view(-1, 1).expand(-1, C), msgs, TORCH_REDUCE[aggr],
                                                                    include_self=False) + x64
    ref_gx, ref_gw = torch.autograd.grad(ref, (x64, w64), g64)
    x, w = x64.detach().float().to(dev()).requires_grad_(True), w64.detach().float().to(dev()).requires_grad_(True)
    out = MixConv(aggr)(x, ei.to(dev()), w)
    close(out, ref.detach(), 1e-5)
    gx, gw = torch.autograd.grad(out, (x, w), g64.float().to(dev()))
    close(gx, ref_gx, 1e-4)
    close(gw, ref_gw, 1e-4)


class PairConv(PN.MessagePassing):
    def __init__(self):
        super().__init__(aggr="max", node_dim=0)

    def message(self, x_i, x_j, size_i, size_j, dim_size, index, ptr=None):
        assert (size_j, size_i, dim_size) == (30, 20, 20) and ptr is None and index.numel() == x_j.shape[0]
        return x_j - x_i


def test_bipartite_pair_of_node_tensors():
    C, E = 12, 200
    gen = torch.Generator().manual_seed(9)
    ei = torch.stack([torch.randint(0, 30, (E,), generator=gen), torch.randint(0, 17, (E,), generator=gen)])
    xs, xd = torch.randn(30, C, generator=gen), torch.randn(20, C, generator=gen)
    out = PairConv().propagate(ei.to(dev()), size=(30, 20), x=(xs.to(dev()), xd.to(dev())))
    msgs = (xs[ei[0]] - xd[ei[1]]).double()            # (fp32 subtraction first: the reference takes the same messages)
    ref = torch.zeros(20, C, dtype=torch.float64).scatter_reduce(0, ei[1].view(-1, 1).expand(-1, C), msgs, "amax", include_self=False)
    assert out.shape == (20, C) and torch.equal(out.cpu().double(), ref)
    with pytest.raises(NotImplementedError):
        PN.MessagePassing(flow="target_to_source").propagate(ei.to(dev()), x=(xs.to(dev()), xd.to(dev())))
    with pytest.raises(ValueError):
        PairConv().propagate(ei.to(dev()), size=(31, 20), x=(xs.to(dev()), xd.to(dev())))


class RelConv(PN.MessagePassing):
    """A relational layer in PyG's idiom: per edge type a bias-free Linear of the neighbour inside ``message``, mean aggregation, and a
    per-node-type Linear of the node itself."""

    def __init__(self, c_in, c_out, node_types, edge_types):
        super().__init__(aggr="mean")
        self.c_out = c_out
        self.rel_lins = torch.nn.ModuleList(torch.nn.Linear(c_in, c_out, bias=False) for _ in range(edge_types))
        self.root_lins = torch.nn.ModuleList(torch.nn.Linear(c_in, c_out, bias=True) for _ in range(node_types))

    def forward(self, x, edge_index, edge_type, node_type):
        out = x.new_zeros(x.shape[0], self.c_out)
        for i in range(len(self.rel_lins)):
            out = out + self.propagate(edge_index[:, edge_type == i], x=x, edge_type=i)
        for i, lin in enumerate(self.root_lins):
            rows = torch.nonzero(node_type == i).view(-1)
            out = out.index_add(0, rows, lin(x[rows]))
        return out

    def message(self, x_j, edge_type: int):
        return self.rel_lins[edge_type](x_j)


def relational_setup():
    N, C_IN, C_OUT, E = 50, 12, 8, 400
    gen = torch.Generator().manual_seed(21)
    ei = graph_data(N)
    edge_type = torch.randint(0, 2, (E,), generator=gen) * 2                       # types 0 and 2; type 1 has no edge
    node_type = torch.randint(0, 2, (N,), generator=gen)
    x = torch.randn(N, C_IN, generator=gen)
    g = torch.randn(N, C_OUT, generator=gen)
    torch.manual_seed(33)
    generic, restated = RelConv(C_IN, C_OUT, 2, 3).to(dev()), PN.RGCNConv(C_IN, C_OUT, 2, 3).to(dev())
    restated.load_state_dict(generic.state_dict())
    return generic, restated, x.to(dev()), ei.to(dev()), edge_type.to(dev()), node_type.to(dev()), g.to(dev())


def step(layer, x, ei, edge_type, node_type, g):
    x = x.clone().requires_grad_(True)
    out = layer(x, ei, edge_type, node_type)
    params = [p for p in layer.parameters()]
    grads = torch.autograd.grad(out, [x] + params, g, allow_unused=True)           # (the empty edge type's weight gets no gradient)
    return out.detach(), [torch.zeros_like(t) if gr is None else gr for t, gr in zip([x] + params, grads)]


def test_relational_layer_matches_the_restated_rgcn_conv():
    generic, restated, *data = relational_setup()
    out_r, grads_r = step(restated, *data)
    out_g, grads_g = step(generic, *data)
    close(out_g, out_r, 1e-5)
    for a, b in zip(grads_g, grads_r):
        close(a, b, 1e-4)
    assert bool((grads_g[2] == 0).all())                                           # rel_lins.1: no edge of its type


def load_accel():
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_mp", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    return accel


def test_relational_layer_under_accel_runs_the_gather_fused_gemm(monkeypatch):
    generic, restated, *data = relational_setup()
    out_r, grads_r = step(restated, *data)
    fused = []
    real = ops.linear_rows

    def counting(x, idx, *a, **kw):
        if isinstance(idx, ops.RowsPlan) and idx.deferred:
            fused.append(idx.S)
        return real(x, idx, *a, **kw)
    monkeypatch.setattr(ops, "linear_rows", counting)
    accel = load_accel()
    with accel.scope():
        assert accel.enabled()
        out_g, grads_g = step(generic, *data)
    assert not accel.enabled()
    edge_type = data[2]
    assert sorted(fused) == sorted(int((edge_type == i).sum()) for i in (0, 2))    # one fused GEMM per non-empty edge type
    close(out_g, out_r, 1e-5)
    for a, b in zip(grads_g, grads_r):
        close(a, b, 1e-4)


class LinConv(PN.MessagePassing):
    def __init__(self, c_in, c_out):
        super().__init__(aggr="mean")
        self.lin = torch.nn.Linear(c_in, c_out, bias=False)

    def forward(self, x, adj):
        return self.propagate(adj, x=x)

    def message(self, x_j, ptr):
        self.saw_ptr = ptr is not None
        return self.lin(x_j)


class FusedConv(LinConv):
    def message_and_aggregate(self, adj_t, x):
        return ops.linear(ops.spmm(adj_t, x, "mean"), self.lin.weight)


def test_sparse_tensor_input_gives_the_edge_list_result():
    N, C = 50, 12
    ei = graph_data(N).to(dev())
    x = torch.randn(N, C, generator=torch.Generator().manual_seed(2)).to(dev())
    adj_t = SparseTensor(row=ei[1], col=ei[0], sparse_sizes=(N, N))
    torch.manual_seed(4)
    conv = LinConv(C, 8).to(dev())
    fused = FusedConv(C, 8).to(dev())
    fused.load_state_dict(conv.state_dict())
    accel = load_accel()
    for scoped in (False, True):
        if scoped:
            accel.enable()
        try:
            by_edges = conv(x, ei)
            assert not conv.saw_ptr
            by_adj = conv(x, adj_t)
            assert conv.saw_ptr
            by_spmm = fused(x, adj_t)                                              # message_and_aggregate is called with the adjacency
        finally:
            accel.disable()
        close(by_adj, by_edges, 1e-5)
        close(by_spmm, by_edges, 1e-5)
    with pytest.raises(NotImplementedError):
        PN.MessagePassing(flow="target_to_source").propagate(adj_t, x=x)
