"""GPU checks of the summing row step (egnn_adam_rows_step_sum_f32, csrc/adam_rows.hip) and ``LazyRowAdam(duplicates="sum")``: one Adam
step over a list of gradient rows that may name a table row several times.

Kernel level: a table of ``n_rows`` rows stands at step S - 1 = 69 with every kind of row the lazy scheme knows (current, never had a
gradient, 5 and 63 steps behind); one entry list per shape, built on the CPU with a fixed seed, names rows 1, 2, 3, 8 and 70 times,
scattered through the list between entries of another node type and two ids outside the table.  The reference is the EXISTING step
kernel on an identically prepared table, fed the unique rows with their gradients summed by torch in fp32 in ascending entry order.
Optimiser level: the 70-step scheme of test_gpu_lazy_adam.py with every step's rows split over three overlapping deposits, against
dense ``torch.optim.Adam`` in float64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from efficient_gnns_amd import _lib, ops
from efficient_gnns_amd.optim import MAX_LAG, LazyRowAdam, RowState

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(37, 128), (11, 20), (9, 4), (7, 260)]
# rows named 70 times: row 0 everywhere; at D = 4 a workgroup serves 256 sorted entries, so three more such rows are needed before a
# run can cross a workgroup boundary
HUBS = {(37, 128): (0,), (11, 20): (0,), (9, 4): (0, 5, 6, 7), (7, 260): (0,)}
S = 70                       # the step the kernels apply; the table stands at S - 1 and was flushed at S - 64
LR = 3e-3
NEVER_ROW, LAG5_ROW, LAG63_ROW = 1, 2, 3
TYPE = 2                     # the table's node type; entries of type 0 are interleaved
F32_THIRD = float(np.float32(1.0 / 3.0))


def rows_per_workgroup(dim):
    groups, lg = dim // 4, 0
    while lg < 6 and (1 << lg) < groups:
        lg += 1
    return 256 >> lg


@functools.lru_cache(maxsize=None)
def entry_list(n_rows, dim):
    """(node_type, local_idx, g, multiplicity per row) on the CPU.  The last table row is never named."""
    gen = torch.Generator().manual_seed(77 * n_rows + dim)
    mult = {0: 70, NEVER_ROW: 8, LAG5_ROW: 3, LAG63_ROW: 2, 4: 1}
    for r in range(5, n_rows - 1):
        mult[r] = (1, 2, 3, 8)[r % 4]
    for r in HUBS[(n_rows, dim)]:
        mult[r] = 70
    idx = [r for r, k in mult.items() for _ in range(k)]
    types = [TYPE] * len(idx)
    idx += [-1, n_rows + 3]                                  # two ids outside the table, of the table's type
    types += [TYPE, TYPE]
    other = torch.randint(0, n_rows, (len(idx) // 3,), generator=gen).tolist()   # another type's entries, same id range
    idx += other
    types += [0] * len(other)
    perm = torch.randperm(len(idx), generator=gen)
    local_idx = torch.tensor(idx, dtype=torch.int64)[perm]
    node_type = torch.tensor(types, dtype=torch.int64)[perm]
    g = 0.1 * torch.randn(len(idx), dim, generator=gen)
    # the properties the scenario is about
    named = sorted(mult)
    counts = [mult[r] for r in named]
    assert {1, 2, 3, 8, 70} <= set(counts) and n_rows - 1 not in mult
    ends = np.cumsum(counts)
    rpw = rows_per_workgroup(dim)
    assert any(e - c < b < e for c, e in zip(counts, ends) for b in range(rpw, int(ends[-1]), rpw)), "no run crosses a workgroup"
    first = {r: int(((local_idx == r) & (node_type == TYPE)).nonzero()[0]) for r in named}
    last = {r: int(((local_idx == r) & (node_type == TYPE)).nonzero()[-1]) for r in named}
    assert any(last[r] - first[r] > mult[r] for r in named if mult[r] > 1), "the entries of a row are not scattered"
    return node_type, local_idx, g, mult


def summed(n_rows, dim, scale):
    """(rows, G): the named rows ascending and scale * (((g[i1] + g[i2]) + ...) + g[ik]) in torch fp32, ascending entry order."""
    node_type, local_idx, g, mult = entry_list(n_rows, dim)
    rows, G = sorted(mult), []
    for r in rows:
        ids = ((local_idx == r) & (node_type == TYPE)).nonzero().view(-1).tolist()
        assert ids == sorted(ids) and len(ids) == mult[r]
        acc = g[ids[0]].clone()
        for i in ids[1:]:
            acc = acc + g[i]
        G.append(acc * torch.tensor(scale, dtype=torch.float32))
    return torch.tensor(rows, dtype=torch.int64), torch.stack(G)


def prepared_table(n_rows, dim):
    """A RowState at step S - 1, flushed at S - 64, rings filled for S - 63 .. S; identical on every call."""
    gen = torch.Generator().manual_seed(5 * n_rows + dim)
    p = torch.nn.Parameter(torch.randn(n_rows, dim, generator=gen).to(DEV))
    st = RowState(p, dict(lr=LR, betas=(0.9, 0.999), eps=1e-8), f"{n_rows}x{dim}")
    st.m.copy_(0.05 * torch.randn(n_rows, dim, generator=gen))
    st.v.copy_(0.01 * torch.rand(n_rows, dim, generator=gen))
    last = torch.full((n_rows,), S - 1, dtype=torch.int32)
    last[NEVER_ROW], last[LAG5_ROW], last[LAG63_ROW] = -1, S - 1 - 5, S - 1 - 63
    st.m[NEVER_ROW], st.v[NEVER_ROW] = 0, 0
    st.last.copy_(last)
    st.t, st.flushed = S - 1, S - MAX_LAG
    for t in range(S - MAX_LAG + 1, S + 1):
        st.ring.fill(t, LR)
    return st


def state_of(st):
    torch.cuda.synchronize()
    return st.param.detach().cpu(), st.m.cpu(), st.v.cpu(), st.last.cpu()


def catch_up(st, node_type, local_idx):
    st.catch_up(TYPE, None if node_type is None else node_type.to(DEV), local_idx.to(DEV))


def plain_step(st, node_type, local_idx, g):
    node_type, local_idx, g = (None if x is None else x.to(DEV) for x in (node_type, local_idx, g))
    _lib.check(_lib.load().egnn_adam_rows_step_f32(ctypes.byref(st._desc(S)), TYPE, _lib.ptr(node_type), _lib.ptr(local_idx),
                                                   local_idx.numel(), _lib.ptr(g), g.stride(0), _lib.stream()), "plain step")
    return state_of(st) + (int(st.dup.item()),)


def sum_step(st, node_type, local_idx, g, scale):
    node_type, local_idx, g = (None if x is None else x.to(DEV) for x in (node_type, local_idx, g))
    lib, n = _lib.load(), local_idx.numel()
    ws_bytes = lib.egnn_adam_rows_step_sum_ws_bytes(n, st.param.shape[0])
    assert ws_bytes <= 32 * n + (1 << 20), "O(n) bytes, independent of the table"
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.egnn_adam_rows_step_sum_f32(ctypes.byref(st._desc(S)), TYPE, _lib.ptr(node_type), _lib.ptr(local_idx), n, _lib.ptr(g),
                                               g.stride(0), scale, _lib.ptr(ws), ws_bytes, _lib.stream()), "sum step")
    return state_of(st) + (int(st.dup.item()),)


@functools.lru_cache(maxsize=None)
def sum_result(n_rows, dim, scale):
    node_type, local_idx, g, _ = entry_list(n_rows, dim)
    st = prepared_table(n_rows, dim)
    catch_up(st, node_type, local_idx)
    return sum_step(st, node_type, local_idx, g, scale)


# ---- 1. bit-equality with the plain step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("n_rows,dim", SHAPES)
def test_sum_step_equals_plain_step_on_presummed_rows(n_rows, dim, scale):
    rows, G = summed(n_rows, dim, scale)
    ref = prepared_table(n_rows, dim)
    before = state_of(ref)
    ref_rows = torch.cat([rows, torch.tensor([-1, n_rows + 3])])          # the plain step counts the two ids outside the table too
    ref_g = torch.cat([G, torch.ones(2, dim)])
    catch_up(ref, None, ref_rows)
    want = plain_step(ref, None, ref_rows, ref_g)
    got = sum_result(n_rows, dim, scale)
    for name, a, b in zip(("p", "m", "v", "last"), got, want):
        assert torch.equal(a, b), (name, float((a.double() - b.double()).abs().max()))
    assert got[4] == 2 and want[4] == 2                                    # dup_count: the entries outside the table, nothing else
    assert (got[3][rows] == S).all() and got[3][n_rows - 1] == S - 1
    for a, b in zip(got[:3], before[:3]):
        assert torch.equal(a[n_rows - 1], b[n_rows - 1]), "a row nobody named moved"
    assert not torch.equal(got[0][NEVER_ROW], before[0][NEVER_ROW])


@pytest.mark.parametrize("n_rows,dim", SHAPES)
def test_sum_step_without_duplicates_equals_plain_step_on_the_same_list(n_rows, dim):
    gen = torch.Generator().manual_seed(n_rows + dim)
    perm = torch.randperm(2 * (n_rows - 1), generator=gen)
    local_idx = torch.cat([torch.arange(n_rows - 1), torch.arange(n_rows - 1)])[perm]       # every row but the last, once per type
    node_type = torch.cat([torch.full((n_rows - 1,), TYPE), torch.zeros(n_rows - 1, dtype=torch.int64)])[perm]
    g = 0.1 * torch.randn(local_idx.numel(), dim, generator=gen)
    out = []
    for step in (plain_step, lambda *a: sum_step(*a, 1.0)):
        st = prepared_table(n_rows, dim)
        catch_up(st, node_type, local_idx)
        out.append(step(st, node_type, local_idx, g))
    for name, a, b in zip(("p", "m", "v", "last"), *out):
        assert torch.equal(a, b), name
    assert out[0][4] == 0 and out[1][4] == 0


def test_row_that_is_not_current_is_counted_and_not_stepped():
    n_rows, dim = SHAPES[1]
    node_type, local_idx, g, _ = entry_list(n_rows, dim)
    st = prepared_table(n_rows, dim)                                       # no catch-up: rows 2 and 3 are behind
    before = state_of(st)
    got = sum_step(st, node_type, local_idx, g, 1.0)
    assert got[4] == 2 + 2                                                 # two ids outside the table, two rows that lost the claim
    for k in range(4):
        assert torch.equal(got[k][[LAG5_ROW, LAG63_ROW]], before[k][[LAG5_ROW, LAG63_ROW]])
    want = sum_result(n_rows, dim, 1.0)
    others = [r for r in range(n_rows) if r not in (LAG5_ROW, LAG63_ROW)]
    for k in range(4):
        assert torch.equal(got[k][others], want[k][others])


def test_empty_list_enqueues_nothing():
    n_rows, dim = SHAPES[2]
    st = prepared_table(n_rows, dim)
    before = state_of(st)
    idx = torch.zeros(1, dtype=torch.int64, device=DEV)                   # valid pointers, n == 0, no workspace
    g = torch.zeros(1, dim, device=DEV)
    rc = _lib.load().egnn_adam_rows_step_sum_f32(ctypes.byref(st._desc(S)), TYPE, _lib.ptr(idx), _lib.ptr(idx), 0, _lib.ptr(g), dim, 1.0,
                                                 None, 0, _lib.stream())
    assert rc == 0
    for a, b in zip(state_of(st), before):
        assert torch.equal(a, b)
    assert int(st.dup.item()) == 0


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,dim", SHAPES)
def test_two_runs_and_a_padded_list_give_equal_bits(n_rows, dim):
    """The second run repeats the first; the third appends 300 entries of the other node type, which changes n, the key width and
    the number of workgroups but not one selected entry's position among the selected ones."""
    node_type, local_idx, g, _ = entry_list(n_rows, dim)
    first = sum_result(n_rows, dim, 0.25)
    st = prepared_table(n_rows, dim)
    catch_up(st, node_type, local_idx)
    again = sum_step(st, node_type, local_idx, g, 0.25)
    pad = 300
    gen = torch.Generator().manual_seed(3)
    st = prepared_table(n_rows, dim)
    nt = torch.cat([node_type, torch.zeros(pad, dtype=torch.int64)])
    li = torch.cat([local_idx, torch.randint(0, n_rows, (pad,), generator=gen)])
    gp = torch.cat([g, torch.randn(pad, dim, generator=gen)])
    catch_up(st, nt, li)
    padded = sum_step(st, nt, li, gp, 0.25)
    for other in (again, padded):
        for name, a, b in zip(("p", "m", "v", "last"), first, other):
            assert torch.equal(a, b), name
        assert other[4] == first[4] == 2


# ---- 2. against dense Adam in float64 ------------------------------------------------------------------------------------------
STEPS = 70
LR0, LR1, LR_SWITCH = 5e-3, 1e-3, 30
NEVER = (3, 4, 5)


def lr_at(t):
    return LR0 if t < LR_SWITCH else LR1


def ulp_at(x):
    return float(np.spacing(np.float32(x)))


@functools.lru_cache(maxsize=None)
def scenario(n_rows, dim):
    """The scheme of test_gpu_lazy_adam.py (row 0 always, row 1 only at step 1, row 2 first at step 40, rows 3-5 never, the others with
    probability 0.3), each step's rows split over three deposits that overlap: all rows, every second row, and rows 0, 1, 4, 7, ...;
    every deposit carries gradient rows of its own.  [(rows, [(rows_k, g_k)] * 3) per step] on the CPU."""
    gen = torch.Generator().manual_seed(1000 * n_rows + dim)
    p0 = torch.randn(n_rows, dim, generator=gen)
    steps = []
    for t in range(1, STEPS + 1):
        pick = torch.rand(n_rows, generator=gen) < 0.3
        pick[0] = True
        pick[1] = t == 1
        pick[2] = pick[2] if t > 40 else t == 40
        for r in NEVER:
            pick[r] = False
        rows = pick.nonzero().view(-1)
        parts = [rows, rows[::2], torch.cat([rows[:1], rows[1::3]])]
        steps.append((rows, [(r, 0.1 * torch.randn(r.numel(), dim, generator=gen)) for r in parts]))
    return p0, steps


@functools.lru_cache(maxsize=None)
def dense_reference(n_rows, dim, dtype):
    """torch.optim.Adam on the CPU (single-tensor path); the gradient of a row is fp32(1/3) times the sum of its deposits' rows in
    deposit order, formed in ``dtype`` (exact in float64)."""
    p0, steps = scenario(n_rows, dim)
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([p], lr=LR0, foreach=False)
    for t, (_, deposits) in enumerate(steps, 1):
        opt.param_groups[0]["lr"] = lr_at(t)
        p.grad = torch.zeros_like(p)
        for rows, g in deposits:
            p.grad[rows] += g.to(dtype)
        p.grad *= torch.tensor(F32_THIRD, dtype=dtype)
        opt.step()
    st = opt.state[p]
    return p.detach().double(), st["exp_avg"].double(), st["exp_avg_sq"].double()


@functools.lru_cache(maxsize=None)
def lazy_sum_run(n_rows, dim):
    p0, steps = scenario(n_rows, dim)
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = LazyRowAdam([p], lr=LR0, lazy=[p], duplicates="sum")
    opt.grad_scale = F32_THIRD
    for t, (_, deposits) in enumerate(steps, 1):
        opt.param_groups[0]["lr"] = lr_at(t)
        opt.zero_grad()
        for rows, g in deposits:
            rows = rows.to(DEV)
            ops.group_input({0: p}, torch.zeros_like(rows), rows, dim).backward(g.to(DEV))
        opt.step()
        assert p.grad is None
    st = p._egnn_rows
    assert 1 <= st.flushed < STEPS, "70 steps must have forced a flush"
    opt.flush()                                            # raises if a gradient row was refused
    return p.detach().cpu(), st.m.cpu(), st.v.cpu(), st.last.cpu()


@pytest.mark.parametrize("n_rows,dim", SHAPES)
def test_summed_deposits_match_dense_adam_in_float64(n_rows, dim):
    """E_sum <= 4 E_ref + one fp32 ulp of max |x| for p, m and v, E_ref being torch's own fp32 CPU run against float64 (the bound of
    test_gpu_lazy_adam.py: both are fp32 chains of equal length, here including the same fp32 sums of three gradient rows)."""
    ref64 = dense_reference(n_rows, dim, torch.float64)
    ref32 = dense_reference(n_rows, dim, torch.float32)
    *got, last = lazy_sum_run(n_rows, dim)
    for name, r64, r32, x in zip("pmv", ref64, ref32, got):
        e_ref = float((r32 - r64).abs().max())
        e_sum = float((x.double() - r64).abs().max())
        bound = 4 * e_ref + ulp_at(float(r64.abs().max()))
        print(f"[adam rows sum {n_rows}x{dim}] {name}: E_ref={e_ref:.3e} E_sum={e_sum:.3e} bound={bound:.3e}")
        assert e_sum <= bound, (name, e_sum, e_ref, bound)
    p0, _ = scenario(n_rows, dim)
    never = list(NEVER)
    assert torch.equal(got[0][never], p0[never]) and (last[never] == -1).all()
    assert (last[[r for r in range(n_rows) if r not in NEVER]] == STEPS).all()


def test_data_parallel_row_list_keeps_every_deposit_of_every_table():
    """``dist._dp_local_rows`` (what a rank hands to the gather): two tables fed by separate ``group_input`` calls, one of them twice,
    all under type id 0 -- the merged list, applied as ONE deposit per table under the table's own id, gives the bits of the
    optimiser's own several-deposit step.  The usual case (one backward, the same arrays with every table) is passed on untouched."""
    from efficient_gnns_amd import dist as DD
    dim = 8
    gen = torch.Generator().manual_seed(4)
    a0, b0 = torch.randn(9, dim, generator=gen), torch.randn(5, dim, generator=gen)
    calls = [("a", torch.tensor([1, 7, 3])), ("b", torch.tensor([4, 0])), ("a", torch.tensor([3, 8, 1, 0]))]
    grads = [torch.randn(r.numel(), dim, generator=gen) for _, r in calls]

    def run(merge):
        t = {"a": torch.nn.Parameter(a0.clone().to(DEV)), "b": torch.nn.Parameter(b0.clone().to(DEV))}
        opt = LazyRowAdam(list(t.values()), lr=1e-2, lazy=list(t.values()), duplicates="sum")
        for _ in range(2):
            opt.zero_grad()
            for (name, rows), g in zip(calls, grads):
                rows = rows.to(DEV)
                ops.group_input({0: t[name]}, torch.zeros_like(rows), rows, dim).backward(g.to(DEV))
            if merge:
                tables = [(3, t["a"]._egnn_rows), (5, t["b"]._egnn_rows)]
                G, idx = DD._dp_local_rows(tables, dim, torch.device(DEV))
                assert G.shape[0] == sum(r.numel() for _, r in calls) and sorted(set(idx[:, 0].tolist())) == [3, 5]
                for k, st in tables:
                    st.deposits = [(G, idx[:, 0].contiguous(), idx[:, 1].contiguous(), k)]
            opt.step(grad_scale=0.5)
        opt.flush()
        return [p.detach().cpu() for p in t.values()] + [t["a"]._egnn_rows.m.cpu(), t["b"]._egnn_rows.v.cpu()]

    for x, y in zip(run(False), run(True)):
        assert torch.equal(x, y)
    # the usual case: one backward over both tables leaves the same arrays with each; they travel as they are
    t = {3: torch.nn.Parameter(a0.clone().to(DEV)), 5: torch.nn.Parameter(b0.clone().to(DEV))}
    opt = LazyRowAdam(list(t.values()), lr=1e-2, lazy=list(t.values()), duplicates="sum")
    nt, li = torch.tensor([3, 5, 3], device=DEV), torch.tensor([2, 1, 0], device=DEV)
    ops.group_input(t, nt, li, dim).backward(torch.ones(3, dim, device=DEV))
    G, idx = DD._dp_local_rows([(k, p._egnn_rows) for k, p in t.items()], dim, torch.device(DEV))
    assert G.data_ptr() == t[3]._egnn_rows.deposits[0][0].data_ptr() and torch.equal(idx, torch.stack([nt, li], dim=1))


# ---- 4. optimiser level --------------------------------------------------------------------------------------------------------
def test_two_deposits_for_one_table_are_summed_and_the_default_still_refuses():
    dim = 4
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(6, dim, generator=gen)
    rows_a, rows_b = torch.tensor([0, 2, 5]), torch.tensor([2, 0, 3])
    grads = [[torch.randn(3, dim, generator=gen) for _ in range(2)] for _ in range(2)]       # two steps, two deposits each

    def run(opt_of):
        p = torch.nn.Parameter(p0.clone().to(DEV))
        opt = opt_of(p)
        for ga, gb in grads:
            opt.zero_grad()
            for rows, g in ((rows_a, ga), (rows_b, gb)):
                rows = rows.to(DEV)
                ops.group_input({0: p}, torch.zeros_like(rows), rows, dim).backward(g.to(DEV))
            opt.step()
        return p, opt

    p, opt = run(lambda p: LazyRowAdam([p], lr=1e-2, lazy=[p], duplicates="sum"))
    assert p.grad is None and p._egnn_rows.t == 2
    opt.flush()                                                            # no refused row
    ref = torch.nn.Parameter(p0.clone())
    dense = torch.optim.Adam([ref], lr=1e-2, foreach=False)
    for ga, gb in grads:
        ref.grad = torch.zeros_like(ref)
        ref.grad[rows_a] += ga
        ref.grad[rows_b] += gb
        dense.step()
    err = float((p.detach().cpu() - ref.detach()).abs().max())
    assert err <= 8 * ulp_at(float(ref.detach().abs().max())), err                 # two steps of ~1e-2 each; a dropped deposit errs by ~1e-2
    with pytest.raises(RuntimeError, match="more than one gradient deposit"):
        run(lambda p: LazyRowAdam([p], lr=1e-2, lazy=[p]))
