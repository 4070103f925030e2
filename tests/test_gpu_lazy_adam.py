"""GPU checks of the row-lazy Adam (efficient-gnns_amd/optim.py, csrc/adam_rows.hip) and the one-launch group_input gather
(ops.group_input): the parameters after ``flush()`` against dense ``torch.optim.Adam`` in float64, "lazy == touched every step with a
zero gradient" bit for bit, rows read in the forward being current, the gather against the mask form, the unique-rows contract, and one
MAG-shaped epoch against ``torch.optim.Adam`` over the same model.

The bare-table tests run 70 steps (more than the 64-step ring, so the forced flush runs) over the same seeded sequence: lr 5e-3, then
1e-3 from step 30; gradient rows 0.1 * N(0, 1) drawn on the CPU; per step row 0 always, row 1 only at step 1, row 2 first at step 40
(then with probability 0.3), rows 3-5 never, every other row with probability 0.3.  The kernels are driven through the optimiser and
``ops.group_input`` (forward: catch-up + gather, backward: the deposit), no model.  References are computed once per shape."""
import functools

import numpy as np
import pytest
import torch

import efficient_gnns_amd as E
import efficient_gnns_amd.data as D
import efficient_gnns_amd.models as PM
import efficient_gnns_amd.utils as PU
from efficient_gnns_amd import _lib, ops
from efficient_gnns_amd.optim import MAX_LAG, LazyRowAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 70
LR0, LR1, LR_SWITCH = 5e-3, 1e-3, 30
SHAPES = [(37, 128), (11, 20), (9, 4)]
NEVER = (3, 4, 5)


@functools.lru_cache(maxsize=None)
def scenario(n_rows, dim):
    """(p0, [(rows, grads) per step]) on the CPU, fp32, fixed seed; rows sorted and unique."""
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
        steps.append((rows, 0.1 * torch.randn(rows.numel(), dim, generator=gen)))
    return p0, steps


def lr_at(t):
    return LR0 if t < LR_SWITCH else LR1


@functools.lru_cache(maxsize=None)
def dense_reference(n_rows, dim, dtype):
    """torch.optim.Adam on the CPU (single-tensor path) over the same gradients with the zero rows filled in: (p, m, v)."""
    p0, steps = scenario(n_rows, dim)
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([p], lr=LR0, foreach=False)
    for t, (rows, g) in enumerate(steps, 1):
        opt.param_groups[0]["lr"] = lr_at(t)
        p.grad = torch.zeros_like(p)
        p.grad[rows] = g.to(dtype)
        opt.step()
    st = opt.state[p]
    return p.detach().double(), st["exp_avg"].double(), st["exp_avg_sq"].double()


def lazy_step(opt, p, rows, g, t):
    """One training step on a bare table: the forward reads (and catches up) the rows, the backward deposits their gradient rows."""
    opt.param_groups[0]["lr"] = lr_at(t)
    rows = rows.to(DEV)
    h = ops.group_input({0: p}, torch.zeros_like(rows), rows, p.shape[1])
    opt.zero_grad()
    h.backward(g.to(DEV))
    opt.step()
    assert p.grad is None
    return h


def lazy_run(n_rows, dim, mode="lazy", upto=STEPS, duplicate_at=None):
    """mode 'lazy': flush only where the optimiser forces one; 'flush': after every step; 'zeros': every row named every step, the
    untouched ones with a zero gradient row.  Returns (param, optimiser) WITHOUT the final flush."""
    p0, steps = scenario(n_rows, dim)
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = LazyRowAdam([p], lr=LR0, lazy=[p])
    for t, (rows, g) in enumerate(steps[:upto], 1):
        if mode == "zeros":
            full = torch.zeros(n_rows, dim)
            full[rows] = g
            rows, g = torch.arange(n_rows), full
        if duplicate_at == t:
            rows, g = torch.cat([rows, rows[:1]]), torch.cat([g, g[:1]])
        lazy_step(opt, p, rows, g, t)
        if mode == "flush":
            opt.flush()
    return p, opt


def pmv(p):
    st = p._egnn_rows
    return p.detach().cpu(), st.m.cpu(), st.v.cpu()


def ulp_at(x):
    return float(np.spacing(np.float32(x)))


@functools.lru_cache(maxsize=None)
def lazy_flushed(n_rows, dim):
    p, opt = lazy_run(n_rows, dim)
    assert p._egnn_rows.flushed >= 1, "70 steps must have forced a flush"
    assert p._egnn_rows.flushed < STEPS
    opt.flush()
    return pmv(p) + (p._egnn_rows.last.cpu(),)


# ---- 1. against dense Adam in float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,dim", SHAPES)
def test_lazy_adam_matches_dense_adam_in_float64(n_rows, dim):
    """E_lazy <= 4 E_ref + one fp32 ulp of max |x| for p, m and v, E_ref being torch's own fp32 CPU run against float64: both are fp32
    chains of equal length whose sqrt and division may round differently at each step; a missed or doubled replay step or a wrong bias
    correction errs by the order of lr * 1e-2.  Never-touched rows stay bit-equal to their initial values with last == -1."""
    ref64 = dense_reference(n_rows, dim, torch.float64)
    ref32 = dense_reference(n_rows, dim, torch.float32)
    *got, last = lazy_flushed(n_rows, dim)
    for name, r64, r32, x in zip("pmv", ref64, ref32, got):
        e_ref = float((r32 - r64).abs().max())
        e_lazy = float((x.double() - r64).abs().max())
        bound = 4 * e_ref + ulp_at(float(r64.abs().max()))
        print(f"[lazy adam {n_rows}x{dim}] {name}: E_ref={e_ref:.3e} E_lazy={e_lazy:.3e} bound={bound:.3e}")
        assert e_lazy <= bound, (name, e_lazy, e_ref, bound)
    p0, _ = scenario(n_rows, dim)
    never = list(NEVER)
    assert torch.equal(got[0][never], p0[never])
    assert (got[1][never] == 0).all() and (got[2][never] == 0).all()
    assert (last[never] == -1).all()
    touched = [r for r in range(n_rows) if r not in NEVER]
    assert (last[touched] == STEPS).all()


# ---- 2. lazy == eager, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,dim", SHAPES)
def test_lazy_equals_flush_every_step_equals_explicit_zero_rows(n_rows, dim):
    lazy = lazy_flushed(n_rows, dim)[:3]
    for mode in ("flush", "zeros"):
        p, opt = lazy_run(n_rows, dim, mode)
        opt.flush()
        for name, a, b in zip("pmv", lazy, pmv(p)):
            assert torch.equal(a, b), (mode, name, float((a - b).abs().max()))


# ---- 3. rows read in the forward are current -----------------------------------------------------------------------------------
def test_forward_reads_current_rows_without_a_flush():
    """Row 1 had its only gradient at step 1.  After 50 steps (no flush has run: 50 < MAX_LAG) a forward over it must return what the
    flush-after-every-step run holds at step 50, bit for bit, under no_grad too."""
    n_rows, dim = SHAPES[0]
    assert 50 < MAX_LAG
    eager, opt_e = lazy_run(n_rows, dim, "flush", upto=50)
    lazy, opt_l = lazy_run(n_rows, dim, "lazy", upto=50)
    st = lazy._egnn_rows
    assert st.flushed == 0 and int(st.last[1]) == 1
    assert not torch.equal(lazy.detach()[1], eager.detach()[1]), "the stored row is behind before it is read"
    rows = torch.tensor([1, 3, 0], device=DEV)
    with torch.no_grad():
        h = ops.group_input({0: lazy}, torch.zeros_like(rows), rows, dim)
    assert torch.equal(h, eager.detach()[rows])
    assert int(st.last[1]) == 50 and int(st.last[3]) == -1 and st.flushed == 0
    # every other lag the sequence holds at step 50 (rows last touched at any earlier step), still without a flush
    rows = torch.arange(n_rows, device=DEV)
    with torch.no_grad():
        h = ops.group_input({0: lazy}, torch.zeros_like(rows), rows, dim)
    assert torch.equal(h, eager.detach()) and st.flushed == 0


# ---- 4. the gather against the mask form ---------------------------------------------------------------------------------------
def mask_form(sources, node_type, local_idx, dim):
    """The mask path of ``RGCN.group_input`` itself (no table carries row state), called on a stand-in for the model."""
    import types
    stand_in = types.SimpleNamespace(in_channels=dim, emb_dict={})
    return PM.RGCN.group_input(stand_in, sources, node_type, local_idx)


@pytest.mark.parametrize("dim", [128, 20])
@pytest.mark.parametrize("n", [1, 333])
def test_group_input_equals_the_mask_form(n, dim):
    """4 node types, type 2 absent from the batch, more than one workgroup at n = 333 (8 or 32 rows per workgroup)."""
    gen = torch.Generator().manual_seed(n + dim)
    sizes = {0: 50, 1: 7, 2: 13, 3: 29}
    sources = {k: torch.randn(s, dim, generator=gen).to(DEV) for k, s in sizes.items()}
    node_type = torch.tensor([0, 1, 3], dtype=torch.int64)[torch.randint(0, 3, (n,), generator=gen)]
    local_idx = (torch.rand(n, generator=gen) * torch.tensor([sizes[int(k)] for k in node_type])).long()
    node_type, local_idx = node_type.to(DEV), local_idx.to(DEV)
    oob = torch.zeros(1, dtype=torch.int32, device=DEV)
    h = ops.group_input(sources, node_type, local_idx, dim, oob=oob)
    assert torch.equal(h, mask_form(sources, node_type, local_idx, dim))
    assert int(oob) == 0
    # a type without a source gives zero rows, like the mask form
    part = {k: v for k, v in sources.items() if k != 1}
    assert torch.equal(ops.group_input(part, node_type, local_idx, dim, oob=oob), mask_form(part, node_type, local_idx, dim))
    assert int(oob) == 0


def test_group_input_reports_out_of_range_rows_and_writes_zeros():
    dim = 20
    sources = {0: torch.randn(5, dim, device=DEV), 1: torch.randn(3, dim, device=DEV)}
    node_type = torch.tensor([0, 1, 1, 0, 2, 0], device=DEV)
    local_idx = torch.tensor([4, 3, 2, -1, 0, 1], device=DEV)        # row 1: index 3 of a 3-row table; row 3: negative; row 4: type 2
    oob = torch.zeros(1, dtype=torch.int32, device=DEV)
    h = ops.group_input(sources, node_type, local_idx, dim, oob=oob)
    assert int(oob) == 3
    assert (h[[1, 3, 4]] == 0).all()
    assert torch.equal(h[0], sources[0][4]) and torch.equal(h[2], sources[1][2]) and torch.equal(h[5], sources[0][1])


def test_flush_reports_rows_the_default_counter_saw_out_of_range():
    """The model path passes no ``oob`` of its own: ``LazyRowAdam.flush`` reads the per-device counter and raises; the gradient of a
    dense source skips the zero-filled rows instead of indexing with them."""
    dim = 20
    ops.group_input_oob(DEV)                                         # start from a clean counter
    table = torch.nn.Parameter(torch.randn(5, dim, device=DEV))
    feats = torch.randn(3, dim, device=DEV, requires_grad=True)      # a dense source: no row state
    opt = LazyRowAdam([table], lr=1e-3, lazy=[table])
    node_type = torch.tensor([0, 1, 1, 0], device=DEV)
    local_idx = torch.tensor([4, 3, 2, 1], device=DEV)               # row 1: index 3 of the 3-row source
    h = ops.group_input({0: table, 1: feats}, node_type, local_idx, dim)
    assert (h[1] == 0).all() and torch.equal(h[2], feats.detach()[2])
    opt.zero_grad()
    h.backward(torch.ones_like(h))
    assert table.grad is None
    want = torch.zeros(3, dim, device=DEV)
    want[2] = 1
    assert torch.equal(feats.grad, want)
    opt.step()
    with pytest.raises(RuntimeError, match="out of range"):
        opt.flush()
    opt.flush()                                                      # reported once
    assert ops.group_input_oob(DEV) == 0


# ---- 5. the unique-rows contract -----------------------------------------------------------------------------------------------
def test_duplicate_row_in_a_batch_is_reported_by_flush():
    """Step 10 names row 0 twice (a plain wrong input).  The next flush raises; every other row is what the clean run holds."""
    n_rows, dim = SHAPES[1]
    clean, opt_c = lazy_run(n_rows, dim, upto=12)
    opt_c.flush()
    dup, opt_d = lazy_run(n_rows, dim, upto=12, duplicate_at=10)
    with pytest.raises(RuntimeError, match="table #0"):
        opt_d.flush()
    others = list(range(1, n_rows))
    for a, b in zip(pmv(clean), pmv(dup)):
        assert torch.equal(a[others], b[others])
    opt_d.flush()                                    # reported once


def test_two_deposits_in_one_step_change_no_table_and_close_detaches():
    dim = 4
    a = torch.nn.Parameter(torch.randn(6, dim, device=DEV))
    b = torch.nn.Parameter(torch.randn(6, dim, device=DEV))
    opt = LazyRowAdam([a, b], lr=1e-2, lazy=[a, b])
    rows = torch.tensor([0, 2], device=DEV)
    zeros = torch.zeros_like(rows)
    opt.zero_grad()
    ops.group_input({0: a}, zeros, rows, dim).sum().backward()
    ops.group_input({0: b}, zeros, rows, dim).sum().backward()
    ops.group_input({0: b}, zeros, rows, dim).sum().backward()       # b twice
    a0 = a.detach().clone()
    with pytest.raises(RuntimeError, match="more than one gradient deposit"):
        opt.step()
    assert a._egnn_rows.t == 0 and b._egnn_rows.t == 0 and torch.equal(a.detach(), a0)      # a did not advance either
    ops.group_input({0: a}, zeros, rows, dim).sum().backward()
    opt.step()
    assert a._egnn_rows.t == 1 and b._egnn_rows.t == 1
    with pytest.raises(NotImplementedError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, 4, device=DEV))]})
    opt.close()
    assert not hasattr(a, "_egnn_rows") and not hasattr(b, "_egnn_rows")
    h = ops.group_input({0: a}, zeros, rows, dim)                    # a dense source again: a dense gradient
    h.sum().backward()
    assert a.grad is not None and float(a.grad.sum()) == 2 * dim
    # a state whose optimiser is gone is flushed and dropped by the next reader
    c = torch.nn.Parameter(torch.randn(6, dim, device=DEV))
    opt = LazyRowAdam([c], lr=1e-2, lazy=[c])
    del opt
    import gc
    gc.collect()
    ops.group_input({0: c}, zeros, rows, dim).sum().backward()
    assert not hasattr(c, "_egnn_rows") and c.grad is not None


# ---- 6. model level ------------------------------------------------------------------------------------------------------------
def _mag_setup():
    from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler
    d = D.mag_hetero_like(0.01, seed=2)
    eid = dict(d.edge_index_dict)
    for key, rev in ((("author", "affiliated_with", "institution"), ("institution", "to", "author")),
                     (("author", "writes", "paper"), ("paper", "to", "author")),
                     (("paper", "has_topic", "field_of_study"), ("field_of_study", "to", "paper"))):
        r, c = eid[key]
        eid[rev] = torch.stack([c, r])
    eid[("paper", "cites", "paper")] = PU.to_undirected(eid[("paper", "cites", "paper")])
    edge_index, edge_type, node_type, local_idx, l2g, key2int = PU.group_hetero_graph(eid, d.num_nodes_dict)
    N = node_type.numel()
    homo = Data(edge_index=edge_index, edge_attr=edge_type, node_type=node_type, local_node_idx=local_idx, num_nodes=N)
    homo.y = node_type.new_full((N, 1), -1)
    homo.y[l2g["paper"]] = d.y_dict["paper"]
    homo.train_mask = torch.zeros(N, dtype=torch.bool)
    homo.train_mask[l2g["paper"][d.split_idx["train"]["paper"]]] = True
    loader = GraphSAINTRandomWalkSampler(homo.to(DEV), batch_size=200, walk_length=2, num_steps=6, sample_coverage=0, save_dir=None, seed=7)
    batches = list(loader)
    assert len(batches) == 6
    x_dict = {key2int["paper"]: d.x_dict["paper"].to(DEV)}
    nn_dict = {key2int[k]: n for k, n in d.num_nodes_dict.items()}
    return d, eid, key2int, batches, x_dict, nn_dict


def test_mag_epoch_equals_dense_adam():
    """One epoch of 6 GraphSAINT batches, RGCN 2 x 16, three optimisers over identically initialised models and identical dropout draws.
    Every parameter of the lazy run lies within 4 x the largest difference between torch's fused and single-tensor runs (the reference's
    own spread) plus one ulp of max |p|; the accuracies are equal; no table ever gets a dense gradient; the state loads into torch."""
    d, eid, key2int, batches, x_dict, nn_dict = _mag_setup()
    hp = dict(alpha=0.9, kd_T=4.0)
    eid_dev = {k: v.to(DEV) for k, v in eid.items()}
    runs = {}
    for name in ("fused", "single", "lazy"):
        torch.manual_seed(0)
        model = PM.RGCN(128, 16, d.num_classes, 2, 0.5, nn_dict, list(x_dict.keys()), len(eid)).to(DEV)
        if name == "lazy":
            opt = PM.mag_optimizer(model, 0.005)
            assert isinstance(opt, E.LazyRowAdam)
        else:
            opt = torch.optim.Adam(model.parameters(), lr=0.005, **({"fused": True} if name == "fused" else {"foreach": False}))
        torch.manual_seed(1)
        loss = PM.mag_train_epoch(model, batches, x_dict, opt, "supervised", hp)[0]
        assert loss == loss and loss > 0
        accs = PM.mag_test(model, x_dict, eid_dev, key2int, d.y_dict["paper"].to(DEV), d.split_idx)
        runs[name] = (model, opt, accs)
    lazy_model, lazy_opt, _ = runs["lazy"]
    for emb in lazy_model.emb_dict.values():
        assert emb.grad is None and emb._egnn_rows.t == 6 and emb._egnn_rows.flushed == 6
    assert runs["fused"][2] == runs["single"][2] == runs["lazy"][2]
    params = {k: [p.detach().double() for p in runs[k][0].parameters()] for k in runs}
    names = [n for n, _ in lazy_model.named_parameters()]
    spread = max(float((a - b).abs().max()) for a, b in zip(params["fused"], params["single"]))
    print(f"[lazy adam mag epoch] spread of the two torch runs = {spread:.3e}")
    for n, a, b, c in zip(names, params["lazy"], params["fused"], params["single"]):
        err = max(float((a - b).abs().max()), float((a - c).abs().max()))        # against BOTH torch runs
        bound = 4 * spread + ulp_at(float(b.abs().max()))
        print(f"[lazy adam mag epoch] {n}: err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (n, err, bound)
    dense = torch.optim.Adam(lazy_model.parameters(), lr=0.005)
    dense.load_state_dict(lazy_opt.state_dict())
    for p in lazy_model.parameters():
        s = dense.state[p]
        assert int(s["step"]) == 6
        for key in ("exp_avg", "exp_avg_sq"):
            assert s[key].shape == p.shape and bool(torch.isfinite(s[key]).all())
    for emb in lazy_model.emb_dict.values():
        assert torch.equal(dense.state[emb]["exp_avg"], emb._egnn_rows.m) and float(dense.state[emb]["exp_avg_sq"].max()) > 0
