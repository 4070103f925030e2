"""Class-width aggregation (32 < K < 64, the 40-class output layer): the 16-lane form behind egnn_spmm_csr_blk_f32 against the
segment schedule it replaces (bit-equal: same cuts, same summation order per element) and against float64.

The graph has 300 rows and 300 source rows.  Source rows that no entry names hold NaN -- one between two named rows (100),
one directly behind the named block (250) and the rest up to 298; source 299, the last row of the descriptor's range, is
named.  A padded slot or a lane past K that touched memory would show up as a NaN.

K = 36 and 40 take the new form; K = 72 (two slices and a tail) stays on the row-block kernel it had and is held to the
same checks.  The split [N, 32] + [N, 8] source layout of the proposal was measured and not built, so there
is no producer-side test: the producers are unchanged."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 300
DEGS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129]   # both sides of the 8- / 16-slot step edges and of seg_max = 64; 129: three hub segments
NAMED = np.array([i for i in range(250) if i != 100] + [299])
SWITCH = "EGNN_SPMM_CLASS_WIDTH"


def _build_graph():
    rng = np.random.default_rng(7)
    rows = []
    for d in DEGS:
        rows.append(np.sort(rng.choice(NAMED, size=d, replace=False)))
    rows.append(np.full(5, 299))                        # row 12: every entry names the last source row
    rows.append(np.array([0]))                          # row 13: names source 0
    rows.append(np.array([5, 5, 5, 7, 7, 41, 41]))      # row 14: repeated column ids
    while len(rows) < N:
        rows.append(np.sort(rng.choice(NAMED, size=int(rng.integers(0, 21)), replace=False)))
    rows[N - 1] = np.array([0, 249, 299])               # the last row is not empty
    cnt = np.array([len(r) for r in rows])
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int64)
    return rowptr, col, cnt, rng


@pytest.fixture(scope="module")
def case():
    import efficient_gnns_amd as E
    dev = torch.device("cuda:0")
    rowptr, col, cnt, rng = _build_graph()
    assert set(np.unique(col)) <= set(NAMED) and {0, 299} <= set(col) and 100 not in col and 250 not in col
    val = rng.standard_normal(col.size).astype(np.float32)
    scale = (0.5 + rng.random(N)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    adj_v = E.SparseTensor(rowptr=t(rowptr), col=t(col), value=t(val), sparse_sizes=(N, N))
    adj_1 = E.SparseTensor(rowptr=t(rowptr), col=t(col), sparse_sizes=(N, N))
    xs, bias, addend = {}, {}, {}
    for K in (32, 36, 40, 72):
        x = rng.standard_normal((N, K)).astype(np.float32)
        named = np.zeros(N, bool)
        named[NAMED] = True
        x[~named] = np.nan
        xs[K] = t(x)
        bias[K] = t(rng.standard_normal(K).astype(np.float32))
        addend[K] = t(rng.standard_normal((N, K)).astype(np.float32))
    return dict(dev=dev, rowptr=rowptr, col=col, cnt=cnt, val=val, scale=t(scale), adj_v=adj_v, adj_1=adj_1, x=xs, bias=bias,
                addend=addend)


@pytest.fixture
def seg_calls(monkeypatch):
    """counts the calls of the segment schedule's entry point (the path the class widths ran on before)"""
    from efficient_gnns_amd import _lib
    lib = _lib.load()
    orig, calls = lib.egnn_spmm_csr_seg_f32, []
    monkeypatch.setattr(lib, "egnn_spmm_csr_seg_f32", lambda *a: (calls.append(1), orig(*a))[1])
    return calls


def _float64(c, K, reduce, use_val, use_bias, use_scale, use_addend):
    """(y64, magnitude of the summed terms) per element, from the named rows only"""
    col = torch.from_numpy(c["col"])
    row = torch.repeat_interleave(torch.arange(N), torch.from_numpy(c["cnt"]))
    x = c["x"][K].cpu().double()
    v = torch.from_numpy(c["val"]).double() if use_val else torch.ones(col.numel(), dtype=torch.float64)
    if use_scale:
        v = v * c["scale"].cpu().double()[col]
    terms = v[:, None] * x[col]
    inv = 1.0 / torch.from_numpy(np.maximum(c["cnt"], 1)).double() if reduce == "mean" else torch.ones(N, dtype=torch.float64)
    y = torch.zeros(N, K, dtype=torch.float64).index_add_(0, row, terms) * inv[:, None]
    mag = torch.zeros(N, K, dtype=torch.float64).index_add_(0, row, terms.abs()) * inv[:, None]
    if use_bias:
        b = c["bias"][K].cpu().double()
        y, mag = y + b, mag + b.abs()
    if use_addend:
        a = c["addend"][K].cpu().double()
        y, mag = y + a, mag + a.abs()
    return y, mag


def _within_float64_bound(c, y, K, reduce, use_val, use_bias, use_scale, use_addend, tag):
    """|y - y64| <= (d + 4) 2^-24 (sum_e |val_e x_e| inv + |bias| + |addend|), d = the row's entry count: recursive summation with
    one rounding per fmaf, plus the roundings of the partial combine, the scale and the bias"""
    y64, mag = _float64(c, K, reduce, use_val, use_bias, use_scale, use_addend)
    d = torch.from_numpy(c["cnt"]).double()[:, None]
    err = (y.cpu().double() - y64).abs()
    bound = (d + 4) * 2.0 ** -24 * mag
    print(f"{tag}: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    return bool((err <= bound).all())


VARIANTS = [("none", False, False, False, False), ("val", True, False, False, False), ("val_bias_scale", True, True, True, False)]


def _check(c, K, reduce, variant, seg_calls, monkeypatch):
    import efficient_gnns_amd.ops as ops
    name, use_val, use_bias, use_scale, use_addend = variant
    adj = c["adj_v"] if use_val else c["adj_1"]
    kw = dict(src_scale=c["scale"] if use_scale else None, bias=c["bias"][K] if use_bias else None,
              addend=c["addend"][K] if use_addend else None)
    x = c["x"][K]
    monkeypatch.delenv(SWITCH, raising=False)
    y = ops.spmm_raw(adj, x, reduce, **kw)[0]
    assert not seg_calls                                                  # the row-block entry point took the call
    assert torch.isfinite(y).all()                                        # no padded lane read a NaN row
    with monkeypatch.context() as m:                                      # the path of this width before the class-width form:
        m.setenv(SWITCH, "0")                                             # the segment schedule below 64 columns, the row-block kernel from there
        old = ops.spmm_raw(adj, x, reduce, **kw)[0]
    assert len(seg_calls) == (1 if K < 64 else 0)
    assert torch.equal(y, old)                                            # (a) bit-equal, all rows
    assert _within_float64_bound(c, y, K, reduce, use_val, use_bias, use_scale, use_addend, f"K={K} {reduce} {name}")   # (b)
    assert torch.equal(ops.spmm_raw(adj, x, reduce, **kw)[0], y)          # (c) run to run


@pytest.mark.parametrize("K", [36, 40, 72])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0])
def test_class_width_matches_segments_and_float64(case, seg_calls, monkeypatch, K, reduce, variant):
    _check(case, K, reduce, variant, seg_calls, monkeypatch)


def test_class_width_with_addend(case, seg_calls, monkeypatch):
    _check(case, 40, "sum", ("all_addend", True, True, True, True), seg_calls, monkeypatch)


def test_fallbacks_take_the_old_path_and_agree(case, seg_calls, monkeypatch):
    """(d) what the new form does not take runs where it ran before, and agrees"""
    import efficient_gnns_amd as E
    import efficient_gnns_amd.ops as ops
    c = case
    adj, x = c["adj_v"], c["x"][40]
    monkeypatch.delenv(SWITCH, raising=False)
    ref = ops.spmm_raw(adj, x, "sum")[0]
    assert not seg_calls
    # the environment switch: the segment schedule, as before
    monkeypatch.setenv(SWITCH, "0")
    assert torch.equal(ops.spmm_raw(adj, x, "sum")[0], ref) and len(seg_calls) == 1
    monkeypatch.delenv(SWITCH)
    # 64-bit indices
    t = lambda a: torch.from_numpy(a).to(c["dev"])  # noqa: E731
    adj64 = E.SparseTensor(rowptr=t(c["rowptr"]), col=t(c["col"]), value=t(c["val"]), sparse_sizes=(N, N))
    adj64._struct["idx"] = (adj64._rowptr, adj64._col, 64)
    assert torch.equal(ops.spmm_raw(adj64, x, "sum")[0], ref) and len(seg_calls) == 2
    # K = 32: one full 128-byte slice, not a class width
    y32 = ops.spmm_raw(adj, c["x"][32], "sum")[0]
    assert len(seg_calls) == 3 and torch.isfinite(y32).all()
    assert _within_float64_bound(c, y32, 32, "sum", True, False, False, False, "K=32")
    # statistics in the epilogue are not offered at this width, as before
    with pytest.raises(ops.HipStatsUnavailable):
        ops.spmm_raw(adj, x, "sum", want_stats=True)
    # a source that is not 16-byte aligned: the row-class schedule (another summation order: held to the float64 bound)
    buf = torch.empty(N * 40 + 1, dtype=torch.float32, device=c["dev"])
    mis = buf[1:].view(N, 40)
    mis.copy_(x)
    assert mis.data_ptr() % 16 != 0
    ym = ops.spmm_raw(adj, mis, "sum")[0]
    assert len(seg_calls) == 3 and torch.isfinite(ym).all()
    assert _within_float64_bound(c, ym, 40, "sum", True, False, False, False, "K=40 unaligned")


def test_one_training_step_is_bit_equal_with_the_form_on_and_off(monkeypatch):
    """One optimisation step and one evaluation of a small GCN (40 classes, dropout with a fixed seed) with the class-width form on and
    with EGNN_SPMM_CLASS_WIDTH=0: the summation order is kept, so losses, evaluation logits, every parameter gradient and every updated
    parameter are torch.equal."""
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.models as PM
    dev = torch.device("cuda:0")
    data = D.arxiv_like(scale=0.01, seed=1)
    x, adj, y = data.x.to(dev), data.adj_t.to(dev), data.y.to(dev)
    tr = data.split_idx["train"].to(dev)
    split = {k: v.to(dev) for k, v in data.split_idx.items()}
    teacher = data.teacher_logits.to(dev)
    hp = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=512, kernel="rbf")

    def run(switch):
        if switch is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, switch)
        torch.manual_seed(3)
        np.random.seed(3)
        model = PM.GCN(data.num_features, 64, data.num_classes, 3, 0.5).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        losses = PM.train_step(model, x, adj, y, tr, opt, "kd", hp, None, teacher)
        grads = [p.grad.clone() for p in model.parameters()]
        params = [p.detach().clone() for p in model.parameters()]
        out, accs = PM.evaluate(model, x, adj, y, split)
        return losses, grads, params, out, accs

    on, off = run(None), run("0")
    assert on[0] == off[0] and on[4] == off[4]
    assert all(torch.isfinite(g).all() for g in on[1]) and torch.isfinite(on[3]).all()
    for a, b in zip(on[1] + on[2] + [on[3]], off[1] + off[2] + [off[3]]):
        assert torch.equal(a, b)
