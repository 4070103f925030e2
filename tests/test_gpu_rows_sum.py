"""GPU checks of row gathers with repeated ids (csrc/rows_sum.hip: egnn_rows_plan_build_i64, egnn_rows_add_runs_f32; ``ops.rows_plan`` and
``duplicates="sum"`` of take_rows / linear_rows / gather_normalize; ``lazy.LazyRows`` under dropin/accel.py).

The kernel is held to float64 ``index_add_`` within the bound of ANY order of k fp32 additions (gamma_k, derived, not measured); the ops
to float64 autograd of torch's ``x[idx]`` at the bar of tests/test_gpu_parity.py::test_linear_rows_fused_gather_gemm_vs_torch; the drop-in
to plain torch modules at the bar of tests/test_gpu_training_parity.py::test_dropin_accel_modules_match_torch."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import efficient_gnns_amd.lazy as lazy
import efficient_gnns_amd.ops as ops
from efficient_gnns_amd import _lib
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = int(re.search(r"#define\s+EGNN_ROWS_SUM_CHUNK\s+(\d+)", open(os.path.join(ROOT, "include", "egnn_hip.h")).read()).group(1))
HUB = 3 * CHUNK + 5


def close(actual, ref, rtol=1e-5, atol_scale=1e-6, msg=""):
    a, r = actual.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    np.testing.assert_allclose(a, r, rtol=rtol, atol=atol_scale * (np.abs(r).max() if r.size else 0.0) + 1e-30, err_msg=msg)


# ------------------------------------------------------------------------------------------------
# the kernels through the C ABI
# ------------------------------------------------------------------------------------------------
def build_plan(idx, n_rows):
    """(sorted keys as int64 bits, the four counters, shift) of a device index tensor, straight from egnn_rows_plan_build_i64."""
    lib, S = _lib.load(), idx.numel()
    keys = torch.empty(S, dtype=torch.int64, device=DEV)
    counters = torch.full((4,), -7, dtype=torch.int32, device=DEV)           # the call writes them: no zeroing by the caller
    nws = lib.egnn_rows_plan_ws_bytes(S, n_rows)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    _lib.check(lib.egnn_rows_plan_build_i64(_lib.ptr(idx), S, n_rows, _lib.ptr(keys), _lib.ptr(counters), _lib.ptr(ws), nws, _lib.stream()),
               "egnn_rows_plan_build_i64")
    return keys, counters.tolist(), max(1, (S - 1).bit_length())


def add_runs(dst, keys, shift, src, C, accumulate):
    lib, S = _lib.load(), src.shape[0]
    nws = lib.egnn_rows_add_runs_ws_bytes(S, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV) if nws else None
    _lib.check(lib.egnn_rows_add_runs_f32(_lib.ptr(dst), dst.stride(0), dst.shape[0], _lib.ptr(keys), S, shift, _lib.ptr(src), src.stride(0), C,
                                          accumulate, _lib.ptr(ws), nws, _lib.stream()), "egnn_rows_add_runs_f32")


def patterns(n_rows, S, g):
    """name -> int64 [S'] row ids in [0, n_rows): every pattern the shape admits (a pattern that does not fit is not listed)."""
    out = {"one_row": torch.full((S,), n_rows - 1, dtype=torch.int64), "random": torch.randint(0, n_rows, (S,), generator=g)}
    out["unique"] = torch.randperm(n_rows, generator=g)[:min(S, n_rows)]
    if S >= HUB:                                             # a hub among singletons: crosses chunk boundaries, ragged tail of 5
        singles = torch.randperm(n_rows, generator=g)
        hub = int(singles[0])
        ids = torch.cat([torch.full((HUB,), hub, dtype=torch.int64), singles[1:1 + min(n_rows - 1, S - HUB)]])
        out["hub"] = ids[torch.randperm(ids.numel(), generator=g)]
    return out


def matrix(rows, C, ld, g, offset4=False):
    """fp32 [rows, C] on the device behind a pitch of ``ld`` floats; ``offset4``: starting 4 bytes past a 16-byte boundary."""
    flat = torch.randn(rows * ld + 4, generator=g).to(DEV)
    assert flat.data_ptr() % 16 == 0
    start = 1 if offset4 else 0
    return flat[start:start + rows * ld].view(rows, ld)[:, :C]


def check_case(n_rows, ids, C, padded, accumulate, g, offset4=False):
    S = ids.numel()
    ld = (C + 4) // 4 * 4 if padded else C                  # padded: the next multiple of 4 above C
    src, dst = matrix(S, C, ld, g, offset4), matrix(n_rows, C, ld, g)
    if not accumulate:
        dst.fill_(float("nan"))                              # every row must be written: named rows summed, the others zeroed
    dst0 = dst.clone()
    # half of the entries arrive negative, as torch allows: the plan wraps and counts them
    flip = torch.rand(S, generator=g) < 0.5
    raw = torch.where(flip, ids - n_rows, ids).to(DEV)
    keys, counters, shift = build_plan(raw, n_rows)
    counts = torch.bincount(ids, minlength=n_rows)
    assert counters == [0, S - int((counts > 0).sum()), int(flip.sum()), int(counts.max())], (counters, n_rows, S)
    add_runs(dst, keys, shift, src, C, accumulate)
    ref = torch.zeros(n_rows, C, dtype=torch.float64) if not accumulate else dst0.cpu().double()
    mag = ref.abs()
    ref.index_add_(0, ids, src.cpu().double())
    mag.index_add_(0, ids, src.cpu().double().abs())
    k = (counts + (1 if accumulate else 0)).double().clamp(min=1)
    gamma = (k * 2.0 ** -24 / (1 - k * 2.0 ** -24)).unsqueeze(1)
    got = dst.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert bool((err <= gamma * mag).all()), (n_rows, S, C, ld, accumulate, float((err - gamma * mag).max()))
    untouched = counts == 0
    if untouched.any():                                      # rows never named: kept (accumulate) or exactly zero
        assert torch.equal(dst.cpu()[untouched], dst0.cpu()[untouched] if accumulate else torch.zeros(int(untouched.sum()), C))
    again = dst0.clone()
    add_runs(again, keys, shift, src, C, accumulate)
    assert torch.equal(again, dst), "two calls differ"
    if int(counts.max()) <= 1:                               # unique ids: the bits of the unique-contract kernels
        want = dst0.clone() if accumulate else torch.zeros_like(dst0)
        if accumulate:
            idx_dev = ids.to(DEV)
            _lib.check(_lib.load().egnn_rows_add_f32(_lib.ptr(want), want.stride(0), _lib.ptr(idx_dev), _lib.ptr(src), src.stride(0), S, C,
                                                     _lib.stream()), "egnn_rows_add_f32")
        else:
            want.index_copy_(0, ids.to(DEV), src)
        assert torch.equal(dst, want)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("C", [1, 3, 4, 40, 256, 260])
def test_run_add_vs_float64_index_add(C, padded):
    g = torch.Generator().manual_seed(1000 * C + padded)
    for n_rows in (1, 7, 300):
        for S in (1, 2, 1000):
            for name, ids in patterns(n_rows, S, g).items():
                for accumulate in (0, 1):
                    check_case(n_rows, ids, C, padded, accumulate, g)


def test_run_add_scalar_path_for_a_source_4_bytes_off():
    g = torch.Generator().manual_seed(5)
    for name, ids in patterns(300, 1000, g).items():
        for accumulate in (0, 1):
            check_case(300, ids, 40, False, accumulate, g, offset4=True)


def test_plan_counts_an_id_out_of_range_and_gives_it_no_key():
    n_rows = 7
    ids = torch.tensor([3, 7, 0, -8, 3, -7, 6], dtype=torch.int64)          # 7 and -8 are outside [-7, 7)
    keys, counters, shift = build_plan(ids.to(DEV), n_rows)
    assert counters == [2, 2, 1, 2]                  # 2 out of range; rows 0 and 3 are named twice; one wrapped (-7 -> 0); longest run 2
    k = keys.cpu().numpy().view(np.uint64)
    assert list(k[-2:]) == [np.uint64(2 ** 64 - 1)] * 2                      # the two entries without a key sort last
    rows, pos = (k[:-2] >> np.uint64(shift)).astype(np.int64), (k[:-2] & np.uint64((1 << shift) - 1)).astype(np.int64)
    assert list(zip(rows, pos)) == [(0, 2), (0, 5), (3, 0), (3, 4), (6, 6)]
    # the sum skips them: only keyed entries reach dst
    src = torch.arange(7 * 4, dtype=torch.float32, device=DEV).view(7, 4)
    dst = torch.full((n_rows, 4), float("nan"), device=DEV)
    add_runs(dst, keys, shift, src, 4, 0)
    ref = torch.zeros(n_rows, 4)
    ref.index_add_(0, torch.tensor([3, 0, 3, 0, 6]), src.cpu()[[0, 2, 4, 5, 6]])
    assert torch.equal(dst.cpu(), ref)


# ------------------------------------------------------------------------------------------------
# ops: duplicates="sum" against float64 autograd of torch's x[idx]
# ------------------------------------------------------------------------------------------------
SHAPES = [(513, 64, 40, 2000), (700, 130, 72, 300)]


def dup_index(n, m, g):
    """torch.randint(n, (m,)) plus one hub (as long as m allows, up to a run of several chunks)."""
    idx = torch.randint(n, (m,), generator=g)
    hub = min(m // 2, HUB)
    idx[torch.randperm(m, generator=g)[:hub]] = int(torch.randint(n, (1,), generator=g))
    assert idx.unique().numel() < m
    return idx


@pytest.mark.parametrize("n,C,P,m", SHAPES)
def test_take_rows_and_gather_normalize_sum_vs_float64(n, C, P, m):
    g = torch.Generator().manual_seed(n + m)
    x, idx, gy = torch.randn(n, C, generator=g), dup_index(n, m, g), torch.randn(m, C, generator=g)
    for fn, ref_fn in ((lambda t, i: ops.take_rows(t, i, duplicates="sum"), lambda t, i: t[i]),
                       (lambda t, i: ops.gather_normalize(t, i, duplicates="sum"), lambda t, i: F.normalize(t[i], p=2, dim=-1))):
        xd = x.double().requires_grad_(True)
        ref = ref_fn(xd, idx)
        ref.backward(gy.double())
        xg = x.to(DEV).requires_grad_(True)
        y = fn(xg, idx.to(DEV))
        y.backward(gy.to(DEV))
        close(y, ref)
        close(xg.grad, xd.grad)


@pytest.mark.parametrize("tap", [False, True])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,C,P,m", SHAPES)
def test_linear_rows_sum_vs_float64(n, C, P, m, padded, tap):
    g = torch.Generator().manual_seed(n + C + m)
    x, w, b = torch.randn(n, C, generator=g), torch.randn(P, C, generator=g) * 0.1, torch.randn(P, generator=g)
    w1, g1 = torch.randn(24, C, generator=g) * 0.1, torch.randn(n, 24, generator=g)
    idx, gy = dup_index(n, m, g), torch.randn(m, P, generator=g)
    xd, wd, bd, w1d = (t.double().requires_grad_(True) for t in (x, w, b, w1))
    hd = xd * 2.0
    ref = F.linear(hd[idx], wd, bd)
    ((ref * gy.double()).sum() + ((F.linear(hd, w1d) * g1.double()).sum() if tap else 0.0)).backward()
    xg = x.to(DEV)
    if padded:
        xg = ops.pad_pitch(xg)
        assert xg.stride(0) % 4 == 0 and xg.shape == (n, C)
    xg.requires_grad_(True)
    wg, bg, w1g = (t.to(DEV).requires_grad_(True) for t in (w, b, w1))
    h = xg * 2.0
    if padded:
        h = ops.pad_pitch(h)
    if tap:
        h = ops.grad_tap(h)
    y = ops.linear_rows(h, idx.to(DEV), wg, bg, duplicates="sum")
    ((y * gy.to(DEV)).sum() + ((ops.linear(h, w1g) * g1.to(DEV)).sum() if tap else 0.0)).backward()
    close(y, ref)
    close(wg.grad, wd.grad)
    close(bg.grad, bd.grad)
    close(xg.grad, xd.grad)
    if tap:
        close(w1g.grad, w1d.grad)


@pytest.mark.parametrize("n,C,Ks,m", [(700, 64, 7, 2000), (1300, 128, 40, 300)])
def test_tap_rows_with_a_plan_under_the_fused_last_layer(n, C, Ks, m):
    """``ops.bn_act_linear`` owns the tap of the last hidden layer: a piece that comes with a plan must leave its fused backward (which
    reads tap rows through the inverse row map of unique ids) for the separate passes.  Against bn_act -> grad_tap -> matmul, whose
    run-sum is held to float64 above; the bar of test_gpu_parity.py::test_bn_act_linear_equals_the_three_separate_ops."""
    g = torch.Generator().manual_seed(n + Ks)
    x0 = (torch.randn(n, C, generator=g) * 2 + torch.randn(C, generator=g)).to(DEV)
    w0, wp0 = (torch.randn(C, Ks, generator=g) * 0.1).to(DEV), (torch.randn(32, C, generator=g) * 0.1).to(DEV)
    idx = dup_index(n, m, g).to(DEV)
    g_xw, g_rows = torch.randn(n, Ks, generator=g).to(DEV), torch.randn(m, 32, generator=g).to(DEV)
    res = []
    for fused in (False, True):
        bn = torch.nn.BatchNorm1d(C).to(DEV)
        x, w, wp = (t.clone().requires_grad_(True) for t in (x0, w0, wp0))
        if fused:
            h, xw = ops.bn_act_linear(x, bn, w, relu=True, p=0.0, training=True)
        else:
            h = ops.grad_tap(ops.bn_act(x, bn, relu=True, p=0.0, training=True))
            xw = ops.matmul(h, w)
        ((xw * g_xw).sum() + (ops.linear_rows(h, idx, wp, duplicates="sum") * g_rows).sum()).backward()
        res.append((x.grad, w.grad, wp.grad, bn.weight.grad, bn.bias.grad))
    for name, u, v in zip(("dx", "dW", "dWp", "dgamma", "dbeta"), *res):
        close(v, u, rtol=2e-5, atol_scale=2e-6, msg=name)


@pytest.mark.parametrize("n,C,P,m", [(513, 64, 40, 300), (700, 130, 72, 300)])
def test_unique_ids_take_the_same_bits_under_sum_and_unique(n, C, P, m, monkeypatch):
    g = torch.Generator().manual_seed(m + C)
    x, w, b = torch.randn(n, C, generator=g).to(DEV), (torch.randn(P, C, generator=g) * 0.1).to(DEV), torch.randn(P, generator=g).to(DEV)
    w1, idx = (torch.randn(24, C, generator=g) * 0.1).to(DEV), torch.randperm(n, generator=g)[:m].to(DEV)
    gy, gc = torch.randn(m, P, generator=g).to(DEV), torch.randn(m, C, generator=g).to(DEV)

    def run(mode):
        out = []
        for fn, go in ((lambda t: ops.take_rows(t, idx, duplicates=mode), gc), (lambda t: ops.gather_normalize(t, idx, duplicates=mode), gc)):
            xg = x.clone().requires_grad_(True)
            y = fn(xg)
            y.backward(go)
            out += [y.detach(), xg.grad]
        for tap in (False, True):
            xg, wg, bg, w1g = (t.clone().requires_grad_(True) for t in (x, w, b, w1))
            h = xg * 2.0
            h = ops.grad_tap(h) if tap else h
            y = ops.linear_rows(h, idx, wg, bg, duplicates=mode)
            ((y * gy).sum() + (ops.linear(h, w1g).square().sum() if tap else 0.0)).backward()
            out += [y.detach(), xg.grad, wg.grad, bg.grad] + ([w1g.grad] if tap else [])
        return out
    a = run("unique")
    plan = ops.rows_plan(idx, n)
    assert plan.dups == 0 and plan.keys is None and plan.idx.data_ptr() == idx.data_ptr()
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the plan of a known index tensor touched the library again"))
    assert ops.rows_plan(idx, n) is plan                                        # from the cache: no launch, no host read
    monkeypatch.undo()
    for u, v in zip(a, run("sum")):
        assert torch.equal(u, v)


def test_an_id_out_of_range_raises_index_error_and_a_capture_refuses_the_build(monkeypatch):
    n = 50
    x = torch.randn(n, 8, device=DEV, requires_grad=True)
    bad = torch.tensor([0, 3, n, 3], device=DEV)
    for fn in (lambda: ops.take_rows(x, bad, duplicates="sum"), lambda: ops.gather_normalize(x, bad, duplicates="sum"),
               lambda: ops.linear_rows(x, bad, torch.randn(4, 8, device=DEV), duplicates="sum")):
        with pytest.raises(IndexError, match="out of range"):
            fn()
    neg = torch.tensor([-1, 3, -n, 3], device=DEV)                              # wrapped, as torch does
    y = ops.take_rows(x, neg, duplicates="sum")
    assert torch.equal(y, x[neg])
    y.sum().backward()
    assert torch.equal(x.grad, torch.zeros(n, 8, device=DEV).index_add_(0, neg % n, torch.ones(4, 8, device=DEV)))
    # the CPU-visible guard: first use of an index tensor while the stream is (said to be) capturing
    fresh = torch.tensor([1, 1, 2], device=DEV)
    monkeypatch.setattr(torch.cuda.graphs, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captur"):
        ops.take_rows(x, fresh, duplicates="sum")
    assert torch.equal(ops.take_rows(x, neg, duplicates="sum"), x[neg])         # a plan built by a warm-up step is simply used


# ------------------------------------------------------------------------------------------------
# the drop-in: a caller spelled like a PyG script, under accel against plain torch modules
# ------------------------------------------------------------------------------------------------
def load_accel():
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_rows", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    return accel


def assert_matches_plain_torch(accel, step, n_params):
    """``step()`` -> [input gradient, parameter gradients ...], once on plain torch modules and once under accel.enable()."""
    ref = step()
    accel.enable()
    try:
        got = step()
    finally:
        accel.disable()
    assert len(got) == len(ref) == 1 + n_params
    for a, b in zip(got, ref):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 2e-5 * scale + 1e-6, (a.shape, float((a - b).abs().max()), scale)


class Script:
    """BatchNorm1d -> F.relu -> F.dropout(training=False) -> h[train_idx], the way a PyG training script spells it."""
    n, C, n_train = 400, 64, 200

    def __init__(self):
        g = torch.Generator().manual_seed(0)
        self.x0 = (torch.randn(self.n, self.C, generator=g) * 2 + 0.5).to(DEV)
        self.train_idx = torch.randperm(self.n, generator=g)[:self.n_train].to(DEV)
        self.src = torch.randint(self.n_train, (1500,), generator=g).to(DEV)
        self.dst = torch.randint(self.n_train, (1500,), generator=g).to(DEV)
        self.sample = torch.randint(self.n, (600,), generator=g).to(DEV)
        self.seen = []

    def hidden(self):
        torch.manual_seed(1)
        bn, lin = torch.nn.BatchNorm1d(self.C).to(DEV), torch.nn.Linear(self.C, 16).to(DEV)
        x = self.x0.clone().requires_grad_(True)
        h = F.dropout(F.relu(bn(x)), p=0.5, training=False)
        self.seen.append(type(h).__name__)
        return bn, lin, x, h

    def lsp_cosine(self):
        bn, lin, x, h = self.hidden()
        f = h[self.train_idx]
        F.cosine_similarity(f[self.src], f[self.dst]).sum().backward()
        return [x.grad, bn.weight.grad, bn.bias.grad]

    def sampled_linear(self):
        bn, lin, x, h = self.hidden()
        lin(h[self.sample]).square().mean().backward()
        return [x.grad, bn.weight.grad, bn.bias.grad, lin.weight.grad, lin.bias.grad]


def test_dropin_edge_endpoints_of_train_rows_match_plain_torch():
    """Loss 1, the LSP cosine line: ``f = h[train_idx]`` then ``f[src]`` / ``f[dst]`` over 1 500 edges among 200 rows -- the composed
    index names every row ~7.5 times.  Before ``duplicates="sum"`` the deferred gather scattered with index_copy_ and each row kept
    ONE edge's gradient."""
    accel, s = load_accel(), Script()
    lazy._COMPOSED.clear()
    assert_matches_plain_torch(accel, s.lsp_cosine, 2)
    assert s.seen == ["Tensor", "LazyBnAct"]                                     # the second run did take the deferred path
    accel.enable()
    try:
        for _ in range(2):
            s.lsp_cosine()
    finally:
        accel.disable()
    assert len(lazy._COMPOSED) == 2                                              # (train_idx, src) and (train_idx, dst): per pair, not per step


def test_dropin_sampled_rows_with_replacement_match_plain_torch_and_the_memo_holds_one_entry():
    """Loss 2: ``Linear(h[torch.randint(n, (600,))])`` -- 600 draws with replacement from 400 rows, the row-compact gradient joining the
    dense one through the tap.  Then one composition, three steps: the composed-index memo holds ONE entry."""
    accel, s = load_accel(), Script()
    assert_matches_plain_torch(accel, s.sampled_linear, 4)
    assert s.seen == ["Tensor", "LazyBnAct"]
    lazy._COMPOSED.clear()
    ops._ROWS_PLANS.clear()
    accel.enable()
    try:
        for _ in range(3):
            bn, lin, x, h = s.hidden()
            lin(h[s.train_idx][s.src]).square().mean().backward()
    finally:
        accel.disable()
    assert len(lazy._COMPOSED) == 1 and len(ops._ROWS_PLANS) == 1               # one composed index, one plan, three steps


def test_dropin_in_place_change_between_indexing_and_use_raises():
    """``f = h[idx]`` of a constant tensor is deferred into the consuming Linear; ``h.mul_(2)`` in between must not leak into f."""
    accel = load_accel()
    accel._BIG_GATHER, accel._MIN_GATHER_ROWS = 1, 1
    h = torch.randn(400, 64, device=DEV)
    idx = torch.randint(400, (600,), device=DEV)
    lin = torch.nn.Linear(64, 16).to(DEV)
    accel.enable()
    try:
        f = h[idx]
        assert isinstance(f, lazy.LazyRows)
        want = lin(h[idx])                                                       # used before the change: fine
        h.mul_(2)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            lin(f)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            f + 1
        with torch.no_grad():
            assert float((lin(h[idx]) - (2 * (want - lin.bias) + lin.bias)).abs().max()) <= 1e-4   # indexing AFTER the change sees it
    finally:
        accel.disable()
