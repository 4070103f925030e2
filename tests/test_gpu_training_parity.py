"""Training-regime parity (run with ``-m gpu``): the configuration the benchmark times -- dropout 0.5, several optimisation
steps, eager launches AND hipGraph replays -- against the CPU oracle, made comparable by injecting the product's dropout masks
into the oracle's ``F.dropout`` (oracle/training_parity.py; /root/reference/arxiv_pyg/gnn.py:48-50,102-195).

Also the regression tests of the round-4 finding: a long torch reduction inside a replayed hipGraph can leave its output
unwritten on this stack (profiles/r04_lsp_trace.txt), so the step contains none and ``GraphedEpoch`` refuses to capture one.
"""
import math

import numpy as np
import pytest
import torch

import efficient_gnns_amd as E
import efficient_gnns_amd.data as D
import efficient_gnns_amd.models as PM
import efficient_gnns_amd.ops as ops
import efficient_gnns_amd.ops_edge as ops_edge
from efficient_gnns_amd import _lib
from efficient_gnns_amd._audit import CaptureAudit, LongReductionInCapture
from efficient_gnns_amd.utils import subgraph
import oracle.training_parity as TP
from oracle.dropout import counter_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=2048, kernel="cosine", proj_dim=64)


def to_dev(data):
    import types
    d = types.SimpleNamespace(**vars(data))
    d.x, d.y, d.adj_t = data.x.to(DEV), data.y.to(DEV), data.adj_t.to(DEV)
    d.split_idx = {k: v.to(DEV) for k, v in data.split_idx.items()}
    d.teacher_out_feat = ops.pad_pitch(data.teacher_out_feat.to(DEV))
    d.teacher_logits = data.teacher_logits.to(DEV)
    return d


@pytest.fixture(scope="module")
def small():
    data = D.arxiv_like(scale=0.1, seed=11)
    return data, to_dev(data)


@pytest.fixture(scope="module")
def full():
    data = D.arxiv_like(scale=1.0, seed=0)
    return data, to_dev(data)


@pytest.mark.parametrize("with_dev_seed", [False, True])
@pytest.mark.parametrize("p", [0.5, 0.25])
def test_counter_mask_restatement_equals_the_kernels_mask(p, with_dev_seed):
    """oracle/dropout.py::counter_mask against the mask the fused BatchNorm kernel applies (csrc/bn_common.h), bit for bit: a
    constant input makes y = beta * gate, i.e. the mask itself."""
    n, C = 3001, 256
    bn = torch.nn.BatchNorm1d(C).to(DEV)
    with torch.no_grad():
        bn.bias.fill_(1.0)
    x = torch.ones(n, C, device=DEV)
    dev_seed = 0x1234567890ABCDEF if with_dev_seed else 0
    prev = ops._DROPOUT_SEED_DEV
    ops._DROPOUT_SEED_DEV = torch.tensor([dev_seed], dtype=torch.int64, device=DEV) if with_dev_seed else None
    try:
        with TP.recorded_seeds(ops) as seeds:
            y = ops.bn_act(x, bn, relu=True, p=p, training=True)
    finally:
        ops._DROPOUT_SEED_DEV = prev
    assert len(seeds) == 1
    want = counter_mask((seeds[0] + dev_seed) & TP.MASK64, n, C, p)
    assert torch.equal(y.cpu(), want), float((y.cpu() != want).float().mean())
    assert abs(float((want == 0).float().mean()) - p) < 0.01


CASES = [("gcn", "nce"), ("gcn", "gpw"), ("gcn", "kd"), ("sage", "lpw"), ("sage", "nce")]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replay"])
@pytest.mark.parametrize("gnn,mode", CASES)
def test_training_trajectory_with_injected_dropout(small, gnn, mode, graph):
    """8 optimisation steps with dropout 0.5 (N = 16 934): every loss term of every step within 2e-4 of the oracle's (the bar of
    the golden trajectories), for eager launches and for GraphedEpoch replays (started from the post-warm-up state)."""
    data, d = small
    hp = dict(HP)
    if mode == "lpw":
        hp.update(beta=100.0)
    if mode == "gpw":
        hp.update(beta=100.0, max_samples=1024)
    r = TP.trajectory(PM, ops, data, d, DEV, gnn, mode, hp, steps=8, graph=graph, subgraph_fn=subgraph, hidden=128, seed=3)
    got, ref = np.array(r["got"]), np.array(r["ref"])
    assert np.isfinite(got).all()
    tag = f"{gnn}+{mode} {'replay' if graph else 'eager'}: max rel {r['max_rel']:.2e}"
    # Bars: the first 3 steps at the golden trajectories' 2e-4; later steps at 1.5e-3 -- Adam divides every gradient component by its
    # own running magnitude, so a component that is rounding noise on one side (an exactly cancelling sum on the other) moves its weight
    # by a full +-lr, and the two fp32 trajectories separate at a rate the reference's own CPU-vs-GPU runs would show as well (measured
    # here: 3e-5 after one step, 3.4e-4 after eight for SAGE + G-CRD at 1/tau = 13.3).  GSP (the mean squared DIFFERENCE of two Gram
    # matrices, 0.018 out of O(1) entries) amplifies operand rounding ~10x from the first step.
    for lo, hi, rtol in ((0, 3, 1.5e-3 if mode == "gpw" else 2e-4), (3, 8, 1.5e-3)):
        for col in (1, 2, 0):
            np.testing.assert_allclose(got[lo:hi, col], ref[lo:hi, col], rtol=rtol, atol=1e-7, err_msg=tag)
    assert len({tuple(g) for g in r["got"]}) == 8, "the steps must differ (weights and masks move)"


@pytest.mark.parametrize("kernel", ["rbf", "cosine"])
def test_lsp_replayed_training_full_size(full, kernel):
    """SAGE-256 + LSP at full size (N = 169 343, E_tr = 679 910), dropout 0.5, GraphedEpoch replays started on an idle device
    (the condition under which r03's replays reported loss_aux = 359): every replayed loss_aux respects the bound that holds for ANY
    finite features, (n_seg / E)(span + ln max_deg) with span = 1 (rbf) / 2 (cosine); the first 6 replays equal the oracle's steps
    with the same masks; rbf: all 25 replays stay at the oracle's value (the student's similarities underflow: 1.9076e-5)."""
    data, d = full
    hp = dict(HP, beta=100.0, kernel=kernel, max_samples=16384, proj_dim=256)
    steps_cmp, steps_all = 6, 25
    oracle, product = TP.build_pair(PM, data, d, DEV, "sage", "lpw", hp, 256, 3, 0.5, 0.01, seed=0)
    pm, _, _, popt = product
    edge_o, edge_p = TP.edges_of(data, d, "lpw", subgraph)
    with TP.recorded_seeds(ops) as seeds:
        ge = PM.GraphedEpoch(pm, d.x, d.adj_t, d.y, d.split_idx["train"], popt, "lpw", hp, d.teacher_out_feat, d.teacher_logits,
                             None, None, edge_index=edge_p, split_idx=d.split_idx, warmup=3)
    host_seeds = seeds[-2:]
    TP.sync_oracle_to(product, oracle)
    ge.redraw()
    torch.cuda.synchronize()
    deg = torch.bincount(edge_o[1], minlength=data.split_idx["train"].numel())
    bound = float((deg > 0).sum()) / edge_o.shape[1] * ((1.0 if kernel == "rbf" else 2.0) + math.log(int(deg.max())))
    got, seeds_by_step = [], []
    for _ in range(steps_all):
        dev_seed = int(ge._seed_dev.item())
        losses, accs = ge.step()
        got.append(losses)
        seeds_by_step.append([(h + dev_seed) & TP.MASK64 for h in host_seeds])
        assert 0.0 <= losses[2] <= bound, (losses, bound)
        assert abs(losses[0] - (losses[1] + 100.0 * losses[2])) <= 1e-5 * abs(losses[0])
    dc = TP.oracle_data(data)
    masks = [TP.masks_for(s, data.num_nodes, 256, 0.5) for s in seeds_by_step[:steps_cmp]]
    ref = TP.oracle_steps(oracle, dc, "lpw", hp, edge_o, masks, 0)
    g, r = np.array(got[:steps_cmp]), np.array(ref)
    np.testing.assert_allclose(g[:, :2], r[:, :2], rtol=2e-4)
    # loss_aux: the KL of two nearly uniform distributions is a small difference of O(1) sums (condition ~1e3, bench.parity_check)
    np.testing.assert_allclose(g[:, 2], r[:, 2], rtol=2e-3 if kernel == "rbf" else 5e-4)
    if kernel == "rbf":
        np.testing.assert_allclose(np.array(got)[:, 2], r[0, 2], rtol=2e-3)


def test_long_torch_reductions_are_flagged_and_refused():
    x = torch.rand(700000, device=DEV)
    with CaptureAudit() as a:
        x.mean()
        (x.view(700, 1000) * 2).sum(1)      # 1000 per output: short
        x.view(2, -1).sum(1)                 # 350 000 per output: long
    assert [f[0] for f in a.flagged] == ["mean", "sum"], a.flagged
    with pytest.raises(LongReductionInCapture):
        a.check("test")
    # the product's own long sums go through the package kernels: nothing to flag
    g = torch.randn(169343, 40, device=DEV)
    with CaptureAudit() as b:
        cs = ops.colsum(g)
    assert not b.flagged
    np.testing.assert_allclose(cs.cpu().double().numpy(), g.double().sum(0).cpu().numpy(), rtol=1e-5, atol=2e-3)


def test_structural_guard_refuses_a_memset_node_the_name_list_does_not_know(small, monkeypatch):
    """The default-on structural guard (_audit.check_captured_graph): with the operator-name audit switched off (EGNN_GRAPH_AUDIT=0) a
    step whose criterion ends in ATen's long ``kl_div(..., 'mean')`` -- the memset node of DESIGN.md 4.1 -- is still refused, at capture
    time, by what the captured graph CONTAINS; nothing is instantiated or replayed."""
    import efficient_gnns_amd.ops_edge as OE
    monkeypatch.setenv("EGNN_GRAPH_AUDIT", "0")
    data, d = small
    hp = dict(HP, beta=100.0)

    def torch_tail(feat, teacher_feat, edge_index, kern, criterion="kld"):
        plan = OE.edge_plan(edge_index, feat.shape[0])
        p_s = OE._SegSoftmax.apply(OE._EdgeSim.apply(feat, plan, kern), plan.ptr_b)
        p_t = OE._SegSoftmax.apply(OE._EdgeSim.apply(teacher_feat, plan, kern), plan.ptr_b)
        # (+ a 4 M-element sum: multi-block for certain, whatever ATen's heuristics make of the 68 k edges of this graph)
        return torch.nn.functional.kl_div(torch.log(p_s), p_t, log_target=False, reduction="mean") + 0.0 * big.sum()
    big = torch.ones(4_000_000, device=DEV)
    monkeypatch.setattr(OE, "lsp_loss", torch_tail)
    torch.manual_seed(0)
    m = PM.SAGE(data.num_features, 128, data.num_classes, 3, 0.5).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=0.01, fused=True, capturable=True)
    ei = subgraph(d.split_idx["train"], torch.stack(d.adj_t.coo()[:2]), relabel_nodes=True, num_nodes=data.num_nodes)[0]
    with pytest.warns(UserWarning, match="long torch reductions"), pytest.raises(LongReductionInCapture, match="memset"):
        PM.GraphedEpoch(m, d.x, d.adj_t, d.y, d.split_idx["train"], opt, "lpw", hp, d.teacher_out_feat, d.teacher_logits,
                        edge_index=ei, split_idx=d.split_idx, warmup=2)


@pytest.mark.parametrize("n,C", [(1, 7), (13, 40), (90941, 40), (169343, 256), (5000, 750), (33, 1024)])
def test_colsum_vs_float64(n, C):
    g = torch.Generator(device=DEV).manual_seed(n + C)
    x = torch.randn(n, C + 3, device=DEV, generator=g)[:, :C]          # a strided view: leading dimension C + 3
    out = ops.colsum(x)
    ref = x.double().sum(0)
    scale = float(x.abs().double().sum(0).max())
    assert float((out.double() - ref).abs().max()) <= 1e-6 * scale + 1e-12
    assert torch.equal(out, ops.colsum(x)), "fixed summation order"


def test_split_counts_equal_torch_counts():
    g = torch.Generator().manual_seed(5)
    n, C = 40011, 40
    logits = torch.randn(n, C, generator=g)
    y = torch.randint(0, C, (n, 1), generator=g)
    perm = torch.randperm(n, generator=g)
    split = {"train": perm[:20000], "valid": perm[20000:29000], "test": perm[29000:39000]}
    out = ops.split_accuracy(logits.to(DEV), y.to(DEV), {k: v.to(DEV) for k, v in split.items()}, counts=True).cpu()
    pred = logits.argmax(1, keepdim=True)
    want = [int((pred[split[k]] == y[split[k]]).sum()) for k in ("train", "valid", "test")] + [20000, 9000, 10000]
    assert out.tolist() == [float(v) for v in want]


def test_lsp_debug_invariants_hold_and_catch_a_broken_distribution(monkeypatch):
    """EGNN_DEBUG_CHECKS: every segment sums to 1 and the KL mean stays inside its bound."""
    data = D.arxiv_like(scale=0.02, seed=5)
    tr = data.split_idx["train"]
    ei = subgraph(tr, torch.stack(data.adj_t.coo()[:2]), relabel_nodes=True, num_nodes=data.num_nodes)[0].to(DEV)
    g = torch.Generator().manual_seed(1)
    f = torch.relu(torch.randn(tr.numel(), 64, generator=g)).to(DEV).requires_grad_(True)
    t = torch.relu(torch.randn(tr.numel(), 96, generator=g)).to(DEV)
    monkeypatch.setattr(ops_edge, "_DEBUG_CHECKS", True)
    loss = ops_edge.lsp_loss(f, t, ei, "cosine")
    assert 0 <= float(loss) < 11
    plan = ops_edge.edge_plan(ei, tr.numel())
    p = torch.full((plan.E,), 0.5, device=DEV)
    with pytest.raises(AssertionError):
        ops_edge._check_lsp_invariants(p, p, plan.ptr_b, loss, p, p, 0)


def test_dropin_accel_modules_match_torch():
    """dropin/accel.py: torch.nn.BatchNorm1d / torch.nn.Linear re-pointed at the package's kernels give torch's values, gradients and
    running statistics (fp32 tolerances of the package's parity tests); other inputs (3-D, CPU) keep torch's path; disable() restores."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_t", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    g = torch.Generator().manual_seed(0)
    n, C, P = 5000, 256, 64
    x0 = torch.randn(n, C, generator=g) * 2 + 0.5
    gy = torch.randn(n, P, generator=g)

    def run():
        torch.manual_seed(1)
        net = torch.nn.Sequential(torch.nn.BatchNorm1d(C), torch.nn.ReLU(), torch.nn.Linear(C, P)).to(DEV)
        x = x0.to(DEV).requires_grad_(True)
        y = net(x)
        y.backward(gy.to(DEV))
        net.eval()
        with torch.no_grad():
            ye = net(x0.to(DEV))
        return [y, x.grad, net[0].weight.grad, net[0].bias.grad, net[2].weight.grad, net[2].bias.grad, net[0].running_mean, net[0].running_var,
                net[0].num_batches_tracked.float(), ye]
    ref = run()
    orig_bn, orig_lin = torch.nn.BatchNorm1d.forward, torch.nn.Linear.forward
    accel.enable()
    try:
        assert accel.enabled() and torch.nn.BatchNorm1d.forward is not orig_bn
        got = run()
        bn3 = torch.nn.BatchNorm1d(4).to(DEV)
        assert bn3(torch.randn(2, 4, 5, device=DEV)).shape == (2, 4, 5)          # 3-D input: torch's own path
        # torch.optim.Adam over GPU parameters without an explicit choice -> the fused implementation, same update as torch's default
        lin_a, lin_b = torch.nn.Linear(16, 8).to(DEV), torch.nn.Linear(16, 8).to(DEV)
        lin_b.load_state_dict(lin_a.state_dict())
        opt_a = torch.optim.Adam([{"params": lin_a.parameters(), "lr": 0.01}])
        assert opt_a.defaults.get("fused") is True and len(opt_a.param_groups[0]["params"]) == 2
        opt_b = torch.optim.Adam([{"params": lin_b.parameters(), "lr": 0.01}], foreach=True)       # an explicit choice is respected
        assert not opt_b.defaults.get("fused")
        xx = torch.randn(32, 16, device=DEV)
        for _ in range(3):
            for lin, opt in ((lin_a, opt_a), (lin_b, opt_b)):
                opt.zero_grad()
                lin(xx).square().mean().backward()
                opt.step()
        assert float((lin_a.weight - lin_b.weight).abs().max()) <= 1e-6
        assert torch.nn.Linear(3, 2)(torch.randn(4, 3)).shape == (4, 2)         # CPU input: torch's own path
    finally:
        accel.disable()
    assert torch.nn.BatchNorm1d.forward is orig_bn and torch.nn.Linear.forward is orig_lin
    for a, b in zip(got, ref):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 2e-5 * scale + 1e-6, (a.shape, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("M,N,K,ta,tb,pad,split_k", [(5000, 256, 128, False, True, 0, None), (5000, 256, 256, False, False, 0, None),
                                                       (300, 72, 50, False, True, 3, None), (4096, 128, 64, False, False, 0, None),
                                                       (64, 40, 9000, True, False, 0, 8), (1000, 256, 96, False, True, 0, 1)])
def test_gemm_accumulating_store_vs_float64(M, N, K, ta, tb, pad, split_k):
    """egnn_gemm_add_f32: C = op(A) op(B) + bias + addend for the DMA form, the register-staged forms (odd pitches: narrow stores),
    split-K; the addend lives behind a pitch (a column block of a wider matrix)."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn((K, M) if ta else (M, K), generator=g)
    b = torch.randn((N, K) if tb else (K, N), generator=g) * 0.1
    bias = torch.randn(N, generator=g)
    add = torch.randn(M, N + pad, generator=g)[:, :N]
    ref = (a.double().t() if ta else a.double()) @ (b.double().t() if tb else b.double()) + bias.double() + add.double()
    out = ops.gemm_raw(a.to(DEV), b.to(DEV), ta, tb, bias.to(DEV), split_k=split_k, addend=add.to(DEV))
    scale = float(ref.abs().max())
    assert float((out.double().cpu() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (K / 256) ** 0.5)


@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("cin,cout", [(128, 256), (256, 256), (256, 40)])
def test_sage_layer_as_one_node_equals_the_composed_operators(reduce, cin, cout):
    """ops._SageLayer (accumulating stores, one autograd node) against lin_l(spmm(x)) + lin_r(x) built from the separate operators:
    output and all five gradients."""
    d = D.arxiv_like(scale=0.05, seed=9)
    adj = d.adj_t.to(DEV)
    g = torch.Generator().manual_seed(cin + cout)
    n = d.num_nodes
    x0 = torch.randn(n, cin, generator=g)
    lin_l, lin_r = torch.nn.Linear(cin, cout).to(DEV), torch.nn.Linear(cin, cout, bias=False).to(DEV)
    gy = torch.randn(n, cout, generator=g).to(DEV)

    def run(fused):
        for p in list(lin_l.parameters()) + list(lin_r.parameters()):
            p.grad = None
        x = x0.to(DEV).requires_grad_(True)
        if fused:
            out = ops.sage_layer(x, adj.set_value(None), lin_l, lin_r, reduce, narrow=cout < cin)
        else:
            out = ops.linear(ops.spmm(adj.set_value(None), x, reduce), lin_l.weight, lin_l.bias) + ops.linear(x, lin_r.weight, None)
        out.backward(gy)
        return [out.detach(), x.grad, lin_l.weight.grad.clone(), lin_l.bias.grad.clone(), lin_r.weight.grad.clone()]
    got, ref = run(True), run(False)
    for name, a, b in zip(("out", "dx", "dWl", "dbl", "dWr"), got, ref):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 3e-5 * scale, (name, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("kernel", ["cosine", "rbf"])
def test_edge_similarity_behind_a_padded_pitch(kernel):
    """egnn_edge_sim_f32 on rows of 750 columns behind a 752 pitch (the teacher features after ops.pad_pitch): the float4 walk
    + trailing columns equals the unpadded tensor's result (scalar walk) and float64."""
    g = torch.Generator().manual_seed(3)
    n, Dm, E_ = 3000, 750, 40000
    F_ = torch.relu(torch.randn(n, Dm, generator=g)) * (0.06 if kernel == "rbf" else 1.0)
    ei = torch.randint(0, n, (2, E_), generator=g)
    plan = ops_edge.EdgePlan(ei.to(DEV), n)
    dense = ops_edge._EdgeSim.apply(F_.to(DEV), plan, kernel)
    padded = ops_edge._EdgeSim.apply(ops.pad_pitch(F_.to(DEV)), plan, kernel)
    a, b = F_.double()[plan.a_in_b.cpu()], F_.double()[plan.b_in_b.cpu()]
    ref = torch.exp(-0.5 * ((a - b) ** 2).sum(1)) if kernel == "rbf" else torch.nn.functional.cosine_similarity(a, b)
    assert float((padded.double().cpu() - ref).abs().max()) <= 2e-6
    assert float((padded - dense).abs().max()) <= 1e-6


def test_grad_tap_does_not_edit_a_gradient_produced_for_another_tensor():
    """a gradient tagged "fresh" by a package backward that reaches the tap through a pass-through node (``tap(h) + c``
    fed to ops.matmul: AddBackward hands the SAME tensor to h and to c) must not be completed in place -- the sibling c would receive
    the projection head's rows as well.  The tag names the tap it was produced for (ops._fresh)."""
    gen = torch.Generator().manual_seed(4)
    n, C = 3000, 64
    h0 = torch.randn(n, C, generator=gen).to(DEV).requires_grad_()
    c0 = torch.randn(n, C, generator=gen).to(DEV).requires_grad_()
    W = torch.randn(C, 32, generator=gen).to(DEV)
    w2 = torch.randn(16, C, generator=gen).to(DEV)
    idx = torch.randperm(n, generator=gen)[:1000].to(DEV)
    gy = torch.randn(n, 32, generator=gen).to(DEV)
    h = ops.grad_tap(h0 * 1.0)
    z = ops.linear_rows(h, idx, w2)
    y = ops.matmul(h + c0, W)
    torch.autograd.backward([y, z], [gy, torch.ones_like(z)])
    dense = gy @ W.t()
    want_h = dense.clone()
    want_h[idx] += torch.ones(1000, 16, device=DEV) @ w2
    assert float((c0.grad - dense).abs().max()) <= 1e-4 * float(dense.abs().max()), "the sibling's gradient received the tap rows"
    assert float((h0.grad - want_h).abs().max()) <= 1e-4 * float(want_h.abs().max())
    # and the direct consumer still completes its own fresh gradient in place (no clone): same values
    h0.grad = None
    h = ops.grad_tap(h0 * 1.0)
    z = ops.linear_rows(h, idx, w2)
    y = ops.matmul(h, W)
    torch.autograd.backward([y, z], [gy, torch.ones_like(z)])
    assert float((h0.grad - want_h).abs().max()) <= 1e-4 * float(want_h.abs().max())


def test_locality_order_is_the_same_on_every_device():
    """dist.locality_order (every rank computes it for itself before the ranges are cut): the GPU result equals the CPU result --
    a rank-dependent order would shard different problems."""
    import efficient_gnns_amd.dist as DD
    d = D.arxiv_like(scale=0.05, seed=1, graph="local")
    perm_c, before_c, after_c = DD.locality_order(d, 8)
    perm_g, before_g, after_g = DD.locality_order(d, 8, device=torch.device(DEV))
    assert before_c == before_g and after_c == after_g
    assert perm_c is not None and torch.equal(perm_c, perm_g)
    assert sum(after_c) <= 0.7 * sum(before_c)     # (>= 40 % at 17 k nodes: tests/test_dist_gloo.py; this 8 k-node graph has 2 communities per range)


@pytest.mark.parametrize("gnn,mode", CASES + [("gcn", "supervised")])
def test_captured_epoch_graph_is_a_chain_of_kernel_nodes(small, gnn, mode):
    """The captured epoch read back through the HIP runtime (hipGraphGetNodes / NodeGetType / GetEdges, _audit.graph_node_kinds; since
    round 5 on EVERY capture, no switch): kernel nodes only, one chain -- no memset node (what ATen's multi-block reductions put
    there: DESIGN.md 4.1), no memcpy node."""
    data, d = small
    hp = dict(HP, beta=100.0 if mode in ("lpw", "gpw") else 0.1)
    torch.manual_seed(0)
    np.random.seed(0)
    m = (PM.GCN if gnn == "gcn" else PM.SAGE)(data.num_features, 128, data.num_classes, 3, 0.5).to(DEV)
    sp = tp = None
    params = list(m.parameters())
    if mode in ("nce", "gpw"):
        sp, tp = PM.make_projection(128, hp["proj_dim"]).to(DEV), PM.make_projection(750, hp["proj_dim"]).to(DEV)
        params += list(sp.parameters()) + list(tp.parameters())
    opt = torch.optim.Adam(params, lr=0.01, fused=True, capturable=True)
    ei = None
    if mode == "lpw":
        ei = subgraph(d.split_idx["train"], torch.stack(d.adj_t.coo()[:2]), relabel_nodes=True, num_nodes=data.num_nodes)[0]
    ge = PM.GraphedEpoch(m, d.x, d.adj_t, d.y, d.split_idx["train"], opt, mode, hp, d.teacher_out_feat, d.teacher_logits, sp, tp,
                         edge_index=ei, split_idx=d.split_idx, warmup=2)
    kinds = ge.node_kinds
    assert kinds is not None and kinds["chain"] and kinds.get("kernel", 0) > 50, kinds
    assert set(kinds) <= {"kernel", "edges", "chain"}, kinds
    losses, accs = ge.step()
    assert all(np.isfinite(v) for v in losses)


@pytest.mark.parametrize("mode", ["supervised", "kd"])
def test_compact_rows_route_equals_the_row_picks_inside_the_kernels(mode):
    """``models._TRAIN_ROWS`` off: ``model(...)[train_idx]`` is gathered and the criteria run on the compact rows.  Same losses and
    the same parameters after one step, bit for bit, as with the row picks inside the CE / KD kernels (the criteria's two forms are
    bit-equal, test_criteria_rows_twins_equal_the_compact_call, and everything behind the logits gradient is the same code); a
    caller's ``out=`` buffer receives the three losses on both routes."""
    d = to_dev(D.arxiv_like(scale=0.004, seed=2))
    tr = d.split_idx["train"]
    hp = dict(alpha=0.9, kd_T=4.0)
    torch.manual_seed(0)
    init = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.0).state_dict()
    runs = {}
    prev = PM._TRAIN_ROWS
    try:
        for flag in (True, False):
            PM._TRAIN_ROWS = flag
            model = PM.GCN(d.num_features, 64, d.num_classes, 3, 0.0).to(DEV)
            model.load_state_dict(init)
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            out = torch.zeros(3, device=DEV)
            ret = PM.train_step_tensors(model, d.x, d.adj_t, d.y, tr, opt, mode, hp, teacher_logits=d.teacher_logits, out=out)
            assert ret.data_ptr() == out.data_ptr() and ret.shape == (3,)
            loss, loss_cls, loss_aux = out.tolist()
            assert math.isfinite(loss) and loss_cls > 0
            if mode == "supervised":
                assert loss == loss_cls and loss_aux == 0
            else:
                assert loss_aux > 0 and loss == pytest.approx(loss_aux * (0.9 * 4.0 * 4.0) + loss_cls * (1 - 0.9), rel=1e-6)
            runs[flag] = (out.clone(), [p.detach().clone() for p in model.parameters()])
    finally:
        PM._TRAIN_ROWS = prev
    assert torch.equal(runs[True][0], runs[False][0]), (runs[True][0].tolist(), runs[False][0].tolist())
    for a, b in zip(runs[True][1], runs[False][1]):
        assert torch.equal(a, b)
