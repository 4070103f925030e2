"""A PyG training script runs unchanged on top of ``efficient-gnns_amd/dropin``: ``tests/dropin_scripts/arxiv_train.py``
(GCN / SAGE classes, ``train()`` / ``test()``) and ``arxiv_train_kd_and_aux.py`` (loss = KD + beta * aux), written against the
PyG / torch-sparse API in the shape of the reference's arxiv training scripts, import ``torch_geometric`` / ``torch_sparse`` /
``criterion`` from the drop-in layer and are checked against the package's own ``train_step`` / ``evaluate`` (GPU) and the
oracle (CPU host layer)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

SCRIPTS = os.path.join(ROOT, "tests", "dropin_scripts")
REF = os.path.join(SCRIPTS, "arxiv_train.py")
REF_KD_AUX = os.path.join(SCRIPTS, "arxiv_train_kd_and_aux.py")
DROPIN = os.path.join(ROOT, "efficient-gnns_amd", "dropin")
_SCRIPT_MODULES = ("arxiv_train",)
_SHIMMED = ("criterion", "torch_geometric", "torch_geometric.nn", "torch_geometric.utils", "torch_geometric.transforms", "torch_sparse")


def _load_accel():
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_ref", os.path.join(DROPIN, "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)
    return accel


def _load_reference_gnn(path=None):
    for name in ("ogb", "ogb.nodeproppred", "torch.utils.tensorboard", "logger"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["ogb.nodeproppred"].PygNodePropPredDataset = None
    sys.modules["ogb.nodeproppred"].Evaluator = object
    sys.modules["torch.utils.tensorboard"].SummaryWriter = object
    sys.modules["logger"].Logger = object
    sys.path.insert(0, DROPIN)
    if SCRIPTS not in sys.path:
        sys.path.insert(0, SCRIPTS)      # (the kd-and-aux script imports its models from arxiv_train.py)
    for stale in _SHIMMED + _SCRIPT_MODULES:
        sys.modules.pop(stale, None)
    spec = importlib.util.spec_from_file_location("ref_gnn_dropin", path or REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dropin_names_resolve_on_cpu():
    """Import-level drop-in check (no GPU needed): every name the reference imports resolves to the new package."""
    sys.path.insert(0, DROPIN)
    try:
        for stale in _SHIMMED:
            sys.modules.pop(stale, None)
        import criterion as C
        import torch_geometric.transforms as T
        from torch_geometric.nn import GCNConv, SAGEConv
        from torch_geometric.utils import softmax, subgraph, to_dense_adj, negative_sampling, add_self_loops  # noqa: F401
        from torch_sparse import SparseTensor
        import efficient_gnns_amd as E
        assert GCNConv is E.GCNConv and SAGEConv is E.SAGEConv and SparseTensor is E.SparseTensor
        assert T.ToSparseTensor is E.ToSparseTensor
        for fn in ("kd_criterion", "fitnet_criterion", "at_criterion", "gpw_criterion", "lpw_criterion", "nce_criterion"):
            assert callable(getattr(C, fn))
        import inspect
        assert str(inspect.signature(C.nce_criterion)) == "(logits, labels, feat, teacher_feat, beta=0.5, nce_T=0.075, max_samples=8192)"
        assert str(inspect.signature(C.kd_criterion)) == "(logits, labels, teacher_logits, alpha=0.9, T=4)"
        assert str(inspect.signature(C.lpw_criterion)) == "(logits, labels, feat, teacher_feat, edge_index, kernel='cosine', beta=100, criterion='kld')"
        assert str(inspect.signature(C.gpw_criterion)) == "(logits, labels, feat, teacher_feat, kernel='cosine', beta=1, max_samples=8192)"
        assert str(inspect.signature(C.fitnet_criterion)) == "(logits, labels, feat, teacher_feat, beta=1000)"
        assert str(inspect.signature(C.at_criterion)) == "(logits, labels, feat, teacher_feat, beta=1000)"
    finally:
        sys.path.remove(DROPIN)
        for stale in _SHIMMED:
            sys.modules.pop(stale, None)


class _Evaluator:
    def eval(self, dd):
        return {"acc": float((dd["y_true"].cpu().numpy() == dd["y_pred"].cpu().numpy()).mean())}


@pytest.mark.gpu
@pytest.mark.parametrize("gnn", ["gcn", "sage"])
@pytest.mark.parametrize("mode", ["nce", "kd", "lpw", "gpw"])
@pytest.mark.parametrize("script,accel_mode", [("gnn", "plain"), ("gnn", "lazy"), ("gnn", "eager"), ("kd_and_aux", "plain"), ("kd_and_aux", "lazy")])
def test_reference_train_loop_runs_unchanged_on_the_new_operators(gnn, mode, script, accel_mode):
    """The script's GCN / SAGE classes, train() and test() (tests/dropin_scripts/arxiv_train.py), imported unchanged
    through efficient-gnns_amd/dropin and executed on the GPU kernels: three optimisation steps and the eval logits equal
    the package's own train_step / evaluate from the same initial weights and the same NumPy draw (dropout 0: the
    reference's F.dropout and the fused kernel's mask are equal only in distribution).
    ``script`` = kd_and_aux: arxiv_train_kd_and_aux.py's train() (loss = KD + beta * aux) against
    ``train_step(kd_and_aux=True)``.  ``accel_mode``: plain = torch's own BatchNorm1d / Linear (launch.py --plain-torch-modules);
    eager = dropin/accel.py with one launch per torch call; lazy = accel's default: BatchNorm1d.forward returns a deferred activation
    that absorbs F.relu / F.dropout and is formed by its consumer (efficient_gnns_amd/lazy.py)."""
    path = REF if script == "gnn" else REF_KD_AUX
    if script == "kd_and_aux" and mode == "kd":
        pytest.skip("the kd-and-aux script's kd branch is arxiv_train.py's")
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.models as PM
    from efficient_gnns_amd.utils import subgraph
    ref = _load_reference_gnn(path)
    accel = None
    if accel_mode != "plain":
        accel = _load_accel()
        accel.LAZY = accel_mode == "lazy"
        accel._BIG_GATHER = accel._MIN_GATHER_ROWS = 1       # (this 3 387-node problem: let the script's deferred constant teacher gather take part)
        accel.enable()
    try:
        dev = torch.device("cuda")
        d = D.arxiv_like(scale=0.02, seed=2)
        data = types.SimpleNamespace(x=d.x.to(dev), y=d.y.to(dev), adj_t=d.adj_t.to(dev))
        split_idx = {k: v.to(dev) for k, v in d.split_idx.items()}
        train_idx = split_idx["train"]
        H, Pj, S = 64, 32, 256
        hp = dict(alpha=0.9, kd_T=4.0, beta={"nce": 0.1, "kd": 0.0, "lpw": 100.0, "gpw": 100.0}[mode], nce_T=0.075, max_samples=S,
                  kernel="rbf" if mode == "lpw" else "cosine", proj_dim=Pj)
        args = argparse.Namespace(training=mode, **{k: hp[k] for k in ("alpha", "kd_T", "beta", "nce_T", "max_samples", "kernel")})
        torch.manual_seed(0)
        model = (ref.GCN if gnn == "gcn" else ref.SAGE)(d.num_features, H, d.num_classes, 3, 0.0).to(dev)
        # projection heads as a PyG script builds them: Linear + BatchNorm1d + ReLU
        sp = torch.nn.Sequential(torch.nn.Linear(H, Pj), torch.nn.BatchNorm1d(Pj), torch.nn.ReLU()).to(dev)
        tp = torch.nn.Sequential(torch.nn.Linear(750, Pj), torch.nn.BatchNorm1d(Pj), torch.nn.ReLU()).to(dev)
        mine = (PM.GCN if gnn == "gcn" else PM.SAGE)(d.num_features, H, d.num_classes, 3, 0.0).to(dev)
        msp, mtp = PM.make_projection(H, Pj).to(dev), PM.make_projection(750, Pj).to(dev)
        mine.load_state_dict(model.state_dict())
        msp.load_state_dict(sp.state_dict())
        mtp.load_state_dict(tp.state_dict())

        def adam(m, a, b):
            return torch.optim.Adam([{"params": m.parameters()}, {"params": a.parameters()}, {"params": b.parameters()}], lr=0.01)
        tf, tl = d.teacher_out_feat.to(dev), d.teacher_logits.to(dev)
        edge_index = None
        if mode == "lpw":   # the train-induced subgraph
            edge_index = subgraph(train_idx, torch.stack(data.adj_t.coo()[:2]), relabel_nodes=True, num_nodes=d.num_nodes)[0]
        out0, accs0 = ref.test(model, data, split_idx, _Evaluator())
        mout0, maccs0 = PM.evaluate(mine, data.x, data.adj_t, data.y, split_idx)
        np.testing.assert_allclose(out0.cpu().numpy(), mout0.cpu().numpy(), rtol=1e-5, atol=1e-5 * float(mout0.abs().max()))
        np.testing.assert_allclose(list(accs0), list(maccs0), atol=1e-6)
        opt, mopt = adam(model, sp, tp), adam(mine, msp, mtp)
        np.random.seed(3)
        got = [ref.train(model, data, train_idx, opt, args, tf, tl, sp, tp, edge_index) for _ in range(3)]
        np.random.seed(3)
        if accel is not None:
            accel.disable()          # the package's own loop below never goes through the re-pointed torch modules; make that certain
        want = [PM.train_step(mine, data.x, data.adj_t, data.y, train_idx, mopt, mode, hp, tf, tl, msp, mtp, edge_index, kd_and_aux=script == "kd_and_aux")
                for _ in range(3)]
        if accel is not None:
            accel.enable()
        # step 1: same weights, same draw -> the kernels' rounding only.  Steps 2-3 are a trajectory: Adam's g / sqrt(v) turns rounding
        # differences of small gradients into O(lr) weight differences, and GSP at beta = 100 multiplies what the loss sees of them
        # (the two sides differ in association order only: fused heads / SAGE's output layer aggregating lin_l(x))
        np.testing.assert_allclose(np.array(got[0]), np.array(want[0]), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(np.array(got), np.array(want), rtol=1e-3 if mode == "gpw" else 2e-4, atol=1e-6)
        assert all(np.isfinite(v) for step in got for v in step)
        out, accs = ref.test(model, data, split_idx, _Evaluator())
        assert out.shape == (d.num_nodes, d.num_classes) and all(0 <= a <= 1 for a in accs)
        if accel_mode == "lazy":     # the deferred form is what ran: out_feat of the script's model is the deferred object, formed by now
            from efficient_gnns_amd.lazy import LazyBnAct, LazyFold, LazyRows
            # the script's `teacher_out_feat[train_idx]`: a row gather of a large constant leaf inside a grad-enabled region is deferred ...
            picked = tf[train_idx]
            assert isinstance(picked, LazyRows) and picked._const and torch.equal(picked._egnn_materialise(), torch.Tensor.index_select(tf, 0, train_idx))
            with torch.no_grad():                          # ... and nothing else is: no_grad regions, tensors in autograd, other index kinds
                assert isinstance(tf[train_idx], torch.Tensor) and isinstance(tf[:5], torch.Tensor) and isinstance(tf[train_idx[0]], torch.Tensor)
            assert isinstance(tf.clone().requires_grad_(True)[train_idx], torch.Tensor)
            assert isinstance(model.out_feat, (LazyBnAct, LazyFold)) and model.out_feat._value is not None
            if gnn == "gcn":
                # inference: the convs have been seen feeding their BatchNorms, so test() ran conv + BN + ReLU as ONE pass (the BatchNorm
                # folded into the conv's weights, lazy.LazyFold); same logits as one launch per torch call
                assert isinstance(model.out_feat, LazyFold) and model.out_feat._relu
                accel.LAZY = False
                out_eager, accs_eager = ref.test(model, data, split_idx, _Evaluator())
                accel.LAZY = True
                np.testing.assert_allclose(out.cpu().numpy(), out_eager.cpu().numpy(), rtol=1e-5, atol=1e-5 * float(out_eager.abs().max()))
                np.testing.assert_allclose(list(accs), list(accs_eager), atol=2.0 / min(int(v.numel()) for v in split_idx.values()))
    finally:
        if accel is not None:
            accel.disable()
        if DROPIN in sys.path:
            sys.path.remove(DROPIN)
        if SCRIPTS in sys.path:
            sys.path.remove(SCRIPTS)
        for stale in _SHIMMED + _SCRIPT_MODULES + ("ref_gnn_dropin",):
            sys.modules.pop(stale, None)


# ------------------------------------------------------------------------------------------------
# CPU variant: the reference's own train()/test() on top of the drop-in HOST layer, kernels replaced by oracle stand-ins
# ------------------------------------------------------------------------------------------------
def _host_layer_worker(q, gnn, mode):
    """Runs in a spawned process: the ops monkeypatches must not leak into the other tests of this session."""
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    import efficient_gnns_amd as E
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.nn as PN
    import efficient_gnns_amd.ops as ops
    import oracle.sparse as OS

    def to_oracle(adj):
        rowptr, col, val = adj.csr()
        return OS.SparseTensor(rowptr=rowptr, col=col, value=val, sparse_sizes=adj.sparse_sizes())

    def gcn_norm(adj):
        g = OS.gcn_norm_sparse(to_oracle(adj))
        return E.SparseTensor(rowptr=g.csr()[0], col=g.csr()[1], value=g.csr()[2], sparse_sizes=g.sparse_sizes())
    PN.gcn_norm = gcn_norm
    ops.spmm = lambda adj, x, reduce="sum", bias=None, addend=None, **_: (OS.matmul(to_oracle(adj), x, reduce) + (0 if bias is None else bias)
                                                                            + (0 if addend is None else addend))
    ops.matmul = lambda x, w, bias=None: x @ w if bias is None else x @ w + bias
    ops.linear = lambda x, w, b=None: F.linear(x, w, b)
    ops.take_rows = lambda x, idx: x[idx]
    ops.cross_entropy = lambda logits, labels, rows=None: F.cross_entropy(logits, labels)
    ops.gather_normalize = lambda x, idx=None, eps=1e-12: F.normalize(x if idx is None else x[idx], p=2, dim=-1)
    ops.nce_unit = lambda f, t, tau: F.cross_entropy(f @ t.t() / tau, torch.arange(f.shape[0]))
    ops.ce_and_kd = lambda logits, labels, teacher, T, rows=None: (
        F.cross_entropy(logits, labels), F.kl_div(F.log_softmax(logits / T, dim=1), F.softmax(teacher / T, dim=1), log_target=False))

    ref = _load_reference_gnn()
    d = D.arxiv_like(scale=0.004, seed=2)
    data = types.SimpleNamespace(x=d.x, y=d.y, adj_t=d.adj_t)
    torch.manual_seed(0)
    np.random.seed(0)
    model = (ref.GCN if gnn == "gcn" else ref.SAGE)(d.num_features, 32, d.num_classes, 3, 0.0)
    sp = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.BatchNorm1d(16), torch.nn.ReLU())
    tp = torch.nn.Sequential(torch.nn.Linear(750, 16), torch.nn.BatchNorm1d(16), torch.nn.ReLU())
    init = {k: v.clone() for m, pre in ((model, "m."), (sp, "s."), (tp, "t.")) for k, v in ((pre + kk, vv) for kk, vv in m.state_dict().items())}
    opt = torch.optim.Adam([{"params": model.parameters()}, {"params": sp.parameters()}, {"params": tp.parameters()}], lr=0.01)
    args = argparse.Namespace(training=mode, alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=96, kernel="rbf")

    class Ev:
        def eval(self, dd):
            return {"acc": float((dd["y_true"].cpu().numpy() == dd["y_pred"].cpu().numpy()).mean())}
    out0, accs0 = ref.test(model, data, d.split_idx, Ev())
    losses = [ref.train(model, data, d.split_idx["train"], opt, args, d.teacher_out_feat, d.teacher_logits, sp, tp, None) for _ in range(3)]
    q.put((losses, out0.numpy(), list(accs0), {k: v.numpy() for k, v in init.items()}))


@pytest.mark.parametrize("gnn,mode", [("gcn", "nce"), ("sage", "kd"), ("sage", "nce"), ("gcn", "supervised")])
def test_reference_train_loop_drives_the_host_layer_on_cpu(gnn, mode):
    """The script's GCN / SAGE / train() / test(), imported unchanged through efficient-gnns_amd/dropin, running on the
    package's host layer (GCNConv, SparseTensor, criterion) with the kernels swapped for oracle stand-ins in a child
    process: the losses of three steps and the initial eval equal the oracle's train_step / evaluate."""
    import torch.multiprocessing as mp
    import efficient_gnns_amd.data as D
    import oracle.models as OM
    import oracle.sparse as OS
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    p = ctx.Process(target=_host_layer_worker, args=(q, gnn, mode))
    p.start()
    import time
    t0 = time.time()
    while q.empty():   # a child that died (e.g. a stand-in out of date with the host layer) must fail the test, not hang it
        assert p.is_alive() or not q.empty(), f"worker exited with {p.exitcode} before reporting"
        assert time.time() - t0 < 600, "worker timed out"
        time.sleep(0.2)
    losses, out0, accs0, init = q.get()
    p.join(300)
    assert p.exitcode == 0
    d = D.arxiv_like(scale=0.004, seed=2)
    rowptr, col, _ = d.adj_t.csr()
    oadj = OS.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=d.adj_t.sparse_sizes())
    om = (OM.GCN if gnn == "gcn" else OM.SAGE)(d.num_features, 32, d.num_classes, 3, 0.0)
    osp, otp = OM.make_projection(32, 16), OM.make_projection(750, 16)
    for m, pre in ((om, "m."), (osp, "s."), (otp, "t.")):
        m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in init.items() if k.startswith(pre)})
    np.random.seed(0)   # the child seeded NumPy before building its modules; the draws of the three steps follow
    oopt = torch.optim.Adam([{"params": om.parameters()}, {"params": osp.parameters()}, {"params": otp.parameters()}], lr=0.01)
    hp = dict(alpha=0.9, kd_T=4.0, beta=0.1, nce_T=0.075, max_samples=96, kernel="rbf")
    ref_out0, ref_accs0 = OM.evaluate(om, d.x, oadj, d.y, d.split_idx)
    ref_losses = [OM.train_step(om, d.x, oadj, d.y, d.split_idx["train"], oopt, mode, hp, d.teacher_out_feat, d.teacher_logits, osp, otp)
                  for _ in range(3)]
    np.testing.assert_allclose(out0, ref_out0.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(accs0, list(ref_accs0), atol=1e-9)
    np.testing.assert_allclose(np.array(losses), np.array(ref_losses), rtol=1e-5, atol=1e-7)
