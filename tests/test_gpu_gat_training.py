"""Trainable GATConv on the gfx950 kernels (csrc/gat.hip backward): one-layer gradients against the oracle (fp32 and float64),
attention dropout against a float64 composite on the regenerated mask, bit-equal repeated backward passes, and the PPI GAT
student / teacher training steps (ppi_pyg/gnn.py:50-83,23-47,185-274) against the same steps on the oracle modules."""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import efficient_gnns_amd as E
import efficient_gnns_amd.data as D
import efficient_gnns_amd.models as PM
import oracle.criterion as OC
import oracle.models as OM
import oracle.nn as ON
import oracle.sparse as OS
from conftest import ROOT
from test_gpu_parity import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCRIPTS = os.path.join(ROOT, "tests", "dropin_scripts")
DROPIN = os.path.join(ROOT, "efficient-gnns_amd", "dropin")


def gat_graph(n=420, avg_deg=6, seed=0, self_loops=True):
    """edge_index (source, target) with duplicate edges, input self loops, isolated nodes (no in- or out-edges), one hub
    target with > 256 entries and one target with 65-256 entries."""
    g = torch.Generator().manual_seed(seed)
    live = n - 20                                                  # nodes live..n-1 stay isolated
    e = live * avg_deg
    src = torch.randint(0, live, (e,), generator=g)
    dst = torch.randint(0, live, (e,), generator=g)
    hub = torch.randint(0, live, (700,), generator=g)              # target 3: > 256 entries (> 256 distinct sources as well)
    mid = torch.randint(0, live, (120,), generator=g)              # target 5: 65-256 entries
    src = torch.cat([src, hub, mid, src[:40]])                     # duplicates of the first 40 edges
    dst = torch.cat([dst, torch.full((700,), 3), torch.full((120,), 5), dst[:40]])
    if self_loops:
        loops = torch.arange(0, live, 7)
        src, dst = torch.cat([src, loops]), torch.cat([dst, loops])
    return torch.stack([src, dst])


def layer_pair(F_in, H, C, concat, seed=1, **kw):
    torch.manual_seed(seed)
    oc = ON.GATConv(F_in, C, heads=H, concat=concat, **kw)
    with torch.no_grad():
        oc.bias.uniform_(-0.1, 0.1)
    pc = E.GATConv(F_in, C, heads=H, concat=concat, **kw).to(DEV)
    pc.load_state_dict(oc.state_dict())
    return oc.train(), pc.train()


GRADS = ("lin_l.weight", "att_l", "att_r", "bias")


def run_layer(conv, x, adj, w):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    out = conv(x, adj)
    (out * w).sum().backward()
    params = dict(conv.named_parameters())
    return out.detach(), x.grad, {k: params[k].grad for k in GRADS}


def check_layer(F_in, H, C, concat, sparse_input, add_self_loops=True, seed=0):
    n = 420
    ei = gat_graph(n, seed=seed, self_loops=add_self_loops)
    g = torch.Generator().manual_seed(seed + 11)
    x = torch.randn(n, F_in, generator=g)
    oc, pc = layer_pair(F_in, H, C, concat, add_self_loops=add_self_loops)
    w = torch.randn(n, H * C if concat else C, generator=g)
    adj_o = OS.to_sparse_tensor(ei, n) if sparse_input else ei
    adj_p = E.to_sparse_tensor(ei.to(DEV), n) if sparse_input else ei.to(DEV)
    out, gx, gp = run_layer(pc, x.to(DEV), adj_p, w.to(DEV))
    ref32 = run_layer(oc, x, adj_o, w)
    ref64 = run_layer(copy.deepcopy(oc).double(), x.double(), adj_o, w.double())
    close(out, ref32[0], rtol=1e-4, atol_scale=1e-4, msg="out vs fp32 oracle")
    close(out, ref64[0], rtol=1e-4, atol_scale=1e-4, msg="out vs float64 oracle")
    close(gx, ref64[1], rtol=1e-4, atol_scale=1e-4, msg="d x")
    for k in GRADS:
        close(gp[k], ref64[2][k], rtol=1e-4, atol_scale=1e-4, msg=f"d {k}")
    return pc


@pytest.mark.parametrize("sparse_input", [False, True], ids=["edge_index", "SparseTensor"])
@pytest.mark.parametrize("H,C,concat", [(4, 256, True), (6, 121, False), (2, 68, True), (2, 68, False), (1, 7, True), (3, 5, True),
                                        (3, 5, False), (2, 8, False)])   # averaged heads at the smallest scalar / float4 shapes
def test_gatconv_gradients_match_oracle(H, C, concat, sparse_input):
    pc = check_layer(24, H, C, concat, sparse_input)
    adj = pc._structure(gat_graph(420).to(DEV) if not sparse_input else E.to_sparse_tensor(gat_graph(420).to(DEV), 420), 420)
    deg = (adj.csr()[0][1:] - adj.csr()[0][:-1]).cpu()
    assert deg.max() > 256 and ((deg > 64) & (deg <= 256)).any() and (deg == 1).any()   # hub, mid row, isolated (self loop only)


@pytest.mark.parametrize("sparse_input", [False, True], ids=["edge_index", "SparseTensor"])
def test_gatconv_gradients_without_self_loops_and_empty_rows(sparse_input):
    pc = check_layer(24, 2, 68, True, sparse_input, add_self_loops=False, seed=3)
    ei = gat_graph(420, seed=3, self_loops=False).to(DEV)
    adj = pc._structure(ei if not sparse_input else E.to_sparse_tensor(ei, 420), 420)
    rp = adj.csr()[0]
    assert bool(((rp[1:] - rp[:-1]) == 0).any())                  # empty target rows


def _composite64(x, W, att_l, att_r, bias, rowptr, col, mult, H, C, concat, slope):
    """GATConv on the CSR entries in float64 with torch autograd: the float64 bar for the dropout backward."""
    n = x.shape[0]
    row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    xl = (x @ W.t()).view(n, H, C)
    a_src, a_dst = (xl * att_l).sum(-1), (xl * att_r).sum(-1)
    s = F.leaky_relu(a_src[col] + a_dst[row], slope)                                     # [E, H]
    m = torch.full((n, H), -float("inf"), dtype=s.dtype).scatter_reduce(0, row[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[row])
    z = torch.zeros(n, H, dtype=s.dtype).index_add(0, row, ex)
    att = ex / (z[row] + 1e-16) * mult.t()
    out = torch.zeros(n, H, C, dtype=s.dtype).index_add(0, row, xl[col] * att[..., None])
    out = out.reshape(n, H * C) if concat else out.mean(1)
    return out + bias


@pytest.mark.parametrize("H,C,concat", [(2, 68, True), (6, 121, False)])
def test_gatconv_attention_dropout_gradients_on_the_regenerated_mask(H, C, concat):
    n, F_in, p = 420, 24, 0.5
    ei = gat_graph(n, seed=5).to(DEV)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n, F_in, generator=g)
    w = torch.randn(n, H * C if concat else C, generator=g)
    _, pc = layer_pair(F_in, H, C, concat, dropout=p)
    torch.manual_seed(123)
    out, gx, gp = run_layer(pc, x.to(DEV), ei, w.to(DEV))
    adj = pc._structure(ei, n)
    torch.manual_seed(123)                                         # the layer's one [H, nnz] draw
    mult = ((torch.rand(H, adj.nnz(), device=DEV) >= p).double() / (1 - p)).cpu()
    assert 0.4 < float((mult > 0).double().mean()) < 0.6
    rowptr, col, _ = adj.csr()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in pc.named_parameters()}
    xr = x.double().requires_grad_(True)
    ref = _composite64(xr, params["lin_l.weight"], params["att_l"], params["att_r"], params["bias"], rowptr.cpu(), col.cpu(), mult,
                       H, C, concat, pc.negative_slope)
    (ref * w.double()).sum().backward()
    close(out, ref, rtol=1e-4, atol_scale=1e-4, msg="out")
    close(gx, xr.grad, rtol=1e-4, atol_scale=1e-4, msg="d x")
    for k in GRADS:
        close(gp[k], params[k].grad, rtol=1e-4, atol_scale=1e-4, msg=f"d {k}")


def test_gatconv_backward_is_deterministic():
    n = 420
    ei = gat_graph(n, seed=7).to(DEV)
    for H, C, concat in ((4, 256, True), (6, 121, False)):         # concatenated heads, and averaged heads on the scalar path
        g = torch.Generator().manual_seed(8)
        x, w = torch.randn(n, 64, generator=g).to(DEV), torch.randn(n, H * C if concat else C, generator=g).to(DEV)
        _, pc = layer_pair(64, H, C, concat)
        a = run_layer(pc, x, ei, w)
        b = run_layer(pc, x, ei, w)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for k in GRADS:
            assert torch.equal(a[2][k], b[2][k]), (H, C, concat, k)


def test_gatconv_eval_mode_still_refuses_gradients():
    _, pc = layer_pair(16, 2, 8, True)
    pc.eval()
    with pytest.raises(NotImplementedError):
        pc(torch.randn(30, 16, device=DEV), gat_graph(30, avg_deg=2).clamp(max=29).to(DEV))


# ------------------------------------------------------------------------------------------------
# PPI models: training steps against the oracle
# ------------------------------------------------------------------------------------------------
def _gpu_graphs(graphs):
    return [types.SimpleNamespace(x=g.x.to(DEV), edge_index=g.edge_index.to(DEV), y=g.y.to(DEV)) for g in graphs]


def _student_pair(seed=0):
    torch.manual_seed(seed)
    om = OM.GAT(50, 68, 121, 5, 0.0, heads=2)                      # the same layers as StudentNet (ppi_pyg/gnn.py:50-83)
    pm = PM.StudentNet(50, 121).to(DEV)
    sd = {}
    for k, v in om.state_dict().items():
        kind, idx, rest = k.split(".", 2)
        sd[f"{'conv' if kind == 'convs' else 'lin'}{int(idx) + 1}.{rest}"] = v
    pm.load_state_dict(sd)
    return om, pm


def test_ppi_student_net_supervised_steps_vs_oracle():
    train, _, _ = D.ppi_like(seed=4, n_train=3, total_train_nodes=3000)
    om, pm = _student_pair()
    oo, po = torch.optim.Adam(om.parameters(), lr=0.005), torch.optim.Adam(pm.parameters(), lr=0.005)
    for g, pg in zip(train, _gpu_graphs(train)):
        ref = OM.ppi_train_epoch(om, None, [g], oo, "supervised", {})
        got = PM.ppi_train_epoch(pm, None, [pg], po, "supervised", {})
        for a, b in zip(got, ref):
            close(a, b, rtol=2e-4, atol_scale=0)


def test_ppi_teacher_net_supervised_step_vs_oracle():
    train, _, _ = D.ppi_like(seed=5, n_train=1, total_train_nodes=1500)
    torch.manual_seed(0)
    ot = OM.TeacherNet(50, 121)
    pt = PM.TeacherNet(50, 121).to(DEV)
    pt.load_state_dict(ot.state_dict())
    oo, po = torch.optim.Adam(ot.parameters(), lr=0.005), torch.optim.Adam(pt.parameters(), lr=0.005)
    ref = OM.ppi_train_epoch(ot, None, train, oo, "supervised", {})
    got = PM.ppi_train_epoch(pt, None, _gpu_graphs(train), po, "supervised", {})
    for a, b in zip(got, ref):
        close(a, b, rtol=2e-4, atol_scale=0)


def _oracle_nce_step(om, ot, g, opt, sp, tp, hp):
    om.train(); sp.train(); tp.train(); ot.eval()
    out = om(g.x, g.edge_index)
    with torch.no_grad():
        ot(g.x, g.edge_index)
        t_feat = ot.out_feat
    loss, lc, la = OC.ppi_nce_criterion(out, g.y, sp(om.out_feat), tp(t_feat), hp["beta"], hp["nce_T"], hp["max_samples"])
    opt.zero_grad(); loss.backward(); opt.step()
    return loss.item(), lc.item(), la.item()


@pytest.mark.parametrize("mode", ["kd", "nce"])
def test_ppi_gat_student_distillation_step_with_frozen_teacher(mode):
    train, _, _ = D.ppi_like(seed=6, n_train=1, total_train_nodes=1400)
    hp = dict(alpha=0.5, kd_T=1.0, beta=0.5, nce_T=0.075, max_samples=8192)
    om, pm = _student_pair(seed=1)
    torch.manual_seed(2)
    ot = OM.TeacherNet(50, 121)
    pt = PM.TeacherNet(50, 121).to(DEV)
    pt.load_state_dict(ot.state_dict())
    if mode == "kd":
        oo, po = torch.optim.Adam(om.parameters(), lr=0.005), torch.optim.Adam(pm.parameters(), lr=0.005)
        ref = OM.ppi_train_epoch(om, ot, train, oo, "kd", hp)
        got = PM.ppi_train_epoch(pm, pt, _gpu_graphs(train), po, "kd", hp)
    else:
        torch.manual_seed(3)
        osp, otp = OM.make_projection(136, 64), OM.make_projection(1024, 64)
        psp, ptp = PM.make_projection(136, 64).to(DEV), PM.make_projection(1024, 64).to(DEV)
        psp.load_state_dict(osp.state_dict()); ptp.load_state_dict(otp.state_dict())

        def adam(m, a, b):
            return torch.optim.Adam([{"params": m.parameters(), "lr": 0.005}, {"params": a.parameters(), "lr": 0.005},
                                     {"params": b.parameters(), "lr": 0.005}])
        ref = _oracle_nce_step(om, ot, train[0], adam(om, osp, otp), osp, otp, hp)
        got = PM.ppi_train_epoch(pm, pt, _gpu_graphs(train), adam(pm, psp, ptp), "nce", hp, psp, ptp)
    for a, b in zip(got, ref):
        close(a, b, rtol=2e-4, atol_scale=0)


def _oracle_aux_step(mode, om, ot, g, opt, sp, tp, hp):
    """``_oracle_nce_step`` for the other feature criteria: ``fitnet`` through the projection heads, ``at`` / ``gpw`` / ``lpw`` on the
    hidden features themselves (ppi_pyg/gnn.py:213-262)."""
    om.train(); ot.eval()
    out = om(g.x, g.edge_index)
    with torch.no_grad():
        ot(g.x, g.edge_index)
        t_feat = ot.out_feat
    if mode == "fitnet":
        sp.train(); tp.train()
        loss, lc, la = OC.ppi_fitnet_criterion(out, g.y, sp(om.out_feat), tp(t_feat), hp["beta"])
    elif mode == "at":
        loss, lc, la = OC.ppi_at_criterion(out, g.y, om.out_feat, t_feat, hp["beta"])
    elif mode == "gpw":
        loss, lc, la = OC.ppi_gpw_criterion(out, g.y, om.out_feat, t_feat, hp["kernel"], hp["beta"], hp["max_samples"])
    else:
        loss, lc, la = OC.ppi_lpw_criterion(out, g.y, om.out_feat, t_feat, g.edge_index, hp["kernel"], hp["beta"])
    opt.zero_grad(); loss.backward(); opt.step()
    return loss.item(), lc.item(), la.item()


@pytest.mark.parametrize("mode,kernel", [("fitnet", None), ("at", None), ("gpw", "rbf"), ("lpw", "cosine")])
def test_ppi_gat_student_feature_distillation_step_with_frozen_teacher(mode, kernel):
    """The ``fitnet`` / ``at`` / ``gpw`` / ``lpw`` rungs of ``ppi_train_epoch``: one step against the oracle's ``ppi_*_criterion``."""
    train, _, _ = D.ppi_like(seed=6, n_train=1, total_train_nodes=1400)
    hp = dict(alpha=0.5, kd_T=1.0, beta=0.5, nce_T=0.075, max_samples=8192, kernel=kernel)   # max_samples > n: no draw
    om, pm = _student_pair(seed=1)
    torch.manual_seed(2)
    ot = OM.TeacherNet(50, 121)
    pt = PM.TeacherNet(50, 121).to(DEV)
    pt.load_state_dict(ot.state_dict())
    torch.manual_seed(3)
    osp, otp = OM.make_projection(136, 64), OM.make_projection(1024, 64)
    psp, ptp = PM.make_projection(136, 64).to(DEV), PM.make_projection(1024, 64).to(DEV)
    psp.load_state_dict(osp.state_dict()); ptp.load_state_dict(otp.state_dict())
    assert train[0].x.shape[0] < hp["max_samples"]

    def adam(m, a, b):
        return torch.optim.Adam([{"params": m.parameters(), "lr": 0.005}, {"params": a.parameters(), "lr": 0.005},
                                 {"params": b.parameters(), "lr": 0.005}])
    ref = _oracle_aux_step(mode, om, ot, train[0], adam(om, osp, otp), osp, otp, hp)
    got = PM.ppi_train_epoch(pm, pt, _gpu_graphs(train), adam(pm, psp, ptp), mode, hp, psp, ptp)
    print(f"ppi {mode}: got {got} oracle {ref}")
    assert ref[2] > 0
    for a, b in zip(got, ref):
        close(a, b, rtol=2e-4, atol_scale=0)


# ------------------------------------------------------------------------------------------------
# drop-in: a PyG-API training loop through the torch_geometric.nn shim, and the same loop on the oracle
# ------------------------------------------------------------------------------------------------
def _load_script(gatconv=None):
    """tests/dropin_scripts/ppi_gat_train.py with torch_geometric.nn from the drop-in shim (``gatconv=None``) or a module whose
    GATConv is ``gatconv``."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "torch_geometric" or k.startswith("torch_geometric.")}
    path_before = list(sys.path)
    try:
        if gatconv is None:
            sys.path.insert(0, DROPIN)
        else:
            pkg, nnm = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.nn")
            nnm.GATConv, pkg.nn = gatconv, nnm
            sys.modules["torch_geometric"], sys.modules["torch_geometric.nn"] = pkg, nnm
        spec = importlib.util.spec_from_file_location("ppi_gat_train_" + ("shim" if gatconv is None else "oracle"),
                                                      os.path.join(SCRIPTS, "ppi_gat_train.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if gatconv is None:
            assert mod.GATConv is E.GATConv
        return mod
    finally:
        sys.path[:] = path_before
        for k in [k for k in sys.modules if k == "torch_geometric" or k.startswith("torch_geometric.")]:
            sys.modules.pop(k)
        sys.modules.update(saved)


def test_dropin_ppi_gat_training_loop_vs_oracle():
    shim, orc = _load_script(), _load_script(ON.GATConv)
    train, _, _ = D.ppi_like(seed=7, n_train=2, total_train_nodes=2400)
    torch.manual_seed(0)
    om = orc.StudentNet(50, 121)
    pm = shim.StudentNet(50, 121).to(DEV)
    pm.load_state_dict(om.state_dict())
    ref = orc.train(om, train, torch.optim.Adam(om.parameters(), lr=0.005), "cpu")
    got = shim.train(pm, train, torch.optim.Adam(pm.parameters(), lr=0.005), DEV)
    assert len(got) == len(ref) == 2
    close(np.array(got), np.array(ref), rtol=2e-4, atol_scale=0)
