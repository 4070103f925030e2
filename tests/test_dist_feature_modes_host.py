"""gloo (CPU) coverage of the fitnet / at / gcd modes of the node-range sharded step (efficient-gnns_amd/dist.py).

The machinery is tests/test_dist_gloo.py's (oracle-backed stand-ins for the ``ops`` entry points, the ~680-node graph, the quiet exit);
on top of it the three split attention-transfer operators and ``ops.fitnet_loss`` are restated in torch, and this file has its own
worker / reference run, which build the projection heads each mode needs.  The reference is ``oracle.models.train_step``.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_dist_gloo import HP, _free_port, _make_data, _patch_ops_with_oracle, _quiet_exit  # noqa: E402

BETA = dict(fitnet=1000.0, at=1e5, gcd=0.1)          # the weights of record (scripts/run_gcn.sh; gnn.py:181-187)
AT_SYMBOLS = ("egnn_at_energy_f32", "egnn_at_partial_f32", "egnn_at_bwd_rows_f32")


def _patch_feature_ops():
    """torch restatements of the operators the three modes add to the seam (same contracts as efficient-gnns_amd/ops.py)."""
    _patch_ops_with_oracle()
    import efficient_gnns_amd.ops as ops
    import torch.nn.functional as F

    def at_energy(f, t):
        es, et = (f.detach() ** 2).sum(1), (t.detach() ** 2).sum(1)
        return es, et, torch.stack([(es * es).sum(), (et * et).sum()])

    def at_partial(es, et, sumsq_global, eps=1e-12):
        raw = sumsq_global.sqrt()
        ns, nt = raw.clamp(min=eps)
        d = es / ns - et / nt
        return torch.stack([ns, nt, raw[0], raw[1]]), torch.stack([(d * d).sum(), (d * es).sum(), (d * et).sum()])

    def at_rows_bwd(f, t, n_global, es, et, scal, sums_global, g, eps=1e-12, need_df=True, need_dt=True):
        ns, nt, raw_s, raw_t = scal
        d = es / ns - et / nt
        ps = es * sums_global[1] / ns ** 3 if raw_s > eps else torch.zeros_like(es)
        pt = et * sums_global[2] / nt ** 3 if raw_t > eps else torch.zeros_like(et)
        c = 2.0 * g / n_global
        ges, get = c * (d / ns - ps), -c * (d / nt - pt)
        return (2.0 * ges[:, None] * f.detach() if need_df else None), (2.0 * get[:, None] * t.detach() if need_dt else None)

    ops.at_energy, ops.at_partial, ops.at_rows_bwd = at_energy, at_partial, at_rows_bwd
    ops.fitnet_loss = lambda f, t, eps=1e-12: F.mse_loss(F.normalize(f, p=2, dim=-1, eps=eps), F.normalize(t, p=2, dim=-1, eps=eps))


def _hp(mode, hp):
    return dict(HP, beta=BETA[mode], **(hp or {}))


def _heads(M, mode):
    """(student head, teacher head) of ``mode`` from the module ``M`` (oracle.models / the product's models): hidden 32, proj 16."""
    if mode == "fitnet":
        return M.make_projection(32, 16), M.make_projection(750, 16)
    if mode == "gcd":
        return M.ProjectionGCD(32, 16), M.ProjectionGCD(750, 16)
    return None, None


def _reference_run(gnn, mode, hp=None, steps=3):
    import oracle.models as OM
    hp = _hp(mode, hp)
    hp.pop("static_sigmas", None)
    d = _make_data(train_ids_below=hp.pop("train_ids_below", None))
    torch.manual_seed(0)
    np.random.seed(0)
    model = (OM.GCN if gnn == "gcn" else OM.SAGE)(d.num_features, 32, d.num_classes, 3, 0.0)
    sp, tp = _heads(OM, mode)
    groups = [{"params": model.parameters(), "lr": 0.01}]
    if sp is not None:
        groups += [{"params": sp.parameters(), "lr": 0.01}, {"params": tp.parameters(), "lr": 0.01}]
    opt = torch.optim.Adam(groups)
    logits, accs = OM.evaluate(model, d.x, d.oracle_adj, d.y, d.split_idx)   # eval at the initial state
    losses = [OM.train_step(model, d.x, d.oracle_adj, d.y, d.split_idx["train"], opt, mode, hp, d.teacher_out_feat, d.teacher_logits, sp, tp)
              for _ in range(steps)]
    return losses, logits, accs


def _worker(rank, world, port, gnn, mode, hp, q):
    hp = _hp(mode, hp)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_feature_ops()
        import efficient_gnns_amd.dist as DD
        import efficient_gnns_amd.models as PM
        d = _make_data(train_ids_below=hp.pop("train_ids_below", None))
        DD._AGG_MODE = "halo"
        prob = DD.ShardedProblem(d, world, rank, "cpu", None, need_gcn=True)     # gcd needs the normalised plan under SAGE as well
        if "static_sigmas" in hp:
            prob.static_sample = DD.StaticSample(prob, hp["max_samples"], sigmas=hp.pop("static_sigmas"))
        torch.manual_seed(0)
        np.random.seed(0)
        model = (PM.GCN if gnn == "gcn" else PM.SAGE)(d.num_features, 32, d.num_classes, 3, 0.0)
        sp, tp = _heads(PM, mode)
        groups = [{"params": model.parameters(), "lr": 0.01}]
        if sp is not None:
            groups += [{"params": sp.parameters(), "lr": 0.01}, {"params": tp.parameters(), "lr": 0.01}]
        for m in (model, sp, tp):
            if m is not None:
                DD.swap_batchnorm(m)
        opt = torch.optim.Adam(groups)
        out, accs = DD.sharded_evaluate(model, prob)
        losses = [DD.sharded_train_step(model, prob, opt, mode, hp, sp, tp) for _ in range(3)]
        with DD.CommTrace() as trace:          # one more step with the collectives recorded
            DD.sharded_train_step(model, prob, opt, mode, hp, sp, tp)
        gathered, comm = [None] * world, [None] * world
        dist.all_gather_object(gathered, (out.numpy(), int(prob.train_local.numel())))
        dist.all_gather_object(comm, trace.records)
        if rank == 0:
            q.put((losses, np.concatenate([g[0] for g in gathered], 0), accs, prob.adj.plan.n_halo, DD.consistent_collectives(comm),
                   [g[1] for g in gathered]))
    except BaseException:
        import traceback
        traceback.print_exc()
        os._exit(1)
    _quiet_exit()


def _spawn_and_collect(target, world, args):
    """Rank 0's payload.  A rank that dies before it is delivered fails the test at once (its peers, stuck in a collective, are ended)."""
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    while q.empty() and all(p.exitcode is None for p in procs):
        procs[0].join(0.05)
    if q.empty():
        codes = [p.exitcode for p in procs]
        for p in procs:
            p.kill()
            p.join()
        pytest.fail(f"a rank ended before the result was delivered: exit codes {codes}")
    got = q.get()          # read before join: the payload is larger than the pipe buffer
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    return got


def _run_and_compare(gnn, mode, world, hp):
    got = _spawn_and_collect(_worker, world, (gnn, mode, hp))
    losses, logits, accs, n_halo, inconsistent, n_train = got
    assert inconsistent is None, inconsistent
    ref_losses, ref_logits, ref_accs = _reference_run(gnn, mode, hp)
    np.testing.assert_allclose(np.array(losses), np.array(ref_losses), rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(logits, ref_logits.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(accs, ref_accs, atol=1e-9)
    assert n_halo > 0
    return n_train


@pytest.mark.parametrize("gnn,mode,world,sigmas", [("gcn", "fitnet", 2, None), ("sage", "fitnet", 3, None), ("gcn", "at", 2, None),
                                                   ("sage", "at", 3, None), ("gcn", "gcd", 2, None), ("sage", "gcd", 3, 6.0)])
def test_sharded_feature_modes_match_single_process_oracle(gnn, mode, world, sigmas):
    """Three steps at the weights of record: steps 2 and 3 see step 1's auxiliary gradient (beta = 1000 / 1e5), so a wrong backward or a
    wrong scaling of a rank's share shows in their losses."""
    hp = dict(max_samples=96)
    if sigmas is not None:
        hp["static_sigmas"] = sigmas
    n_train = _run_and_compare(gnn, mode, world, hp)
    assert all(n > 0 for n in n_train)


@pytest.mark.parametrize("mode", ["fitnet", "at", "gcd"])
def test_sharded_feature_modes_with_a_rank_without_train_rows(mode):
    """Every train node below id 300, three ranks: the last one owns no train row and still runs every collective of the step (the two
    AT all-reduces, both heads' SyncBN, gcd's halo exchanges forward and backward) -- a missing one is a hang, a detached term an error."""
    n_train = _run_and_compare("gcn", mode, 3, dict(max_samples=64, train_ids_below=300))
    assert n_train[-1] == 0 and n_train[0] > 0


def _at_grad_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_feature_ops()
        import efficient_gnns_amd.dist as DD
        f_all, t_all, cuts = _at_problem()
        f = f_all[cuts[rank]:cuts[rank + 1]].clone().requires_grad_(True)
        t = t_all[cuts[rank]:cuts[rank + 1]].clone().requires_grad_(True)
        loss = DD._DistAT.apply(f, t, f_all.shape[0], 1e-12, None)
        (loss * 3.0).backward()
        everyone = [None] * world
        dist.all_gather_object(everyone, (loss.item(), f.grad.numpy(), t.grad.numpy()))
        if rank == 0:
            q.put(everyone)
    except BaseException:
        import traceback
        traceback.print_exc()
        os._exit(1)
    _quiet_exit()


def _at_problem():
    g = torch.Generator().manual_seed(11)
    n = 23
    return torch.randn(n, 32, generator=g), torch.randn(n, 75, generator=g) * 0.3, [0, 14, 23, 23]      # the last rank owns no row


def test_dist_at_gradients_match_the_oracle_on_the_concatenated_rows():
    import oracle.criterion as OC
    everyone = _spawn_and_collect(_at_grad_worker, 3, ())
    f_all, t_all, cuts = _at_problem()
    f, t = f_all.clone().requires_grad_(True), t_all.clone().requires_grad_(True)
    logits, labels = torch.zeros(f.shape[0], 2), torch.zeros(f.shape[0], dtype=torch.int64)
    ref = OC.at_criterion(logits, labels, f, t, 1.0)[2]
    (ref * 3.0).backward()
    for r, (loss, df, dt) in enumerate(everyone):
        np.testing.assert_allclose(loss, ref.item(), rtol=2e-5)                 # the global value on every rank, the empty one included
        for got, full in ((df, f.grad.numpy()), (dt, t.grad.numpy())):
            want = full[cuts[r]:cuts[r + 1]]
            assert got.shape == want.shape
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * float(np.abs(full).max()))


def test_split_at_entry_points_are_declared_and_bound():
    from efficient_gnns_amd import _lib
    with open(os.path.join(ROOT, "include", "egnn_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", header)
    for name in AT_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/egnn_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i32 and len(args) == n_args, (name, n_args, len(args))
