#!/usr/bin/env python3
"""Secondary BASELINE.json configs that bench.py does not time (tools only; numbers go to profiles/ and DESIGN.md):

  configs[0]  PPI, 2-layer GCN-256 student, logit KD, one optimisation step per graph (ppi_pyg/gnn.py:185-274) --
              timed WITH the frozen GAT teacher (TeacherNet) forward inside every step, as the reference does
              (:208-209), and WITHOUT it (teacher logits precomputed), on the GPU and with the CPU oracle;
  configs[4]  MAG-shaped SAGE-mean aggregation (mag_pyg/gnn.py:162): the mean-SpMM at N = 1.94 M / 42 M entries.
  --saint     (runs alone) the MAG GraphSAINT mini-batch (mag_pyg/gnn.py:174-268,361-366) at mag_hetero_like(--mag-scale),
              batch_size 20 000, walk_length 2 and 3: (i) one batch of the device sampler split into walk / select / induced /
              relations, (ii) the same batch formed with torch ops on the same GPU (gathers, unique, a boolean edge mask,
              RGCNConv._relations: what a user without saint.py writes), (iii) one student step and one teacher-in-the-loop kd
              step with batch.relations and with relations=None.  HIP events, median over --saint-reps batches after warm-up.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (cap_cpu_threads)
import efficient_gnns_amd as E  # noqa: E402
import efficient_gnns_amd.data as D  # noqa: E402
import efficient_gnns_amd.models as PM  # noqa: E402
import efficient_gnns_amd.ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mag-scale", type=float, default=1.0)
ap.add_argument("--cpu-graphs", type=int, default=4, help="PPI graphs timed with the CPU oracle (0 = skip)")
ap.add_argument("--saint", action="store_true", help="time the MAG GraphSAINT mini-batch leg only")
ap.add_argument("--saint-reps", type=int, default=9)
ap.add_argument("--saint-out", default=None, help="also write the --saint result lines to this file")
args = ap.parse_args()
bench.cap_cpu_threads()
dev = torch.device("cuda", 0)


def sync():
    torch.cuda.synchronize()


def saint_leg():
    import statistics
    import efficient_gnns_amd.utils as PU
    from efficient_gnns_amd import _lib
    from efficient_gnns_amd.nn import RGCNConv
    from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler
    lines = []
    t0 = time.perf_counter()
    d = D.mag_hetero_like(scale=args.mag_scale, seed=0)
    eid = {k: v.to(dev) for k, v in d.edge_index_dict.items()}
    for key, rev in ((("author", "affiliated_with", "institution"), ("institution", "to", "author")),
                     (("author", "writes", "paper"), ("paper", "to", "author")),
                     (("paper", "has_topic", "field_of_study"), ("field_of_study", "to", "paper"))):
        r, c = eid[key]
        eid[rev] = torch.stack([c, r])
    eid[("paper", "cites", "paper")] = PU.to_undirected(eid[("paper", "cites", "paper")])
    edge_index, edge_type, node_type, local_idx, l2g, key2int = PU.group_hetero_graph(eid, d.num_nodes_dict)
    N, E_ = node_type.numel(), edge_index.shape[1]
    homo = Data(edge_index=edge_index, edge_attr=edge_type, node_type=node_type, local_node_idx=local_idx, num_nodes=N)
    homo.y = node_type.new_full((N, 1), -1)
    homo.y[l2g["paper"]] = d.y_dict["paper"].to(dev)
    homo.train_mask = torch.zeros(N, dtype=torch.bool, device=dev)
    homo.train_mask[l2g["paper"][d.split_idx["train"]["paper"].to(dev)]] = True
    T, NT, B, reps = len(eid), len(d.num_nodes_dict), 20_000, args.saint_reps
    sync()
    prep_s = time.perf_counter() - t0

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def med(xs):
        return round(statistics.median(xs), 3)

    for L in (2, 3):
        t0 = time.perf_counter()
        smp = GraphSAINTRandomWalkSampler(homo, batch_size=B, walk_length=L, num_steps=1, seed=1)
        sync()
        res = {"what": "mag_saint_batch", "N": N, "E": E_, "edge_types": T, "batch_size": B, "walk_length": L, "reps": reps,
               "dataset_prep_s": round(prep_s, 1), "sampler_construction_s": round(time.perf_counter() - t0, 2)}
        # (i) the device sampler: whole batches (events around sample(), which contains its one host read), then its stages
        tot, wall = [], []
        for i in range(reps + 3):
            a, b_ = ev(), ev()
            sync()
            w0 = time.perf_counter()
            a.record()
            bt = smp.sample()
            b_.record()
            sync()
            if i >= 3:
                tot.append(a.elapsed_time(b_))
                wall.append((time.perf_counter() - w0) * 1e3)
        res["device_batch_ms"], res["device_batch_wall_ms"] = med(tot), med(wall)
        res["n_sub"], res["e_sub"] = bt.num_nodes, bt.edge_index.shape[1]
        lib, p, st = _lib.load(), _lib.ptr, _lib.stream()
        cap = min(N, B * (L + 1))
        rel_rowptr, rel_col = smp._rel[2], smp._rel[3]
        stage = {k: [] for k in ("walk", "select", "induced", "relations")}
        for i in range(reps + 3):
            flag = smp._flag.zero_()
            walks = torch.empty((B, L + 1), dtype=torch.int64, device=dev)
            relabel, node_buf = torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
            counts, eptr = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap + 1, dtype=torch.int64, device=dev)
            rcounts, rptr = torch.empty(T * cap, dtype=torch.int64, device=dev), torch.empty(T * cap + 1, dtype=torch.int64, device=dev)
            ws_n, ws_c, ws_r = smp._workspace(N), smp._workspace(cap), smp._workspace(T * cap)
            e = [ev() for _ in range(7)]
            sync()
            e[0].record()
            _lib.check(lib.egnn_saint_random_walk_i64(p(smp._rowptr), p(smp._col), N, E_, B, L, None, None, 5 + i, None, p(walks), p(flag), st), "walk")
            e[1].record()
            _lib.check(lib.egnn_saint_select_i64(p(flag), N, p(relabel), p(node_buf), cap, p(ws_n), ws_n.numel(), st), "select")
            e[2].record()
            n_dev = relabel[N:]
            _lib.check(lib.egnn_saint_induced_count_i64(p(smp._rowptr), p(smp._col), p(node_buf), cap, p(n_dev), 1, 0, N, p(flag), p(counts),
                                                        p(eptr), p(ws_c), ws_c.numel(), st), "count")
            e[3].record()
            _lib.check(lib.egnn_saint_induced_count_i64(p(rel_rowptr), p(rel_col), p(node_buf), cap, p(n_dev), T, N, N, p(flag), p(rcounts),
                                                        p(rptr), p(ws_r), ws_r.numel(), st), "rel count")
            e[4].record()
            sizes = torch.cat([n_dev, eptr[cap:], rptr[-1:]]).tolist()
            n_sub, e_sub, r_sub = sizes
            ei, eidx, rcol = (torch.empty((2, e_sub), dtype=torch.int64, device=dev), torch.empty(e_sub, dtype=torch.int64, device=dev),
                              torch.empty(r_sub, dtype=torch.int64, device=dev))
            e[4].record()
            _lib.check(lib.egnn_saint_induced_fill_i64(p(smp._rowptr), p(smp._col), p(smp._val), p(node_buf), cap, p(n_dev), 1, 0, N, p(flag),
                                                       p(relabel), p(eptr), e_sub, p(ei[0]), p(ei[1]), p(eidx), st), "fill")
            e[5].record()
            _lib.check(lib.egnn_saint_induced_fill_i64(p(rel_rowptr), p(rel_col), None, p(node_buf), cap, p(n_dev), T, N, N, p(flag),
                                                       p(relabel), p(rptr), r_sub, None, p(rcol), None, st), "rel fill")
            e[6].record()
            sync()
            if i >= 3:
                stage["walk"].append(e[0].elapsed_time(e[1]))
                stage["select"].append(e[1].elapsed_time(e[2]))
                stage["induced"].append(e[2].elapsed_time(e[3]) + e[4].elapsed_time(e[5]))
                stage["relations"].append(e[3].elapsed_time(e[4]) + e[5].elapsed_time(e[6]))
        for k, v in stage.items():
            res[f"device_{k}_ms"] = med(v)
        # (ii) the same batch with torch ops on the same GPU
        rowptr, col, val = smp._rowptr, smp._col, smp._val
        row = torch.repeat_interleave(torch.arange(N, device=dev), rowptr[1:] - rowptr[:-1])
        conv = RGCNConv(8, 8, NT, T).to(dev)
        tstage = {k: [] for k in ("walk", "select", "induced", "relations", "total")}
        for i in range(reps + 3):
            e = [ev() for _ in range(5)]
            sync()
            e[0].record()
            cur = torch.randint(0, N, (B,), device=dev)
            rnd = torch.rand((B, L), device=dev)
            nodes = [cur]
            for s_ in range(L):
                r0 = rowptr[cur]
                deg = rowptr[cur + 1] - r0
                k_ = torch.minimum((rnd[:, s_] * deg.to(torch.float32)).to(torch.int64), deg - 1).clamp_min(0)
                cur = torch.where(deg > 0, col[(r0 + k_).clamp_max(E_ - 1)], cur)
                nodes.append(cur)
            e[1].record()
            node_idx = torch.stack(nodes, 1).view(-1).unique()
            e[2].record()
            sel = torch.zeros(N, dtype=torch.bool, device=dev)
            sel[node_idx] = True
            keep = sel[row] & sel[col]
            relab = torch.zeros(N, dtype=torch.int64, device=dev)
            relab[node_idx] = torch.arange(node_idx.numel(), device=dev)
            tei = torch.stack([relab[row[keep]], relab[col[keep]]])
            teidx = val[keep]
            tea, tnt = edge_type[teidx], node_type[node_idx]
            tli, ty, tm = local_idx[node_idx], homo.y[node_idx], homo.train_mask[node_idx]
            e[3].record()
            conv._relations(tei, tea, tnt, node_idx.numel())
            e[4].record()
            sync()
            if i >= 3:
                for j, k in enumerate(("walk", "select", "induced", "relations")):
                    tstage[k].append(e[j].elapsed_time(e[j + 1]))
                tstage["total"].append(e[0].elapsed_time(e[4]))
        for k, v in tstage.items():
            res[f"torch_{k}_ms"] = med(v)
        lines.append(res)
        print(json.dumps(res), flush=True)
        # (iii) training steps: student (2 x 64) and kd with the 3 x 512 teacher in the loop, with and without batch.relations
        if L == 2:
            x_dict = {key2int["paper"]: d.x_dict["paper"].to(dev)}
            nn_dict = {key2int[k]: n for k, n in d.num_nodes_dict.items()}
            torch.manual_seed(0)
            student = PM.RGCN(128, 64, d.num_classes, 2, 0.5, nn_dict, list(x_dict), T).to(dev)
            teacher = PM.RGCN(128, 512, d.num_classes, 3, 0.5, nn_dict, list(x_dict), T).to(dev).eval().requires_grad_(False)
            opt_ = torch.optim.Adam(student.parameters(), lr=0.005)
            hp = dict(alpha=0.9, kd_T=4.0)
            step = {"what": "mag_saint_step", "walk_length": L, "batch_size": B, "reps": reps, "student": "RGCN 2x64", "teacher": "RGCN 3x512"}
            for mode in ("supervised", "kd"):
                for with_rel in (True, False):
                    ts = []
                    for i in range(reps + 2):
                        bt = smp.sample()
                        if not with_rel:
                            bt.relations = None
                        a, b_ = ev(), ev()
                        sync()
                        a.record()
                        loss = PM.mag_batch_loss(student, bt, x_dict, mode, hp, teacher)[0]
                        opt_.zero_grad()
                        loss.backward()
                        opt_.step()
                        b_.record()
                        sync()
                        if i >= 2:
                            ts.append(a.elapsed_time(b_))
                    step[f"{mode}_step_ms_" + ("batch_relations" if with_rel else "relations_none")] = med(ts)
            lines.append(step)
            print(json.dumps(step), flush=True)
            del student, teacher, opt_
    if args.saint_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.saint_out)), exist_ok=True)
        with open(args.saint_out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if args.saint:
    saint_leg()
    sys.exit(0)


# ---------------------------------------------------------------- PPI
train, _, _ = D.ppi_like(seed=0)
gpu_graphs = [(g.x.to(dev), g.edge_index.to(dev), g.y.to(dev), g.teacher_logits.to(dev)) for g in train]
torch.manual_seed(0)
student = PM.GCN(50, 256, 121, 2, 0.0, cached=False).to(dev)
teacher = PM.TeacherNet(50, 121).to(dev).eval().requires_grad_(False)
opt = torch.optim.Adam(student.parameters(), lr=0.005)


def ppi_epoch(with_teacher):
    student.train()
    tot = 0.0
    for x, ei, y, tl in gpu_graphs:
        if with_teacher:
            with torch.no_grad():
                tl = teacher(x, ei)
        loss, _, _ = E.ppi_kd_criterion(student(x, ei), y, tl, 0.5, 1.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        tot += loss.item()                      # the reference accumulates loss.item() per batch (gnn.py:262-266)
    return tot


res = {}
for with_teacher in (False, True):
    for _ in range(2):
        ppi_epoch(with_teacher)
    sync()
    t0 = time.perf_counter()
    for _ in range(5):
        ppi_epoch(with_teacher)
    sync()
    res["ppi_epoch_ms_with_teacher" if with_teacher else "ppi_epoch_ms_teacher_precomputed"] = round((time.perf_counter() - t0) / 5 * 1e3, 2)
x, ei, _, _ = gpu_graphs[0]
for _ in range(3):
    with torch.no_grad():
        teacher(x, ei)
sync()
t0 = time.perf_counter()
for _ in range(20):
    with torch.no_grad():
        teacher(x, ei)
sync()
res["teacher_forward_ms_graph0"] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
res["graph0_nodes_edges"] = [int(x.shape[0]), int(ei.shape[1])]

if args.cpu_graphs > 0:
    import oracle.criterion as OC
    import oracle.models as OM
    torch.manual_seed(0)
    ostu, otea = OM.GCN(50, 256, 121, 2, 0.0, cached=False), OM.TeacherNet(50, 121).eval()
    oopt = torch.optim.Adam(ostu.parameters(), lr=0.005)
    sub = train[:args.cpu_graphs]
    for with_teacher in (False, True):
        t0 = time.perf_counter()
        for g in sub:
            tl = g.teacher_logits
            if with_teacher:
                with torch.no_grad():
                    tl = otea(g.x, g.edge_index)
            loss = OC.ppi_kd_criterion(ostu(g.x, g.edge_index), g.y, tl, 0.5, 1.0)[0]
            oopt.zero_grad()
            loss.backward()
            oopt.step()
        dt = time.perf_counter() - t0
        nodes = sum(g.num_nodes for g in sub)
        allnodes = sum(g.num_nodes for g in train)
        res["cpu_oracle_ppi_epoch_ms_" + ("with_teacher" if with_teacher else "teacher_precomputed") + "_extrapolated"] = round(
            dt * allnodes / nodes * 1e3, 1)
    res["cpu_threads"] = torch.get_num_threads()
    res["cpu_sample"] = f"{args.cpu_graphs} of 20 training graphs, scaled by node count"
print(json.dumps({"what": "ppi_2l_gcn_kd", **res}))

# ---------------------------------------------------------------- MAG-shaped mean aggregation
t0 = time.perf_counter()
d = D.mag_like(scale=args.mag_scale, seed=0)
gen_s = time.perf_counter() - t0
adj = d.adj_t.to(dev)
out = {"what": "mag_mean_spmm", "N": d.num_nodes, "nnz": adj.nnz(), "graph_generation_s": round(gen_s, 1)}
for K in (128, 256):
    xg = torch.randn(d.num_nodes, K, device=dev)
    for _ in range(2):
        ops.spmm_raw(adj, xg, "mean")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        ops.spmm_raw(adj, xg, "mean")
    e1.record()
    sync()
    us = e0.elapsed_time(e1) / 5 * 1e3
    alg = adj.spmm_algorithmic_bytes(K)
    out[f"K{K}_us"] = round(us, 1)
    out[f"K{K}_alg_GBs"] = round(alg / us / 1e3, 1)
    out[f"K{K}_gather_GBs"] = round(adj.nnz() * K * 4 / us / 1e3, 1)
    del xg
print(json.dumps(out))
