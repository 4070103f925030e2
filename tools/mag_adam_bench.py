#!/usr/bin/env python3
"""The MAG mini-batch step under three optimisers, in ONE process (tools only; numbers go to profiles/ and DESIGN.md 6c):

  (a) torch.optim.Adam(model.parameters())               -- the reference's optimiser (mag_pyg/gnn.py:424), as tools/ppi_mag_bench.py times it
  (b) torch.optim.Adam(model.parameters(), fused=True)
  (c) models.mag_optimizer(model, lr)                    -- optim.LazyRowAdam: the embedding tables stepped row-lazily

mag_hetero_like(--mag-scale), GraphSAINT batch 20 000, walk length 2, supervised student R-GCN 2 x 64 with batch.relations.  Per case,
over the same batches (sampler seed) and the same initial weights: the one-step time (HIP events, median of --reps steps after --warmup)
split into forward + loss | backward | optimiser step, the peak device memory of those steps above what model, graph and sampler
hold before the optimiser exists (so the optimiser state counts in every case; its own size is reported as optimizer_state_MB), and
one epoch of --epoch-steps steps plus
the end-of-epoch flush plus mag_test (the flush is timed on its own as well).  One JSON line per case."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (cap_cpu_threads)
import efficient_gnns_amd.data as D  # noqa: E402
import efficient_gnns_amd.models as PM  # noqa: E402
import efficient_gnns_amd.utils as PU  # noqa: E402
from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mag-scale", type=float, default=1.0)
ap.add_argument("--batch-size", type=int, default=20_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--epoch-steps", type=int, default=30)
ap.add_argument("--out", default=None, help="also write the result lines to this file")
args = ap.parse_args()
bench.cap_cpu_threads()
if not torch.cuda.is_available():
    sys.exit("mag_adam_bench.py measures on the GPU only")
dev = torch.device("cuda", 0)


def ev():
    return torch.cuda.Event(enable_timing=True)


def med(xs):
    return round(statistics.median(xs), 3)


def state_bytes(opt):
    """Bytes of optimiser state on the device: torch Adam's per-parameter tensors; for LazyRowAdam also m, v and last of every table."""
    tensors = []
    for st in getattr(opt, "_rows", {}).values():
        tensors += [st.m, st.v, st.last, st.dup]
    inner = getattr(opt, "_inner", None) if hasattr(opt, "_rows") else opt
    if inner is not None:
        for s in inner.state.values():
            tensors += [v for v in s.values() if torch.is_tensor(v) and v.is_cuda]
    return sum(t.numel() * t.element_size() for t in tensors)


d = D.mag_hetero_like(scale=args.mag_scale, seed=0)
eid = {k: v.to(dev) for k, v in d.edge_index_dict.items()}
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
homo.y[l2g["paper"]] = d.y_dict["paper"].to(dev)
homo.train_mask = torch.zeros(N, dtype=torch.bool, device=dev)
homo.train_mask[l2g["paper"][d.split_idx["train"]["paper"].to(dev)]] = True
x_dict = {key2int["paper"]: d.x_dict["paper"].to(dev)}
nn_dict = {key2int[k]: n for k, n in d.num_nodes_dict.items()}
y_paper = d.y_dict["paper"].to(dev)
hp = dict(alpha=0.9, kd_T=4.0)
LR = 0.005
CASES = {
    "a_adam": lambda m: torch.optim.Adam(m.parameters(), lr=LR),
    "b_adam_fused": lambda m: torch.optim.Adam(m.parameters(), lr=LR, fused=True),
    "c_lazy_rows": lambda m: PM.mag_optimizer(m, LR),
}
lines = []
for name, make in CASES.items():
    torch.manual_seed(0)
    model = PM.RGCN(128, 64, d.num_classes, 2, 0.5, nn_dict, list(x_dict), len(eid)).to(dev)
    PM.train_mode(model)
    smp = GraphSAINTRandomWalkSampler(homo, batch_size=args.batch_size, walk_length=2, num_steps=1, seed=1)
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated()
    opt = make(model)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    stage = {k: [] for k in ("forward_loss", "backward", "optimizer", "step")}
    for i in range(args.reps + args.warmup):
        bt = smp.sample()
        e = [ev() for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        loss = PM.mag_batch_loss(model, bt, x_dict, "supervised", hp)[0]
        e[1].record()
        opt.zero_grad()
        loss.backward()
        e[2].record()
        opt.step()
        e[3].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            for j, k in enumerate(("forward_loss", "backward", "optimizer")):
                stage[k].append(e[j].elapsed_time(e[j + 1]))
            stage["step"].append(e[0].elapsed_time(e[3]))
    res = {"what": "mag_adam_step", "case": name, "N": N, "batch_size": args.batch_size, "walk_length": 2, "student": "RGCN 2x64",
           "reps": args.reps, "warmup": args.warmup, "n_sub": bt.num_nodes}
    for k, v in stage.items():
        res[f"{k}_ms"] = med(v)
    res["peak_step_memory_MB"] = round((torch.cuda.max_memory_allocated() - base_mem) / 2 ** 20, 1)
    res["optimizer_state_MB"] = round(state_bytes(opt) / 2 ** 20, 1)
    res["model_graph_sampler_MB"] = round(base_mem / 2 ** 20, 1)
    # one epoch: --epoch-steps steps, the end-of-epoch flush (inside mag_train_epoch), then mag_test
    loader = GraphSAINTRandomWalkSampler(homo, batch_size=args.batch_size, walk_length=2, num_steps=args.epoch_steps, seed=2)
    flush_ev = []
    if hasattr(opt, "flush"):
        inner_flush = opt.flush

        def timed_flush():
            a, b = ev(), ev()
            a.record()
            inner_flush()
            b.record()
            flush_ev.append((a, b))
        opt.flush = timed_flush
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    PM.mag_train_epoch(model, loader, x_dict, opt, "supervised", hp)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    accs = PM.mag_test(model, x_dict, eid, key2int, y_paper, d.split_idx)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res["epoch_steps"] = args.epoch_steps
    res["epoch_train_ms"] = round((t1 - t0) * 1e3, 1)
    res["epoch_test_ms"] = round((t2 - t1) * 1e3, 1)
    res["epoch_total_ms"] = round((t2 - t0) * 1e3, 1)
    res["epoch_flush_ms"] = round(sum(a.elapsed_time(b) for a, b in flush_ev), 3) if flush_ev else None
    res["accs"] = [round(a, 4) for a in accs]
    lines.append(res)
    print(json.dumps(res), flush=True)
    del model, opt, smp, loader, loss, bt
    gc.collect()
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
