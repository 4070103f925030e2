#!/usr/bin/env python3
"""ms per PPI training step of the GAT student (``StudentNet``, ppi_pyg/gnn.py:50-83) and the GAT teacher (``TeacherNet``,
:23-47, ppi_pyg/train_teacher.py): ``model.train()``, forward, multi-label BCE with logits, backward, Adam step, over the 20
``data.ppi_like`` train graphs.  Synchronised CUDA events around every step; the warm-up epoch is excluded.  Prints one JSON line.

  --steps K      timed steps per model (cycling over the 20 graphs)
  --breakdown    also times forward (to the loss) and backward (+ optimiser step) separately
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (cap_cpu_threads)
import efficient_gnns_amd.data as D  # noqa: E402
import efficient_gnns_amd.models as PM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--breakdown", action="store_true")
args = ap.parse_args()
bench.cap_cpu_threads()
dev = torch.device("cuda", 0)

train, _, _ = D.ppi_like(seed=0)
graphs = [(g.x.to(dev), g.edge_index.to(dev), g.y.to(dev)) for g in train]


def time_model(model):
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    model.train()

    def step(x, ei, y, ev):
        ev[0].record()
        loss = F.binary_cross_entropy_with_logits(model(x, ei), y)
        ev[1].record()
        opt.zero_grad()
        loss.backward()
        opt.step()
        ev[2].record()

    for x, ei, y in graphs:                                        # warm-up: one epoch (structures cached, kernels loaded)
        step(x, ei, y, [torch.cuda.Event(enable_timing=True) for _ in range(3)])
    torch.cuda.synchronize()
    fwd, tot = [], []
    for k in range(args.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        step(*graphs[k % len(graphs)], ev)
        torch.cuda.synchronize()
        fwd.append(ev[0].elapsed_time(ev[1]))
        tot.append(ev[0].elapsed_time(ev[2]))
    n = len(tot)
    out = {"ms_per_step": round(sum(tot) / n, 4)}
    if args.breakdown:
        out["fwd_ms"] = round(sum(fwd) / n, 4)
        out["bwd_step_ms"] = round((sum(tot) - sum(fwd)) / n, 4)
    return out


torch.manual_seed(0)
res = {"workload": "ppi_gat_train", "graphs": len(graphs), "nodes": sum(g[0].shape[0] for g in graphs),
       "steps": args.steps, "student": time_model(PM.StudentNet(50, 121).to(dev)),
       "teacher": time_model(PM.TeacherNet(50, 121).to(dev))}
print(json.dumps(res), flush=True)
