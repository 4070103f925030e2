#!/usr/bin/env python3
"""egnn_rows_add_runs_f32 against torch.Tensor.index_add_ on the same device tensors (tools only; the numbers go to DESIGN.md 3.5).

Shape: the arxiv LSP gradient -- the edge endpoints of the train subgraph of ``data.arxiv_like(--scale)`` index the [n_train, C] rows of
``out_feat[train_idx]`` (C = 256), so row r is named as often as train node r has edges inside the subgraph (power law: a hub thousands
of times, the median a handful).  Timed with device events, median of --reps calls after --warmup, alternating the two; the plan build
(keys, sort, counters, ONE host read) is timed on its own with a host clock around a synchronise.  Also checks the two results against
each other within the bound of k fp32 additions in any order, and two run-add calls bit for bit.  One JSON line."""
import argparse
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
import efficient_gnns_amd.ops as ops  # noqa: E402
from efficient_gnns_amd import _lib  # noqa: E402
from efficient_gnns_amd.utils import subgraph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--C", type=int, default=256)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the result line to this file")
ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)                       # before the first load
bench.cap_cpu_threads()
if not torch.cuda.is_available():
    sys.exit("rows_sum_bench.py measures on the GPU only")
dev = torch.device("cuda", 0)

d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=False)
row, col, _ = d.adj_t.coo()
train_idx = d.split_idx["train"]
ei = subgraph(train_idx, torch.stack([row, col]), relabel_nodes=True, num_nodes=d.num_nodes)[0]
n_rows, idx = train_idx.numel(), ei[0].contiguous().to(dev)          # the source endpoints, in the edge list's order
S, C = idx.numel(), args.C
g = torch.Generator().manual_seed(0)
src = torch.randn(S, C, generator=g).to(dev)
counts = torch.bincount(idx, minlength=n_rows)


def timed_plan():
    ops._ROWS_PLANS.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = ops.rows_plan(idx, n_rows)
    torch.cuda.synchronize()
    return plan, (time.perf_counter() - t0) * 1e3


plan, _ = timed_plan()                                               # first call: code objects, hipCUB's configuration
plan_ms = [timed_plan()[1] for _ in range(5)]
plan = ops.rows_plan(idx, n_rows)
assert plan.dups == S - int((counts > 0).sum()) and plan.longest == int(counts.max())

out_runs, out_atomic = torch.empty(n_rows, C, device=dev), torch.empty(n_rows, C, device=dev)


def run_add():
    ops._rows_add_runs(out_runs, plan, src, False)


def index_add():
    out_atomic.zero_()
    out_atomic.index_add_(0, idx, src)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


times = {"run_add": [], "index_add": []}
for i in range(args.warmup + args.reps):
    for name, fn in (("run_add", run_add), ("index_add", index_add)):
        t = event_ms(fn)
        if i >= args.warmup:
            times[name].append(t)
first = out_runs.clone()
run_add()
torch.cuda.synchronize()
k = counts.double().clamp(min=1).unsqueeze(1)
gamma = k * 2.0 ** -24 / (1 - k * 2.0 ** -24)
mag = torch.zeros(n_rows, C, dtype=torch.float64, device=dev).index_add_(0, idx, src.double().abs())
res = {"what": "rows_add_runs vs index_add_", "scale": args.scale, "n_rows": n_rows, "S": S, "C": C, "duplicates": plan.dups,
       "longest_run": plan.longest, "median_run": float(counts[counts > 0].double().median()),
       "run_add_ms": round(statistics.median(times["run_add"]), 4), "index_add_ms": round(statistics.median(times["index_add"]), 4),
       "index_add_includes": "zero_() of the [n_rows, C] output (run_add zeroes unnamed rows itself)",
       "plan_build_ms": round(statistics.median(plan_ms), 3), "reps": args.reps, "warmup": args.warmup,
       "two_run_add_calls_bit_equal": bool(torch.equal(first, out_runs)),
       "within_any_order_bound_of_each_other": bool(((out_runs.double() - out_atomic.double()).abs() <= 2 * gamma * mag).all())}
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
