#!/usr/bin/env python3
"""egnn_sddmm_csr_f32 (the value gradient of an aggregation) against the torch-op form and against the SpMM over the same adjacency
(tools only; the numbers go to DESIGN.md 3.1b).

Shape: the gcn-normalised adjacency A^ of ``data.arxiv_like(--scale)`` (nnz ~ 2.48 M at scale 1: power law, hub rows of more than
13 000 entries), at every width of --K.  Three things are timed in one process, alternating, each as --launches calls between two device
events, median of --reps such windows after --warmup:
  sddmm   ops.sddmm(A^, g, x)                      the new kernel
  torch   (g[row] * x[col]).sum(-1)                what a user would otherwise write: two [nnz, K] temporaries
  spmm    ops.spmm_raw(A^, x, "sum")               the yardstick: gathers the same nnz * K * 4 bytes, writes Y rows where the SDDMM
                                                   reads G rows and writes nnz floats
Also checks the kernel against the torch-op form within the bound of a length-K fp32 dot product in any order, and two kernel calls bit
for bit.  One JSON line per width."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (cap_cpu_threads)
import efficient_gnns_amd.data as D  # noqa: E402
import efficient_gnns_amd.ops as ops  # noqa: E402
from efficient_gnns_amd.sparse import gcn_norm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--K", type=int, nargs="+", default=[256, 40])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--launches", type=int, default=20, help="calls between the two events of one timed window")
ap.add_argument("--out", default=None, help="also append the result lines to this file")
args = ap.parse_args()
bench.cap_cpu_threads()
if not torch.cuda.is_available():
    sys.exit("sddmm_bench.py measures on the GPU only")
dev = torch.device("cuda", 0)

d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=False)
adj = gcn_norm(d.adj_t.to(dev))
n, nnz = adj.sparse_size(0), adj.nnz()
row, col = adj._row(), adj._col
_, _, bits = adj._index_arrays()
cnt = adj.storage.rowcount()


def window_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


lines = []
for K in args.K:
    gen = torch.Generator().manual_seed(K)
    g, x = torch.randn(n, K, generator=gen).to(dev), torch.randn(n, K, generator=gen).to(dev)
    fns = {"sddmm": lambda: ops.sddmm(adj, g, x), "torch": lambda: (g[row] * x[col]).sum(-1), "spmm": lambda: ops.spmm_raw(adj, x, "sum")}
    times = {k: [] for k in fns}
    for i in range(args.warmup + args.reps):
        for name, fn in fns.items():
            t = window_ms(fn, args.launches)
            if i >= args.warmup:
                times[name].append(t)
    got, again, ref = ops.sddmm(adj, g, x), ops.sddmm(adj, g, x), (g.double()[row] * x.double()[col])
    u = 2.0 ** -24
    bound = (K + 2) * u / (1 - (K + 2) * u) * ref.abs().sum(-1)
    med = {k: statistics.median(v) for k, v in times.items()}
    index_bytes = nnz * (bits // 8) + (n + 1) * (bits // 8)
    res = {"what": "sddmm vs torch ops vs spmm", "scale": args.scale, "n": n, "nnz": nnz, "K": K, "index_bits": bits,
           "longest_row": int(cnt.max()), "median_row": float(cnt.double().median()),
           "sddmm_us": round(med["sddmm"] * 1e3, 2), "torch_ops_us": round(med["torch"] * 1e3, 2), "spmm_us": round(med["spmm"] * 1e3, 2),
           "sddmm_over_spmm": round(med["sddmm"] / med["spmm"], 3), "sddmm_over_torch_ops": round(med["sddmm"] / med["torch"], 3),
           "algorithmic_bytes": {"gather_x": 4 * nnz * K, "read_g": 4 * n * K, "index": index_bytes, "write_dval": 4 * nnz},
           "sddmm_algorithmic_GBps": round((4 * nnz * K + 4 * n * K + index_bytes + 4 * nnz) / (med["sddmm"] * 1e-3) / 1e9, 1),
           "reps": args.reps, "warmup": args.warmup, "launches_per_window": args.launches,
           "two_calls_bit_equal": bool(torch.equal(got, again)),
           "within_any_order_bound_of_float64": bool(((got.double() - ref.sum(-1)).abs() <= bound).all())}
    del ref, bound
    print(json.dumps(res), flush=True)
    lines.append(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
