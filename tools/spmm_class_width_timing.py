#!/usr/bin/env python3
"""Per-call time of the class-width (K = 40) aggregation on the headline graph: the segment schedule it ran on
(EGNN_SPMM_CLASS_WIDTH=0) against the 16-lane form behind egnn_spmm_csr_blk_f32 (csrc/spmm_blk.hip).

    python tools/spmm_class_width_timing.py [--out FILE.json] [--k 40] [--timeout 300]

The parent process never opens the GPU: every case runs in a child process of its own under a time limit.  A child
alternates the two paths (5 warm-ups, then 30 calls each, one device-event pair per call behind a filler kernel that keeps the
queue busy while the host enqueues; the combine launch of the hub rows is inside the pair on both sides), checks that the
outputs are torch.equal and prints one JSON line with the medians.  Cases: A^ (GCN forward / evaluation) and A^T (backward)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("forward", "backward")
SWITCH = "EGNN_SPMM_CLASS_WIDTH"


def child(case: str, K: int) -> None:
    import torch
    sys.path.insert(0, ROOT)
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.ops as ops
    from efficient_gnns_amd.build import source_stamp
    from efficient_gnns_amd.sparse import gcn_norm

    dev = torch.device("cuda:0")
    data = D.arxiv_like(1.0, with_teacher=False)
    adj = gcn_norm(data.adj_t.to(dev))
    if case == "backward":
        adj = adj.t()
    n = adj.sparse_size(1)
    x = torch.randn(n, K, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    filler = torch.randn(4096, 4096, device=dev)

    def path(switch):
        def f():
            os.environ[SWITCH] = switch      # read by ops at every call
            return ops.spmm_raw(adj, x, "sum")[0]
        return f

    paths = {"segments": path("0"), "class_width": path("1")}
    outs = {k: f() for k, f in paths.items()}
    equal = bool(torch.equal(outs["segments"], outs["class_width"]))
    times = {k: [] for k in paths}
    for it in range(35):
        for k, f in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(filler, filler)          # the device is still busy when the timed launches are enqueued
            a.record()
            f()
            b.record()
            b.synchronize()
            if it >= 5:
                times[k].append(a.elapsed_time(b) * 1e3)
    res = dict(case=case, K=K, n=n, nnz=adj.nnz(), equal=equal, source_stamp=source_stamp(), device=torch.cuda.get_device_name(0))
    for k, t in times.items():
        t.sort()
        res[k] = dict(median_us=round(t[len(t) // 2], 2), min_us=round(t[0], 2), max_us=round(t[-1], 2), calls=len(t))
    print("RESULT " + json.dumps(res), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child process")
    ap.add_argument("--child", default=None, choices=CASES)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.k)
        return 0
    results = []
    for case in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--k", str(args.k)], capture_output=True,
                               text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{case}: time limit", file=sys.stderr)
            return 1
        if p.returncode != 0:     # a failed child ends the run: nothing more is started on the device
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            return p.returncode or 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        results.append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/spmm_class_width_timing.py", per_call=results), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
