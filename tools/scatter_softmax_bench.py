#!/usr/bin/env python3
"""Milliseconds of the attention softmax of a user-defined conv, forward + backward, at the size of the arxiv message graph (the
``data.arxiv_like`` graph, bidirected, one loop per node: ``utils.dgl_bidirected_with_self_loops``; the edges in a seeded random
order, the targets are the softmax groups), for ``H`` heads in {1, 3, 8}, run on the same GPU in the same process:

  hip          ``ops.scatter_softmax(scores [E, H], plan=...)`` (csrc/scatter_softmax.hip) over a READY deferred plan -- inside
               ``MessagePassing.propagate`` the plan is the one the lift and the aggregation use anyway
  hip+plan     the same with the deferred ``ops.rows_plan`` built inside the timed region (a softmax outside ``propagate``)
  torch        torch ops only: ``scatter_reduce(amax)`` + gathers + ``index_add_``, differentiated by autograd
  argsort      H = 1 only: the 1-D ``utils.softmax`` path (argsort, two gathers, sorted-segment kernels, inverse permutation)

Every form computes exp(x - max) / (sum + 1e-16) and its gradient for the same upstream gradient; the outputs and gradients are
compared with the torch form before the timing (max abs difference, printed).  Warm-up rounds first, then alternating repeats timed
with device events around forward + backward; median and minimum are reported.  Prints a table and one JSON line per H.

  python tools/scatter_softmax_bench.py [--scale 1.0] [--heads 1 3 8] [--reps 15] [--warmup 5] [--sorted]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(args):
    import torch

    sys.path.insert(0, ROOT)
    import bench  # noqa: E402  (cap_cpu_threads)
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.utils as PU
    from efficient_gnns_amd import _lib, ops

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)                   # before the first load
    bench.cap_cpu_threads()
    assert torch.cuda.is_available(), "scatter_softmax_bench needs a GPU"
    dev = torch.device("cuda", 0)
    d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=False)
    row, _, _ = PU.dgl_bidirected_with_self_loops(d.adj_t).coo()                   # row = the target of every message
    n, E = d.num_nodes, row.numel()
    if not args.sorted:
        row = row[torch.randperm(E, generator=torch.Generator().manual_seed(0))]
    index = row.to(dev).contiguous()
    longest = int(torch.bincount(row, minlength=n).max())
    plan = ops.rows_plan(index, n, check="deferred")
    print(f"softmax over {E} scores in {n} groups (longest {longest}), forward + backward")

    for H in args.heads:
        g0 = torch.Generator().manual_seed(H)
        x = (3 * torch.randn(E, H, generator=g0)).to(dev).requires_grad_(True)
        gy = torch.randn(E, H, generator=g0).to(dev)

        def hip(p=plan):
            out = ops.scatter_softmax(x, index, n, plan=p, eps=1e-16)
            return out, torch.autograd.grad(out, x, gy)[0]

        def hip_plan():
            return hip(ops.rows_plan(index, n, check="deferred"))

        def torch_form():
            ix = index.view(-1, 1).expand(E, H)
            m = torch.zeros(n, H, device=dev).scatter_reduce(0, ix, x.detach(), "amax", include_self=False)
            e = (x - m.index_select(0, index)).exp()
            z = torch.zeros(n, H, device=dev).index_add_(0, index, e)
            out = e / (z.index_select(0, index) + 1e-16)
            return out, torch.autograd.grad(out, x, gy)[0]

        def argsort_form():
            out = PU.softmax(x[:, 0], index, num_nodes=n)
            return out.view(-1, 1), torch.autograd.grad(out, x, gy[:, 0])[0]

        forms = {"hip": hip, "hip+plan": hip_plan, "torch": torch_form}
        if H == 1:
            forms["argsort"] = argsort_form
        ref_out, ref_gx = torch_form()
        diffs = {}
        for name, fn in forms.items():
            out, gx = fn()
            diffs[name] = (float((out - ref_out).detach().abs().max()), float((gx - ref_gx).abs().max()))
        times = {k: [] for k in forms}
        for rep in range(args.warmup + args.reps):
            for name, fn in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[name].append(a.elapsed_time(b))
        res = {"what": "scatter_softmax_fwd_bwd", "scale": args.scale, "groups": n, "scores": E, "longest_group": longest, "heads": H,
               "sorted_index": bool(args.sorted), "reps": args.reps, "warmup": args.warmup, "rows_oob": ops.rows_oob(dev)}
        print(f"H = {H}")
        print(f"{'form':<12}{'median ms':>12}{'min ms':>10}{'max |out - torch|':>22}{'max |dx - torch|':>20}")
        for name in forms:
            med, lo = statistics.median(times[name]), min(times[name])
            res[name + "_ms"], res[name + "_min_ms"] = round(med, 3), round(lo, 3)
            res[name + "_max_abs_diff"] = [float(f"{v:.3e}") for v in diffs[name]]
            print(f"{name:<12}{med:>12.3f}{lo:>10.3f}{diffs[name][0]:>22.3e}{diffs[name][1]:>20.3e}")
        print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the arxiv graph's size (1.0: 169 343 nodes)")
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sorted", action="store_true", help="keep the edges grouped by target instead of a random order")
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    main(ap.parse_args())
