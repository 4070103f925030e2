#!/usr/bin/env python3
"""Milliseconds and peak memory of one edge-feature message-passing layer -- lift, add the edge's row, relu, aggregation -- forward +
backward, in three forms run on the same GPU in the same process over READY plans:

  fused        ``ops.gather_add_scatter(x, plan_src, plan_dst, n, edge, "relu")`` (csrc/gather_edge_scatter.hip): no [E, C] message tensor
  unfused      the composition it replaces: ``ops.scatter(torch.relu(ops.take_rows(x, plan_src) + edge), None, n, plan=plan_dst)``
  torch        torch ops only: ``index_select``, add, relu, ``index_add_``, differentiated by autograd

Cases: the arxiv message graph (the ``data.arxiv_like`` graph, bidirected, one loop per node, the edges in a seeded random order) at
C = 256, and a ``data.molhiv_like`` batch of 512 graphs at C = 300 (the GIN-E student's width).  The three forms get the same operands
and upstream gradient; outputs and gradients are compared before the timing (fused against unfused must be bit-equal: value, dx and
dedge).  Warm-up rounds first, then alternating repeats timed with device events around forward + backward; median and minimum are
reported, and per form the peak allocated memory of one forward + backward above what the operands hold.  Prints a table and appends
one JSON line per case to profiles/gine_bench.jsonl.  ``ops.FUSE_EDGE_ROWS`` ships True only if the fused median does not exceed the
unfused one at both cases.

  python tools/gine_bench.py [--scale 1.0] [--reps 11] [--warmup 3] [--out profiles/gine_bench.jsonl]
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
    from efficient_gnns_amd import _lib, ops, saint

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)                   # before the first load
    bench.cap_cpu_threads()
    assert torch.cuda.is_available(), "gine_bench needs a GPU"
    ops.FUSE_EDGE_ROWS = True                                       # the walk itself is measured, whatever the shipped switch says
    dev = torch.device("cuda", 0)

    def arxiv():
        d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=False)
        row, col, _ = PU.dgl_bidirected_with_self_loops(d.adj_t).coo()             # row = the target, col = the source of every message
        perm = torch.randperm(row.numel(), generator=torch.Generator().manual_seed(0))
        return d.num_nodes, col[perm], row[perm]

    def molhiv():
        b = saint.Batch.from_data_list(D.molhiv_like(512, seed=0))
        return b.num_nodes, b.edge_index[0], b.edge_index[1]

    for graph, C in (("arxiv", 256), ("molhiv_like_512", 300)):
        n, src, dst = arxiv() if graph == "arxiv" else molhiv()
        src, dst = src.to(dev).contiguous(), dst.to(dev).contiguous()
        plan_src, plan_dst = ops.rows_plan(src, n, check="deferred"), ops.rows_plan(dst, n, check="deferred")
        longest = int(torch.bincount(dst.cpu(), minlength=n).max())
        E = src.numel()
        g0 = torch.Generator().manual_seed(C)
        x = torch.randn(n, C, generator=g0).to(dev).requires_grad_(True)
        edge = torch.randn(E, C, generator=g0).to(dev).requires_grad_(True)
        gy = torch.randn(n, C, generator=g0).to(dev)
        wrt = [x, edge]

        def fused():
            out = ops.gather_add_scatter(x, plan_src, plan_dst, n, edge, "relu", "sum")
            return out, torch.autograd.grad(out, wrt, gy)

        def unfused():
            out = ops.scatter(torch.relu(ops.take_rows(x, plan_src) + edge), None, n, "sum", plan=plan_dst)
            return out, torch.autograd.grad(out, wrt, gy)

        def torch_form():
            out = torch.zeros(n, C, device=dev).index_add_(0, dst, torch.relu(x.index_select(0, src) + edge))
            return out, torch.autograd.grad(out, wrt, gy)

        forms = {"fused": fused, "unfused": unfused, "torch": torch_form}
        ref_out, ref_g = unfused()
        diffs, peaks = {}, {}
        for name, fn in forms.items():
            out, gs = fn()
            diffs[name] = [float((out - ref_out).detach().abs().max())] + [float((a - b).abs().max()) for a, b in zip(gs, ref_g)]
            del out, gs
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            fn()
            torch.cuda.synchronize()
            peaks[name] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        out, gs = fused()
        bit_equal = bool(torch.equal(out, ref_out) and torch.equal(gs[0], ref_g[0]) and torch.equal(gs[1], ref_g[1]))
        del out, gs, ref_out, ref_g
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
        res = {"what": "gather_add_scatter_fwd_bwd", "graph": graph, "scale": args.scale if graph == "arxiv" else 1.0, "nodes": n, "edges": E,
               "longest_run": longest, "C": C, "act": "relu", "reps": args.reps, "warmup": args.warmup,
               "fused_bit_equal_out_dx_dedge": bit_equal, "rows_oob": ops.rows_oob(dev)}
        print(f"{graph}: {E} edges, {n} nodes (longest run {longest}), C = {C}; fused == unfused bits: {bit_equal}")
        print(f"{'form':<10}{'median ms':>12}{'min ms':>10}{'peak MiB':>12}   max |out, dx, dedge - unfused|")
        for name in forms:
            med, lo = statistics.median(times[name]), min(times[name])
            res[name + "_ms"], res[name + "_min_ms"], res[name + "_peak_mib"] = round(med, 3), round(lo, 3), round(peaks[name], 1)
            res[name + "_max_abs_diff"] = [float(f"{v:.3e}") for v in diffs[name]]
            print(f"{name:<10}{med:>12.3f}{lo:>10.3f}{peaks[name]:>12.1f}   " + ", ".join(f"{v:.3e}" for v in diffs[name]))
        print(json.dumps(res))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(res) + "\n")
        del x, gy, edge, wrt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the arxiv graph's size (1.0: 169 343 nodes)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gine_bench.jsonl"), help="the jsonl file to append to ('' for none)")
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    main(ap.parse_args())
