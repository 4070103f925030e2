#!/usr/bin/env python3
"""Milliseconds and peak memory of one weighted-sum message-passing layer -- lift, per-edge weight, aggregation -- forward + backward,
in three forms run on the same GPU in the same process over READY plans:

  fused        ``ops.gather_scatter(x, plan_src, plan_dst, n, w)`` (csrc/gather_scatter.hip): no [E, C] tensor
  unfused      the composition it replaces: ``ops.scatter(ops.take_rows(x, plan_src) * w, None, n, plan=plan_dst)``
  torch        torch ops only: ``index_select``, multiply, ``index_add_``, differentiated by autograd

Cases: the arxiv message graph (the ``data.arxiv_like`` graph, bidirected, one loop per node, the edges in a seeded random order)
at C = 256 with and without a weight and at C = 750 as 3 heads x 250 with softmax weights, and one GraphSAINT-batch-sized case
(38 155 nodes, 186 292 random edges, C = 128: DESIGN 3.5a's stage table).  The three forms get the same operands and upstream
gradient; outputs and gradients are compared before the timing (fused against unfused must be bit-equal except the weights'
gradient).  Warm-up rounds first, then alternating repeats timed with device events around forward + backward; median and minimum are
reported, and per form the peak allocated memory of one forward + backward above what the operands hold.  Prints a table and
appends one JSON line per case to profiles/gather_scatter_bench.jsonl.

  python tools/gather_scatter_bench.py [--scale 1.0] [--reps 11] [--warmup 3] [--out profiles/gather_scatter_bench.jsonl]
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
    assert torch.cuda.is_available(), "gather_scatter_bench needs a GPU"
    dev = torch.device("cuda", 0)

    def arxiv():
        d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=False)
        row, col, _ = PU.dgl_bidirected_with_self_loops(d.adj_t).coo()             # row = the target, col = the source of every message
        perm = torch.randperm(row.numel(), generator=torch.Generator().manual_seed(0))
        return d.num_nodes, col[perm], row[perm]

    def saint_batch():
        g = torch.Generator().manual_seed(1)
        n, E = 38155, 186292
        return n, torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)

    graphs = {}
    cases = [("arxiv", 256, 1, "none"), ("arxiv", 256, 1, "edge"), ("arxiv", 750, 3, "softmax"), ("saint_batch", 128, 1, "edge")]
    for graph, C, H, weights in cases:
        if graph not in graphs:
            n, src, dst = arxiv() if graph == "arxiv" else saint_batch()
            src, dst = src.to(dev).contiguous(), dst.to(dev).contiguous()
            graphs[graph] = (n, src, dst, ops.rows_plan(src, n, check="deferred"), ops.rows_plan(dst, n, check="deferred"),
                             int(torch.bincount(dst.cpu(), minlength=n).max()))
        n, src, dst, plan_src, plan_dst, longest = graphs[graph]
        E, Dh = src.numel(), C // H
        g0 = torch.Generator().manual_seed(C + H)
        x = torch.randn(n, C, generator=g0).to(dev).requires_grad_(True)
        gy = torch.randn(n, C, generator=g0).to(dev)
        w = None
        if weights == "edge":
            w = torch.rand(E, 1, generator=g0).to(dev).requires_grad_(True)
        elif weights == "softmax":
            with torch.no_grad():
                w = ops.scatter_softmax((3 * torch.randn(E, H, generator=g0)).to(dev), None, n, plan=plan_dst, eps=1e-16)
            w = w.requires_grad_(True)
        wrt = [x] if w is None else [x, w]

        def fused():
            out = ops.gather_scatter(x, plan_src, plan_dst, n, w, "sum")
            return out, torch.autograd.grad(out, wrt, gy)

        def unfused():
            msg = ops.take_rows(x, plan_src)
            if w is not None:
                msg = (msg.view(E, H, Dh) * w.view(E, H, 1)).view(E, C)
            out = ops.scatter(msg, None, n, "sum", plan=plan_dst)
            return out, torch.autograd.grad(out, wrt, gy)

        def torch_form():
            msg = x.index_select(0, src)
            if w is not None:
                msg = (msg.view(E, H, Dh) * w.view(E, H, 1)).view(E, C)
            out = torch.zeros(n, C, device=dev).index_add_(0, dst, msg)
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
        bit_equal = bool(torch.equal(out, ref_out) and torch.equal(gs[0], ref_g[0]))
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
        res = {"what": "gather_scatter_fwd_bwd", "graph": graph, "scale": args.scale if graph == "arxiv" else 1.0, "nodes": n, "edges": E,
               "longest_run": longest, "C": C, "H": H, "weights": weights, "reps": args.reps, "warmup": args.warmup,
               "fused_bit_equal_out_dx": bit_equal, "rows_oob": ops.rows_oob(dev)}
        print(f"{graph}: {E} edges, {n} nodes (longest run {longest}), C = {C}, H = {H}, weights = {weights}; fused == unfused bits: {bit_equal}")
        print(f"{'form':<10}{'median ms':>12}{'min ms':>10}{'peak MiB':>12}   max |out, dx, (dw) - unfused|")
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
        del x, gy, w, wrt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the arxiv graph's size (1.0: 169 343 nodes)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_scatter_bench.jsonl"), help="the jsonl file to append to ('' for none)")
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    main(ap.parse_args())
