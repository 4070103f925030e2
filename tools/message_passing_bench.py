#!/usr/bin/env python3
"""Milliseconds of ONE relational layer, forward + backward, on ONE MAG-shaped GraphSAINT batch (``data.mag_hetero_like`` grouped into
one graph, ``saint.GraphSAINTRandomWalkSampler``), run three ways on the same GPU in the same process:

  generic   a conv written in PyG's idiom on ``nn.MessagePassing``: per edge type ``propagate(edge_index[:, mask], x=x, edge_type=i)``
            with a bias-free Linear in ``message`` and mean aggregation, per node type a root Linear -- outside ``accel`` (gather,
            torch Linear over every message, ``ops.scatter``) and inside ``accel.scope()`` (gather-fused ``ops.linear_rows``)
  rgcn      ``nn.RGCNConv`` with the same weights: the algebraically reordered form (mean-SpMM, then one GEMM per edge type) over the
            batch's ready ``relations``
  torch     the same layer with torch ops only: ``index_select``, torch Linear, ``index_add_`` and a degree count per edge type

The generic forms build their plans per call (``ops.rows_plan(check="deferred")``: no host read); what they and the torch form pay
per step for the fresh ``edge_index[:, mask]`` tensors (a boolean mask and its ``nonzero`` per edge type) is inside the timed
region, as in a training loop.  Warm-up rounds first, then alternating repeats timed with device events; the median is reported.
The three outputs are compared before the timing (max abs difference, printed).  Prints a table and one JSON line.

``--stages`` (runs alone): the pieces of ONE propagate call on synthetic uniform endpoints (``--stage-nodes`` nodes, ``--stage-edges``
edges, targets among the first quarter of the nodes), each timed by itself with device events around the single call (so the host's
share of a call is inside the figure): the deferred plan build, ``take_rows`` / ``scatter`` / ``linear_rows`` forward and backward,
next to ``index_select`` / ``index_add_`` on the same tensors.

  python tools/message_passing_bench.py [--mag-scale 0.05] [--batch-size 20000] [--walk-length 2] [--in 128] [--out 64]
                                        [--reps 9] [--warmup 3]
  python tools/message_passing_bench.py --stages [--stage-nodes 38155] [--stage-edges 186292] [--in 128] [--out 64]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stages(args):
    import torch

    sys.path.insert(0, ROOT)
    from efficient_gnns_amd import ops

    assert torch.cuda.is_available(), "message_passing_bench needs a GPU"
    dev = torch.device("cuda", 0)
    n, E, C, Co = args.stage_nodes, args.stage_edges, args.c_in, args.c_out
    g = torch.Generator().manual_seed(0)
    src, dst = torch.randint(0, n, (E,), generator=g).to(dev), torch.randint(0, max(1, n // 4), (E,), generator=g).to(dev)
    x, w = torch.randn(n, C, device=dev, requires_grad=True), torch.randn(Co, C, device=dev)
    gout, gy = torch.randn(n, Co, device=dev), torch.randn(E, C, device=dev)
    m = torch.randn(E, Co, device=dev, requires_grad=True)

    def timed(fn, reps=20, warm=5):
        ts = []
        for i in range(reps + warm):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                ts.append(a.elapsed_time(b))
        return round(statistics.median(ts), 4)
    pj, pi = ops.rows_plan(src, n, check="deferred"), ops.rows_plan(dst, n, check="deferred")
    xj, mean = ops.take_rows(x, pj), ops.scatter(m, None, n, "mean", plan=pi)
    res = {"what": "message_passing_stages", "nodes": n, "edges": E, "c_in": C, "c_out": Co,
           "plan_deferred_ms": timed(lambda: ops.rows_plan(src, n, check="deferred")),
           "take_rows_fwd_ms": timed(lambda: ops.take_rows(x.detach(), pj)),
           "take_rows_bwd_ms": timed(lambda: torch.autograd.grad(xj, x, gy, retain_graph=True)),
           "scatter_mean_fwd_ms": timed(lambda: ops.scatter(m.detach(), None, n, "mean", plan=pi)),
           "scatter_max_fwd_ms": timed(lambda: ops.scatter(m.detach(), None, n, "max", plan=pi)),
           "scatter_mean_bwd_ms": timed(lambda: torch.autograd.grad(mean, m, gout, retain_graph=True)),
           "linear_rows_fwd_ms": timed(lambda: ops.linear_rows(x.detach(), pj, w)),
           "torch_index_select_ms": timed(lambda: x.detach().index_select(0, src)),
           "torch_index_add_messages_ms": timed(lambda: torch.zeros(n, Co, device=dev).index_add_(0, dst, m.detach())),
           "torch_index_add_gather_bwd_ms": timed(lambda: torch.zeros(n, C, device=dev).index_add_(0, src, gy)),
           "edge_mask_select_ms": timed(lambda: torch.stack([src, dst])[:, src > 100])}
    for k, v in res.items():
        print(f"{k:<34}{v}")
    print(json.dumps(res))


def main(args):
    import torch

    sys.path.insert(0, ROOT)
    import bench  # noqa: E402  (cap_cpu_threads)
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.utils as PU
    from efficient_gnns_amd import nn as PN
    from efficient_gnns_amd import ops
    from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler

    bench.cap_cpu_threads()
    assert torch.cuda.is_available(), "message_passing_bench needs a GPU"
    dev = torch.device("cuda", 0)
    spec = importlib.util.spec_from_file_location("egnn_dropin_accel_bench", os.path.join(ROOT, "efficient-gnns_amd", "dropin", "accel.py"))
    accel = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(accel)

    d = D.mag_hetero_like(scale=args.mag_scale, seed=0)
    eid = {k: v.to(dev) for k, v in d.edge_index_dict.items()}
    for key, rev in ((("author", "affiliated_with", "institution"), ("institution", "to", "author")),
                     (("author", "writes", "paper"), ("paper", "to", "author")),
                     (("paper", "has_topic", "field_of_study"), ("field_of_study", "to", "paper"))):
        r, c = eid[key]
        eid[rev] = torch.stack([c, r])
    eid[("paper", "cites", "paper")] = PU.to_undirected(eid[("paper", "cites", "paper")])
    edge_index, edge_type, node_type, local_idx, _, _ = PU.group_hetero_graph(eid, d.num_nodes_dict)
    N = node_type.numel()
    homo = Data(edge_index=edge_index, edge_attr=edge_type, node_type=node_type, local_node_idx=local_idx, num_nodes=N)
    T, NT = len(eid), len(d.num_nodes_dict)
    sampler = GraphSAINTRandomWalkSampler(homo, batch_size=args.batch_size, walk_length=args.walk_length, num_steps=1, seed=1,
                                          num_edge_types=T, num_node_types=NT)
    batch = next(iter(sampler))
    ei, et, nt = batch.edge_index, batch.edge_attr, batch.node_type
    n, E = int(batch.num_nodes), ei.shape[1]
    c_in, c_out = args.c_in, args.c_out

    class GenericConv(PN.MessagePassing):
        def __init__(self):
            super().__init__(aggr="mean")
            self.rel_lins = torch.nn.ModuleList(torch.nn.Linear(c_in, c_out, bias=False) for _ in range(T))
            self.root_lins = torch.nn.ModuleList(torch.nn.Linear(c_in, c_out, bias=True) for _ in range(NT))

        def forward(self, x, edge_index, edge_type, node_type):
            out = x.new_zeros(x.shape[0], c_out)
            for i in range(T):
                out = out + self.propagate(edge_index[:, edge_type == i], x=x, edge_type=i)
            for i, lin in enumerate(self.root_lins):
                rows = torch.nonzero(node_type == i).view(-1)
                out = out.index_add(0, rows, lin(x[rows]))
            return out

        def message(self, x_j, edge_type: int):
            return self.rel_lins[edge_type](x_j)

    class TorchConv(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.rel_lins = torch.nn.ModuleList(torch.nn.Linear(c_in, c_out, bias=False) for _ in range(T))
            self.root_lins = torch.nn.ModuleList(torch.nn.Linear(c_in, c_out, bias=True) for _ in range(NT))

        def forward(self, x, edge_index, edge_type, node_type):
            out = x.new_zeros(x.shape[0], c_out)
            for i in range(T):
                sel = edge_index[:, edge_type == i]
                msg = self.rel_lins[i](x.index_select(0, sel[0]))
                deg = torch.zeros(x.shape[0], device=x.device).index_add_(0, sel[1], torch.ones(sel.shape[1], device=x.device))
                out = out + torch.zeros_like(out).index_add_(0, sel[1], msg) / deg.clamp_min(1).view(-1, 1)
            for i, lin in enumerate(self.root_lins):
                rows = torch.nonzero(node_type == i).view(-1)
                out = out.index_add(0, rows, lin(x.index_select(0, rows)))
            return out

    torch.manual_seed(0)
    generic, rgcn, plain = GenericConv().to(dev), PN.RGCNConv(c_in, c_out, NT, T).to(dev), TorchConv().to(dev)
    rgcn.load_state_dict(generic.state_dict())
    plain.load_state_dict(generic.state_dict())
    x = torch.randn(n, c_in, device=dev, requires_grad=True)
    g = torch.randn(n, c_out, device=dev)

    def run(layer, **kw):
        out = layer(x, ei, et, nt, **kw)
        grads = torch.autograd.grad(out, [x] + [p for p in layer.parameters()], g, allow_unused=True)
        return out, grads[0]

    def run_accel():
        with accel.scope():
            return run(generic)
    forms = {"generic": lambda: run(generic), "generic_accel": run_accel, "rgcn": lambda: run(rgcn, relations=batch.relations),
             "torch": lambda: run(plain)}
    ref_out, ref_gx = forms["torch"]()
    diffs = {}
    for name, fn in forms.items():
        out, gx = fn()
        diffs[name] = (float((out - ref_out).detach().abs().max()), float((gx - ref_gx).abs().max()))
    scale = (float(ref_out.detach().abs().max()), float(ref_gx.abs().max()))
    oob = ops.rows_oob(dev)

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
    res = {"what": "message_passing_layer", "mag_scale": args.mag_scale, "batch_nodes": n, "batch_edges": E, "edge_types": T, "node_types": NT,
           "edges_per_type": [int((et == i).sum()) for i in range(T)], "c_in": c_in, "c_out": c_out, "reps": args.reps, "warmup": args.warmup,
           "rows_oob": oob}
    print(f"one relational layer, forward + backward: {n} nodes, {E} edges, {T} edge types, {c_in} -> {c_out}")
    print(f"{'form':<16}{'median ms':>12}{'min ms':>10}{'max |out - torch|':>22}{'max |dx - torch|':>20}")
    for name in forms:
        med, lo = statistics.median(times[name]), min(times[name])
        res[name + "_ms"], res[name + "_min_ms"] = round(med, 3), round(lo, 3)
        res[name + "_max_abs_diff"] = [float(f"{v:.3e}") for v in diffs[name]]
        print(f"{name:<16}{med:>12.3f}{lo:>10.3f}{diffs[name][0]:>22.3e}{diffs[name][1]:>20.3e}")
    print(f"(max |out| = {scale[0]:.3f}, max |dx| = {scale[1]:.3f})")
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mag-scale", type=float, default=0.05)
    ap.add_argument("--batch-size", type=int, default=20_000)
    ap.add_argument("--walk-length", type=int, default=2)
    ap.add_argument("--in", dest="c_in", type=int, default=128)
    ap.add_argument("--out", dest="c_out", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stages", action="store_true", help="time the pieces of one propagate call on synthetic endpoints only")
    ap.add_argument("--stage-nodes", type=int, default=38_155)
    ap.add_argument("--stage-edges", type=int, default=186_292)
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    a = ap.parse_args()
    if a.lib:                                                        # before the first load
        sys.path.insert(0, ROOT)
        importlib.import_module("efficient_gnns_amd._lib").LIB_PATH = os.path.abspath(a.lib)
    stages(a) if a.stages else main(a)
