#!/usr/bin/env python3
"""ms per training step of the arxiv GAT teacher (``models.ArxivGAT`` 3 layers x 250 x 3 heads, arxiv_dgl/gat.py:116-148 with the
script-of-record configuration of arxiv_dgl/scripts/gat-teachers.sh: --use-norm --use-labels --n-label-iters=1 --no-attn-dst
--edge-drop=0.3 --input-drop=0.25, RMSprop) on ``data.arxiv_like`` at full size, and -- in the same process, with HIP events -- the
fused layer forward (egnn_gat_layer_fwd_f32) next to the launch sequence the inference forward makes for the same layer
(ops_edge.gat_coefficients, the source scaling, the [N, H*250] -> [N, H*252] pad, ops_edge.gat_aggregate, the target scaling).
Prints one JSON line.

  --steps K      timed training steps (after --warmup W untimed ones)
  --scale S      graph size as a fraction of ogbn-arxiv (default 1.0: N = 169 343)
  --reps R       timed repetitions of each layer-forward variant (interleaved)
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (cap_cpu_threads)
import efficient_gnns_amd.data as D  # noqa: E402
import efficient_gnns_amd.models as PM  # noqa: E402
from efficient_gnns_amd import _lib, ops_edge  # noqa: E402
from efficient_gnns_amd.utils import dgl_bidirected_with_self_loops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
bench.cap_cpu_threads()
dev = torch.device("cuda", 0)

d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=False)
n, C = d.num_nodes, d.num_classes
adj = dgl_bidirected_with_self_loops(d.adj_t.to(dev))
x, y = d.x.to(dev), d.y.to(dev)
tr, va, te = (d.split_idx[k].to(dev) for k in ("train", "valid", "test"))
H, Fh = 3, 250


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


# ---- the training step
torch.manual_seed(0)
model = PM.ArxivGAT(d.num_features + C, C, Fh, 3, H, F.relu, dropout=0.75, input_drop=0.25, attn_drop=0.0, edge_drop=0.3,
                    use_attn_dst=False, use_symmetric_norm=True).to(dev)
opt = torch.optim.RMSprop(model.parameters(), lr=0.002, weight_decay=0)


def step(ev):
    """arxiv_gat_train_step with events between its phases: label-reuse forward | forward to the loss | backward + optimizer."""
    model.train()
    lab, pred_idx = PM.arxiv_gat_label_split(tr, 0.5)
    feat = PM.add_labels(x, y, lab, C)
    opt.zero_grad()
    ev[0].record()
    pred = model(adj, feat).detach()
    unl = torch.cat([pred_idx, va, te])
    feat[unl, -C:] = F.softmax(pred[unl], dim=-1)
    ev[1].record()
    loss = PM.arxiv_gat_loss(model(adj, feat)[pred_idx], y[pred_idx])
    ev[2].record()
    loss.backward()
    opt.step()
    ev[3].record()
    return loss


tot, fwd0, fwd1, bwd, losses = [], [], [], [], []
for k in range(args.warmup + args.steps):
    PM.arxiv_gat_adjust_learning_rate(opt, 0.002, k + 1)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    loss = step(ev)
    torch.cuda.synchronize()
    if k >= args.warmup:
        fwd0.append(ev[0].elapsed_time(ev[1])); fwd1.append(ev[1].elapsed_time(ev[2])); bwd.append(ev[2].elapsed_time(ev[3]))
        tot.append(ev[0].elapsed_time(ev[3]))
    losses.append(round(float(loss), 4))
train = {"ms_per_step": stats(tot), "label_reuse_fwd_ms": stats(fwd0), "fwd_ms": stats(fwd1), "bwd_step_ms": stats(bwd),
         "loss_first_last": [losses[0], losses[-1]], "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
del model, opt
torch.cuda.empty_cache()

# ---- one hidden layer's attention + aggregation: fused launch vs the inference forward's launch sequence
torch.manual_seed(1)
conv = PM.DGLGATConv(H * Fh, Fh, num_heads=H, use_attn_dst=False, use_symmetric_norm=True, residual=True).to(dev)
xl = torch.randn(n, H * Fh, device=dev)
in_sqrt, out_rsqrt, _ = conv._degrees(adj)
r, q = out_rsqrt.reshape(n).contiguous(), in_sqrt.reshape(n).contiguous()
attn_l = conv.attn_l.detach()
nnz = adj.nnz()
plain = adj.set_value(None) if adj.has_value() else adj
conv.edge_drop = 0.3
keep = conv._draw_edge_keep(nnz, dev).to(torch.uint8)
el = (ops_edge.gat_logits(xl, attn_l, None, H, Fh)[:, :H] * out_rsqrt).contiguous()
er = torch.zeros(n, H, device=dev)


def fused(keep_mask):
    import ctypes
    att = torch.empty(H, nnz, dtype=torch.float32, device=dev)
    out = torch.empty(n, H * Fh, dtype=torch.float32, device=dev)
    desc = ops_edge._gat_layer_desc(plain, False, n, nnz, H, Fh, xl, el, None, attn_l, None, keep_mask, None, r, q, 0.2)
    _lib.check(_lib.load().egnn_gat_layer_fwd_f32(ctypes.byref(desc), _lib.ptr(att), _lib.ptr(out), H * Fh, _lib.stream()), "fwd")
    return out.view(n, H, Fh)


def sequence():
    """nn.DGLGATConv.forward (eval) from the attention launch on: attention, scaled source copy, pad, H SpMMs, target scale."""
    att = ops_edge.gat_coefficients(adj, el, er, 0.2)
    src = xl * out_rsqrt
    Fp = (Fh + 3) // 4 * 4
    src_heads = F.pad(src.view(n, H, Fh), (0, Fp - Fh)).reshape(n, H * Fp)
    out = ops_edge.gat_aggregate(plain, att, src_heads, Fp)
    return out.view(n, H, Fp)[:, :, :Fh] * in_sqrt.view(n, 1, 1)


variants = {"fused_all_edges": lambda: fused(None), "sequence_all_edges": sequence, "fused_edge_drop_0.3": lambda: fused(keep)}
with torch.no_grad():
    a, b = fused(None), sequence()
    err = float((a - b).abs().max() / b.abs().max())
    for f in variants.values():                                     # warm-up: plans cached, kernels loaded
        f(); f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.reps):                                      # interleaved, so drift hits every variant alike
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
layer = {k: stats(v) for k, v in times.items()}
layer["fused_vs_sequence_max_rel_diff"] = err
res = {"workload": "arxiv_gat_teacher_train", "nodes": n, "nnz": nnz, "heads": H, "hidden": Fh, "steps": args.steps,
       "warmup": args.warmup, "train": train, "layer_forward_ms": layer, "reps": args.reps, "build": _lib.build_info()}
print(json.dumps(res), flush=True)
