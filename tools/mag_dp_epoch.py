#!/usr/bin/env python3
"""Full-size timings of the summing row step and the accumulating MAG epoch on ONE MI355X (tools only; numbers go to profiles/ and
DESIGN.md 6c).  mag_hetero_like(--mag-scale), GraphSAINT batch 20 000, walk length 2, supervised student R-GCN 2 x 64.

  step    egnn_adam_rows_step_sum_f32 against egnn_adam_rows_step_f32 on the rows of ONE real batch (unique rows: both kernels do the
          same Adam work; the difference is the key build and the radix sort), per table launch set as ``LazyRowAdam`` issues them --
          one call per embedding table over the whole batch list -- HIP events, median of --reps after --warmup; and the summing step on
          the concatenated rows of 2, 4 and 8 batches (what a data-parallel step of that many ranks applies).
  epoch   ``mag_accumulate_epoch`` over --epoch-steps batches with accumulate in {1, 2, 4} (accumulate = 1 under the default optimiser:
          the plain loop of this commit), wall clock including the end-of-epoch flush, --epoch-reps consecutive epochs per case.
  bytes   what a data-parallel step gathers for W in {2, 4, 8}: sum(n_r) * (4 D + 16) from real batch sizes, next to the dense table
          gradients an all-reduce would move.

``--baseline --package-root CHECKOUT`` times only what a checkout without the summing step has -- egnn_adam_rows_step_f32 on the
same batch and the plain ``mag_train_epoch`` under ``mag_optimizer(model, lr)`` -- with that checkout's package and library: the
figures of the commit before, for the comparison.

Multi-GPU throughput is not measured here: it cannot be on a one-GPU box.  One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--mag-scale", type=float, default=1.0)
ap.add_argument("--batch-size", type=int, default=20_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--epoch-steps", type=int, default=30)
ap.add_argument("--epoch-reps", type=int, default=5, help="timed epochs per case (median and minimum are reported)")
ap.add_argument("--out", default=None, help="also write the result lines to this file")
ap.add_argument("--baseline", action="store_true", help="only the plain step and the plain epoch (what a checkout without the summing step has)")
ap.add_argument("--package-root", default=None, help="import the package (and its built library) from this checkout instead of this one")
args = ap.parse_args()
ROOT = os.path.abspath(args.package_root) if args.package_root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (cap_cpu_threads)
import efficient_gnns_amd.data as D  # noqa: E402
import efficient_gnns_amd.models as PM  # noqa: E402
import efficient_gnns_amd.utils as PU  # noqa: E402
from efficient_gnns_amd import _lib  # noqa: E402
from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler  # noqa: E402

bench.cap_cpu_threads()
if not torch.cuda.is_available():
    sys.exit("mag_dp_epoch.py measures on the GPU only")
dev = torch.device("cuda", 0)
lines = []


def emit(res):
    lines.append(res)
    print(json.dumps(res), flush=True)


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
hp = dict(alpha=0.9, kd_T=4.0)
LR, DIM = 0.005, 128


def new_model():
    torch.manual_seed(0)
    return PM.RGCN(DIM, 64, d.num_classes, 2, 0.5, nn_dict, list(x_dict), len(eid)).to(dev)


# ---- step: the two kernels on the rows of real batches --------------------------------------------------------------------------
model = new_model()
opt = PM.mag_optimizer(model, LR) if args.baseline else PM.mag_optimizer(model, LR, duplicates="sum")
batches = list(GraphSAINTRandomWalkSampler(homo, batch_size=args.batch_size, walk_length=2, num_steps=8, seed=1))
tables = [(int(k), emb._egnn_rows) for k, emb in model.emb_dict.items()]
dense_table_bytes = sum(st.param.numel() * 4 for _, st in tables)
lib = _lib.load()


def timed_steps(n_batches, summing):
    """Median ms of one step of ALL tables over the concatenated rows of ``n_batches`` batches.  Every repetition advances the step
    (the rows are caught up first, outside the timed region), so each timed call does the full Adam work."""
    nt = torch.cat([b.node_type for b in batches[:n_batches]])
    li = torch.cat([b.local_node_idx for b in batches[:n_batches]])
    g = 0.01 * torch.randn(nt.numel(), DIM, device=dev)
    ws = {k: torch.empty(lib.egnn_adam_rows_step_sum_ws_bytes(nt.numel(), st.param.shape[0]) if summing else 0, dtype=torch.uint8, device=dev)
          for k, st in tables}
    ms = []
    for i in range(args.reps + args.warmup):
        for k, st in tables:
            st.catch_up(k, nt, li)
            st.t += 1
            st.ring.fill(st.t, LR)
            if st.t - st.flushed >= 60:
                st._flush_to(st.t - 1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for k, st in tables:
            desc = ctypes.byref(st._desc(st.t))
            if summing:
                _lib.check(lib.egnn_adam_rows_step_sum_f32(desc, k, nt.data_ptr(), li.data_ptr(), nt.numel(), g.data_ptr(), DIM, 1.0 / n_batches,
                                                           ws[k].data_ptr(), ws[k].numel(), _lib.stream()), "sum step")
            else:
                _lib.check(lib.egnn_adam_rows_step_f32(desc, k, nt.data_ptr(), li.data_ptr(), nt.numel(), g.data_ptr(), DIM, _lib.stream()), "step")
        b.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append(a.elapsed_time(b))
    refused = sum(int(st.dup.item()) for _, st in tables)
    for _, st in tables:
        st.dup.zero_()
    table_rows = int(sum(int((nt == k).sum()) for k, _ in tables))
    return dict(entries=int(nt.numel()), table_entries=table_rows, ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
                refused_rows=refused, workspace_bytes_per_table=[int(w.numel()) for w in ws.values()])


emit(dict(what="adam_rows_step", kernel="egnn_adam_rows_step_f32", baseline=args.baseline, batches=1, **timed_steps(1, False)))
for nb in (() if args.baseline else (1, 2, 4, 8)):
    emit(dict(what="adam_rows_step", kernel="egnn_adam_rows_step_sum_f32", batches=nb, **timed_steps(nb, True)))

# ---- bytes: what a data-parallel step gathers -----------------------------------------------------------------------------------
sizes = [int(b.node_type.numel()) for b in batches]
for W in (() if args.baseline else (2, 4, 8)):
    emit(dict(what="dp_gather_bytes", world=W, rows=sizes[:W], gathered_bytes=sum(sizes[:W]) * (4 * DIM + 16),
              dense_all_reduce_bytes=dense_table_bytes))
opt.close()
del model, opt, batches, tables
torch.cuda.empty_cache()

# ---- epoch: accumulate in {1, 2, 4} -------------------------------------------------------------------------------------------
def epoch(model, loader, opt, k):
    if args.baseline:
        return PM.mag_train_epoch(model, loader, x_dict, opt, "supervised", hp)
    return PM.mag_accumulate_epoch(model, loader, x_dict, opt, "supervised", hp, accumulate=k)


for k, duplicates in (((1, "refuse"),) if args.baseline else ((1, "refuse"), (1, "sum"), (2, "sum"), (4, "sum"))):
    model = new_model()
    opt = PM.mag_optimizer(model, LR) if args.baseline else PM.mag_optimizer(model, LR, duplicates=duplicates)
    warm = GraphSAINTRandomWalkSampler(homo, batch_size=args.batch_size, walk_length=2, num_steps=4, seed=3)
    epoch(model, warm, opt, k)
    loader = GraphSAINTRandomWalkSampler(homo, batch_size=args.batch_size, walk_length=2, num_steps=args.epoch_steps, seed=2)
    ms, losses = [], []
    for _ in range(args.epoch_reps):                     # consecutive epochs of one run: the sampler's stream and the training go on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses.append(epoch(model, loader, opt, k)[0])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    emit(dict(what="mag_epoch", baseline=args.baseline, accumulate=k, duplicates=duplicates, batches=args.epoch_steps, optimiser_steps=-(-args.epoch_steps // k),
              epochs=args.epoch_reps, epoch_train_ms=round(statistics.median(ms), 1), epoch_train_ms_min=round(min(ms), 1),
              epoch_train_ms_all=[round(v, 1) for v in ms], first_loss=round(losses[0], 5)))
    opt.close()
    del model, opt, loader, warm
    torch.cuda.empty_cache()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
