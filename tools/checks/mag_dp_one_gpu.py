"""The data-parallel MAG epoch (efficient-gnns_amd/dist.py: mag_dp_train_epoch) with world_size > 1 ON THE REAL HIP KERNELS, on a
one-GPU box: W processes share ``cuda:0`` and ``hostcomm`` carries the collectives over gloo (RCCL refuses two ranks on one device).

Problem: ``mag_hetero_like(0.01, seed=2)``, RGCN 2 x 16, 6 GraphSAINT batches from the rank-sliced sampler (W = 4 leaves a partial last
round), dropout seeded per batch (``seed=1``).  Per mode (supervised, kd, nce) every rank runs one epoch under
``LazyRowAdam(duplicates="sum")`` inside a ``CommTrace``; checksums of the dense parameters, the tables and their m / v / last are
exchanged; rank 0 compares with two single-process dense-Adam runs (fused, single-tensor) of ``mag_accumulate_epoch(accumulate=W, seed=1)``
over the same stream (bound: 4 x their spread + one ulp of max |p|), checks that a table row was named by two ranks in one round, and
that the table-gradient payload per step is sum(n_r) * (4 D + 16) bytes.

    python tools/checks/mag_dp_one_gpu.py --world 2 --out /tmp/mag_dp_w2.json
    python tools/checks/mag_dp_one_gpu.py --world 1 --backend nccl --out /tmp/mag_dp_rccl1.json

With ``--backend nccl --world 1`` the whole path (gather included) runs over RCCL with one rank and must equal
``mag_accumulate_epoch(accumulate=1, seed=1)`` under the default optimiser bit for bit.  Exit code 0 and the line MAG-DP-OK when every mode
is inside its bars.  Used by tests/test_gpu_mag_dp_multirank.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

MODES = ("supervised", "kd", "nce")
N_BATCHES, LR, SEED = 6, 0.005, 1
HP = dict(alpha=0.9, kd_T=4.0, beta=0.5, nce_T=0.075, max_samples=8192)      # max_samples > train rows of a batch: no host draw


def _problem(dev):
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.utils as PU
    from efficient_gnns_amd.saint import Data
    d = D.mag_hetero_like(0.01, seed=2)
    eid = dict(d.edge_index_dict)
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
    homo.y[l2g["paper"]] = d.y_dict["paper"]
    homo.train_mask = torch.zeros(N, dtype=torch.bool)
    homo.train_mask[l2g["paper"][d.split_idx["train"]["paper"]]] = True
    x_dict = {key2int["paper"]: d.x_dict["paper"].to(dev)}
    nn_dict = {key2int[k]: n for k, n in d.num_nodes_dict.items()}
    return d, homo.to(dev), len(eid), x_dict, nn_dict, key2int["paper"]


def _sampler(homo, rank, world):
    from efficient_gnns_amd.saint import GraphSAINTRandomWalkSampler
    return GraphSAINTRandomWalkSampler(homo, batch_size=200, walk_length=2, num_steps=N_BATCHES, sample_coverage=0, save_dir=None, seed=7,
                                       rank=rank, world=world)


def _build(mode, d, n_rel, x_dict, nn_dict, dev):
    """Identically initialised on every call: (student, teacher, student_proj, teacher_proj, all trainable parameters)."""
    import efficient_gnns_amd.models as PM
    torch.manual_seed(0)
    model = PM.RGCN(128, 16, d.num_classes, 2, 0.5, nn_dict, list(x_dict.keys()), n_rel).to(dev)
    teacher = sp = tp = None
    if mode != "supervised":
        teacher = PM.RGCN(128, 32, d.num_classes, 2, 0.5, nn_dict, list(x_dict.keys()), n_rel).to(dev)
        for p in teacher.parameters():
            p.requires_grad_(False)
    params = list(model.parameters())
    if mode == "nce":
        sp, tp = PM.make_projection(16, 8).to(dev), PM.make_projection(32, 8).to(dev)
        params += list(sp.parameters()) + list(tp.parameters())
    return model, teacher, sp, tp, params


def _checksums(tensors):
    """Two int64 sums over the raw 32-bit words of every tensor (plain and position-weighted): equal bits <=> equal sums, in practice."""
    out = []
    for t in tensors:
        w = t.detach().contiguous().view(-1).view(torch.int32).to(torch.int64)
        pos = torch.arange(w.numel(), device=w.device) % 1000003 + 1
        out.append((int(w.sum()), int((w * pos).sum())))
    return out


def _state(model, params):
    tensors = list(params)
    for emb in model.emb_dict.values():
        st = emb._egnn_rows
        tensors += [st.m, st.v, st.last]
    return tensors


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _reference(mode, world, d, homo, n_rel, x_dict, nn_dict, dev):
    """Rank 0: dense Adam, fused and single-tensor, over the same stream with ``accumulate=world``."""
    import efficient_gnns_amd.models as PM
    out = []
    for kw in ({"fused": True}, {"foreach": False}):
        model, teacher, sp, tp, params = _build(mode, d, n_rel, x_dict, nn_dict, dev)
        opt = torch.optim.Adam(params, lr=LR, **kw)
        loss = PM.mag_accumulate_epoch(model, _sampler(homo, 0, 1), x_dict, opt, mode, HP, teacher, sp, tp, accumulate=world, seed=SEED)
        out.append(([p.detach().double() for p in params], loss))
    return out


def _stream_facts(homo, paper, emb_dim):
    """From the world-1 stream: rows per batch, and per candidate world whether two batches of one round share a table row."""
    batches = list(_sampler(homo, 0, 1))
    rows = [int(b.node_type.numel()) for b in batches]
    keys = [set(zip(b.node_type.tolist(), b.local_node_idx.tolist())) for b in batches]
    keys = [{k for k in ks if k[0] != paper} for ks in keys]
    return rows, keys


def _worker(rank, world, port, backend, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)                      # every rank on the ONE device
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    ok = True
    try:
        import efficient_gnns_amd.dist as DD
        import efficient_gnns_amd.models as PM
        from efficient_gnns_amd import hostcomm
        from efficient_gnns_amd.optim import LazyRowAdam
        if backend == "gloo":
            hostcomm.install()
        d, homo, n_rel, x_dict, nn_dict, paper = _problem(dev)
        rows, keys = _stream_facts(homo, paper, 128)
        report = {}
        for mode in MODES:
            model, teacher, sp, tp, params = _build(mode, d, n_rel, x_dict, nn_dict, dev)
            opt = LazyRowAdam(params, lr=LR, lazy=list(model.emb_dict.values()), duplicates="sum")
            loader = _sampler(homo, rank, world)
            with DD.CommTrace() as trace:
                losses = DD.mag_dp_train_epoch(model, loader, x_dict, opt, mode, HP, teacher, sp, tp, seed=SEED)
            torch.cuda.synchronize()
            stats = dict(DD.LAST_DP_STATS)
            assert all(emb.grad is None for emb in model.emb_dict.values())
            gathered = [None] * world
            dist.all_gather_object(gathered, (_checksums(_state(model, params)), trace.records, list(losses), stats))
            if rank != 0:
                dist.barrier()                    # rank 0 runs the references meanwhile
                continue
            entry = dict(mode=mode, world=world, backend=backend, losses=list(losses), rows_per_batch=rows)
            entry["replicas_identical"] = all(g[0] == gathered[0][0] for g in gathered)
            entry["losses_identical"] = all(g[2] == gathered[0][2] for g in gathered)
            entry["collectives_mismatch"] = DD.consistent_collectives([g[1] for g in gathered])
            rounds = [list(range(f, min(f + world, N_BATCHES))) for f in range(0, N_BATCHES, world)]
            entry["rounds"] = rounds
            entry["partial_last_round"] = len(rounds[-1]) < world
            want_rows = [[rows[b] for b in rd] + [0] * (world - len(rd)) for rd in rounds]
            entry["rows_gathered"], entry["rows_expected"] = stats["rows"], want_rows
            entry["payload_bytes"] = stats["payload_bytes"]
            entry["payload_expected"] = [sum(r) * (4 * 128 + 16) for r in want_rows]
            # what the trace saw: per round one size gather and two padded row gathers of world * max(n_r) rows
            gat = [r for r in trace.records if r[0] == "all_gather_into_tensor"]
            entry["gathers_traced"] = len(gat)
            entry["gather_bytes_traced"] = [sum(r[2] for r in gat[3 * i:3 * i + 3]) for i in range(len(rounds))]
            entry["gather_bytes_padded_expected"] = [world * 8 + world * max(r) * (4 * 128 + 16) for r in want_rows]
            entry["shared_rows_per_round"] = [max((len(keys[a] & keys[b]) for a in rd for b in rd if a < b), default=0) for rd in rounds]
            if backend == "nccl" and world == 1:
                ref_model, ref_teacher, ref_sp, ref_tp, ref_params = _build(mode, d, n_rel, x_dict, nn_dict, dev)
                ref_opt = LazyRowAdam(ref_params, lr=LR, lazy=list(ref_model.emb_dict.values()))
                ref_loss = PM.mag_accumulate_epoch(ref_model, _sampler(homo, 0, 1), x_dict, ref_opt, mode, HP, ref_teacher, ref_sp, ref_tp,
                                                   accumulate=1, seed=SEED)
                entry["equals_single_process_bitwise"] = _checksums(_state(ref_model, ref_params)) == gathered[0][0]
                entry["ref_losses"] = list(ref_loss)
                entry["ok"] = bool(entry["equals_single_process_bitwise"] and entry["collectives_mismatch"] is None
                                   and entry["payload_bytes"] == entry["payload_expected"])
            else:
                (pa, loss_a), (pb, loss_b) = _reference(mode, world, d, homo, n_rel, x_dict, nn_dict, dev)
                got = [p.detach().double() for p in params]
                spread = max(float((a - b).abs().max()) for a, b in zip(pa, pb))
                errs, bounds = [], []
                for g, a, b in zip(got, pa, pb):
                    errs.append(max(float((g - a).abs().max()), float((g - b).abs().max())))
                    bounds.append(4 * spread + _ulp(float(a.abs().max())))
                worst = max(range(len(errs)), key=lambda i: errs[i] / bounds[i])
                entry.update(spread=spread, worst_err=errs[worst], worst_bound=bounds[worst], ref_losses=[list(loss_a), list(loss_b)],
                             within_bound=all(e <= b for e, b in zip(errs, bounds)))
                entry["ok"] = bool(entry["replicas_identical"] and entry["losses_identical"] and entry["collectives_mismatch"] is None
                                   and entry["within_bound"] and entry["rows_gathered"] == want_rows
                                   and entry["payload_bytes"] == entry["payload_expected"]
                                   and entry["gather_bytes_traced"] == entry["gather_bytes_padded_expected"]
                                   and max(entry["shared_rows_per_round"]) > 0)
            report[mode] = entry
            with open(out_path, "w") as f:
                json.dump(report, f, indent=1)
            print(f"[mag dp w={world} {backend}] {mode}: ok={entry['ok']} " +
                  " ".join(f"{k}={entry[k]}" for k in ("replicas_identical", "worst_err", "worst_bound", "spread", "shared_rows_per_round",
                                                       "payload_bytes", "equals_single_process_bitwise") if k in entry), flush=True)
            dist.barrier()
        if rank == 0:
            ok = all(e["ok"] for e in report.values()) and len(report) == len(MODES)
    except BaseException:
        import traceback
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
    try:
        dist.barrier()
        dist.destroy_process_group()
    finally:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0 if ok else 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--backend", default="gloo", choices=("gloo", "nccl"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.backend == "nccl" and args.world != 1:
        sys.exit("RCCL refuses two ranks on one device: --backend nccl needs --world 1")
    if not 1 <= args.world <= 8:
        sys.exit("--world must be 1..8 (every rank opens the one GPU)")
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, args.world, port, args.backend, args.out)) for r in range(args.world)]
    for p in procs:
        p.start()
    import time
    codes, deadline = [], time.monotonic() + 150                   # the whole run takes ~30 s; one limit for all ranks together
    for p in procs:
        p.join(max(0.0, deadline - time.monotonic()))
        codes.append(p.exitcode)
    for p in procs:
        if p.is_alive():
            p.kill()
    if any(c != 0 for c in codes):
        print(f"MAG-DP-FAILED exit codes {codes}")
        sys.exit(1)
    print("MAG-DP-OK")


if __name__ == "__main__":
    main()
