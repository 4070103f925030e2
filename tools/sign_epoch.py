#!/usr/bin/env python3
"""Seconds per SIGN training epoch and per ``sign_test`` at the reference's shape (arxiv_dgl/sign.py defaults: R = 5, hidden 512,
ff_layer 2, dropout 0.5, input dropout 0.1, batches of 50 000 / 100 000) on ``data.arxiv_like``, for the package (``models.SIGN`` on
the HIP kernels) and -- on the same GPU, in the same process, alternating -- for the same model written with plain ``torch.nn``
modules, which is what a user has without the package.  ``kernels`` times each of the three csrc/sign.hip entry points against the
ATen sequence it replaces (HIP events).

The parent process never opens the GPU: it starts one child per measurement (``--only`` picks some), each under its own time limit,
and stops at the first child that fails.  Every child prints one JSON line.

  python tools/sign_epoch.py [--only kernels,supervised,kd,nce] [--scale 1.0] [--reps 5] [--warmup 2] [--limit 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("supervised", "kd", "nce")
HP = dict(alpha=0.9, kd_T=4.0, beta=0.5, nce_T=0.075, max_samples=8192, kernel="rbf")
R, HIDDEN, FF, P_DROP, P_IN, BATCH, EVAL_BATCH, PROJ = 5, 512, 2, 0.5, 0.1, 50_000, 100_000, 256


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}


def parent(args):
    for what in args.only.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--scale", str(args.scale), "--reps", str(args.reps),
               "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"[sign_epoch] {what}: no result within {args.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"[sign_epoch] {what}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


def child(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from torch import nn

    sys.path.insert(0, ROOT)
    import bench  # noqa: E402  (cap_cpu_threads)
    import efficient_gnns_amd.data as D
    import efficient_gnns_amd.models as PM
    from efficient_gnns_amd import ops
    from efficient_gnns_amd.transforms import neighbor_average_features

    bench.cap_cpu_threads()
    assert torch.cuda.is_available(), "sign_epoch needs a GPU"
    dev = torch.device("cuda", 0)
    H = R + 1

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if args.child == "kernels":
        B = max(64, int(BATCH * args.scale))
        n = max(B, int(169_343 * args.scale))
        g = torch.Generator().manual_seed(0)
        feats = [torch.randn(n, 128, generator=g).to(dev) for _ in range(H)]
        batch = torch.randperm(n, generator=g)[:B].to(dev)
        z = torch.randn(B, H * HIDDEN, generator=g).to(dev)
        dy = torch.randn(B, H * HIDDEN, generator=g).to(dev)
        slopes = [torch.full((1,), 0.25, device=dev, requires_grad=True) for _ in range(H)]

        def aten_gather():
            return torch.cat([F.dropout(x[batch], P_IN, True) for x in feats], dim=1)

        def aten_prelu(zz):
            return torch.cat([F.dropout(F.prelu(zz[:, h * HIDDEN:(h + 1) * HIDDEN], slopes[h]), P_DROP, True) for h in range(H)], dim=1)

        def run_bwd(fwd, colsum_pass):
            zz = z.detach().requires_grad_(True)
            y = fwd(zz)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            y.backward(dy)
            if colsum_pass:
                zz.grad.sum(0)                                    # the bias gradient of the producing Linear: a second pass in ATen
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        def run_ev(fn):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            with torch.no_grad():
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        hip_prelu = lambda zz: ops.prelu_drop(zz, slopes, HIDDEN, P_DROP, True)   # noqa: E731
        pairs = {"gather_drop": (lambda: run_ev(lambda: ops.sign_gather_drop(feats, batch, P_IN, True)), lambda: run_ev(aten_gather)),
                 "prelu_drop_fwd": (lambda: run_ev(lambda: hip_prelu(z)), lambda: run_ev(lambda: aten_prelu(z))),
                 "prelu_drop_bwd": (lambda: run_bwd(hip_prelu, False), lambda: run_bwd(aten_prelu, True))}
        res = {"what": "kernels", "B": B, "H": H, "F": 128, "hidden": HIDDEN, "unit": "ms", "reps": 4 * args.reps}
        for name, (hip, aten) in pairs.items():
            for _ in range(3):
                hip(), aten()
            th, ta = [], []
            for _ in range(4 * args.reps):                        # alternating
                th.append(hip())
                ta.append(aten())
            res[name] = {"hip": stats(th), "aten": stats(ta), "aten_over_hip": round(statistics.median(ta) / statistics.median(th), 3)}
        print(json.dumps(res), flush=True)
        return 0

    mode = args.child
    if mode not in MODES:
        raise SystemExit(f"unknown measurement '{mode}'")
    d = D.arxiv_like(scale=args.scale, seed=0, with_teacher=True)
    with torch.no_grad():
        feats = neighbor_average_features(d.adj_t.to(dev), d.x.to(dev), R)
    labels = d.y.view(-1).to(dev)
    tof, tl = ops.pad_pitch(d.teacher_out_feat.to(dev)), d.teacher_logits.to(dev)
    train_nid, val_nid, test_nid = (d.split_idx[k].to(dev) for k in ("train", "valid", "test"))
    n, C = d.num_nodes, d.num_classes
    bs, ebs = max(64, int(BATCH * args.scale)), max(64, int(EVAL_BATCH * args.scale))

    class TorchFF(nn.Module):
        """The feed-forward block with torch.nn modules only."""

        def __init__(self, i, h, o, L, p):
            super().__init__()
            dims = [i] + [h] * (L - 1) + [o]
            self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))
            self.prelu, self.dropout = nn.PReLU(), nn.Dropout(p)

        def forward(self, x):
            for k, lin in enumerate(self.layers):
                x = lin(x)
                if k < len(self.layers) - 1:
                    x = self.dropout(self.prelu(x))
            return x

    class TorchSIGN(nn.Module):
        def __init__(self):
            super().__init__()
            self.dropout, self.prelu, self.input_drop = nn.Dropout(P_DROP), nn.PReLU(), nn.Dropout(P_IN)
            self.inception_ffs = nn.ModuleList(TorchFF(128, HIDDEN, HIDDEN, FF, P_DROP) for _ in range(H))
            self.project = TorchFF(H * HIDDEN, HIDDEN, C, FF, P_DROP)

        def forward(self, xs):
            hs = [ff(self.input_drop(x)) for x, ff in zip(xs, self.inception_ffs)]
            self.out_feat = self.dropout(self.prelu(torch.cat(hs, dim=-1)))
            return self.project(self.out_feat)

    def torch_epoch(model, opt, batches, sp, tp):
        model.train()
        for batch in batches:
            logits = model([x[batch] for x in feats])
            y = labels[batch]
            if mode == "supervised":
                loss = F.cross_entropy(logits, y)
            else:
                T = HP["kd_T"]
                kd = F.kl_div(F.log_softmax(logits / T, dim=1), F.softmax(tl[batch] / T, dim=1), reduction="mean")
                loss = kd * (HP["alpha"] * T * T) + F.cross_entropy(logits, y) * (1 - HP["alpha"])
                if mode == "nce":
                    f, t = sp(model.out_feat), tp(tof[batch])
                    pick = torch.from_numpy(np.random.choice(f.shape[0], HP["max_samples"], replace=False)).to(dev) \
                        if HP["max_samples"] < f.shape[0] else torch.arange(f.shape[0], device=dev)
                    f, t = F.normalize(f[pick], dim=-1), F.normalize(t[pick], dim=-1)
                    aux = F.cross_entropy(f @ t.t() / HP["nce_T"], torch.arange(f.shape[0], device=dev))
                    loss = loss + HP["beta"] * aux
            opt.zero_grad()
            loss.backward()
            opt.step()
        return float(loss)

    @torch.no_grad()
    def torch_test(model):
        model.eval()
        logits = torch.cat([model([x[i:i + ebs] for x in feats]) for i in range(0, n, ebs)], dim=0)
        pred = logits.argmax(-1)
        return [float((pred[i] == labels[i]).float().mean()) for i in (train_nid, val_nid, test_nid)]

    def build(kind):
        torch.manual_seed(0)
        model = (PM.SIGN(128, HIDDEN, C, H, FF, P_DROP, P_IN) if kind == "hip" else TorchSIGN()).to(dev)
        sp = tp = None
        groups = [{"params": model.parameters()}]
        if mode == "nce":
            if kind == "hip":
                sp, tp = PM.make_sign_projections(HIDDEN, H, PROJ)
            else:
                sp = nn.Sequential(nn.Linear(HIDDEN * H, PROJ), nn.BatchNorm1d(PROJ), nn.ReLU())
                tp = nn.Sequential(nn.Linear(750, PROJ), nn.BatchNorm1d(PROJ), nn.ReLU())
            sp, tp = sp.to(dev), tp.to(dev)
            groups += [{"params": sp.parameters()}, {"params": tp.parameters()}]
        return model, torch.optim.Adam(groups, lr=0.001), sp, tp

    def batches():
        perm = train_nid[torch.randperm(train_nid.numel(), device=dev)]
        return [perm[i:i + bs] for i in range(0, perm.numel(), bs)]

    hip, aten = build("hip"), build("aten")
    eval_batches = [range(i, min(i + ebs, n)) for i in range(0, n, ebs)]
    runs = {
        "epoch_hip": lambda: PM.sign_train_epoch(hip[0], feats, labels, hip[1], batches(), mode, HP, tof, tl, hip[2], hip[3]),
        "epoch_torch": lambda: torch_epoch(aten[0], aten[1], batches(), aten[2], aten[3]),
        "test_hip": lambda: PM.sign_test(hip[0], feats, labels, eval_batches, train_nid, val_nid, test_nid),
        "test_torch": lambda: torch_test(aten[0]),
    }
    times = {k: [] for k in runs}
    for i in range(args.warmup + args.reps):                      # alternating; the first `warmup` rounds are not kept
        for k, fn in runs.items():
            t = timed(fn)
            if i >= args.warmup:
                times[k].append(t)
    res = {"what": mode, "N": n, "train_rows": int(train_nid.numel()), "batch": bs, "eval_batch": ebs, "steps_per_epoch": len(batches()),
           "unit": "s", **{k: stats(v) for k, v in times.items()}}
    res["epoch_torch_over_hip"] = round(res["epoch_torch"]["median"] / res["epoch_hip"]["median"], 3)
    res["test_torch_over_hip"] = round(res["test_torch"]["median"] / res["test_hip"]["median"], 3)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="kernels," + ",".join(MODES))
    ap.add_argument("--child", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds each measurement may take")
    a = ap.parse_args()
    sys.exit(child(a) if a.child else parent(a))
