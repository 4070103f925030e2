#!/usr/bin/env python3
"""Milliseconds and peak device bytes of the three structure-preservation metrics (efficient-gnns_amd/similarity.py) at the arxiv
validation shape of arxiv_pyg/correlation.py -- N = 29 799 rows, student width 256, teacher width 750, a synthetic symmetric edge
list -- and, on the same GPU in the same process, of the torch-op form a user has without the package:

  global   F.normalize, two torch.mm (two N x N Grams), triu selection, torch.corrcoef
  local    F.normalize, F.cosine_similarity over the gathered edge rows, torch.corrcoef

  kcka     F.normalize, torch.mm, the distance matrix, its median over the upper triangle, torch.exp, centring by row / column
           means, three sums -- at ``--kcka-torch-n`` rows (default 8 192), a size the N x N form still fits; the package is timed at
           that size too and, alone, at N

(linear CKA has no torch-op column: the reference's n x n centring is O(n^3) and is not what anyone would run at this N.)
Everything a form allocates inside its call is counted in its time and its peak: for the torch-op global form that is the N x N bool
mask of the ``triu`` selection (0.9 GB) next to the two Grams, their ``1 - ...`` copies and the two selected vectors.
After the timing, both global values are compared with a float64 value formed on the device in row chunks (untimed): at 444 M pairs
``torch.corrcoef``'s fp32 reductions are themselves a source of error.
Warm-up rounds first, then alternating repeats timed with device events; peak bytes are ``torch.cuda.max_memory_allocated`` above
what was allocated when the call began.  Prints a table and one JSON line.

  python tools/similarity_bench.py [--n 29799] [--ds 256] [--dt 750] [--degree 8] [--reps 5] [--warmup 2]
                                   [--metrics global,local,cka,kcka] [--kcka-torch-n 8192] [--lib PATH/libegnn_hip.so]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(args):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    import bench  # noqa: E402  (cap_cpu_threads)
    import efficient_gnns_amd as E

    if args.lib:
        E._lib.LIB_PATH = os.path.abspath(args.lib)                   # before the first load
    bench.cap_cpu_threads()
    assert torch.cuda.is_available(), "similarity_bench needs a GPU"
    dev = torch.device("cuda", 0)
    N, Ds, Dt = args.n, args.ds, args.dt
    g = torch.Generator().manual_seed(0)
    z = torch.randn(N, 16, generator=g)
    feat = torch.relu(z @ torch.randn(16, Ds, generator=g) + 0.5 * torch.randn(N, Ds, generator=g)).to(dev)
    teacher = torch.relu(z @ torch.randn(16, Dt, generator=g) + 0.5 * torch.randn(N, Dt, generator=g)).to(dev)
    a = torch.randint(0, N, (N * args.degree // 2,), generator=g)
    b = torch.randint(0, N, (N * args.degree // 2,), generator=g)
    edge_index = torch.stack([torch.cat([a, b]), torch.cat([b, a])]).to(dev)     # symmetric, in the index space of the N rows
    src, dst = edge_index

    def torch_global():
        fs, ft = F.normalize(feat, p=2, dim=-1), F.normalize(teacher, p=2, dim=-1)
        upper = torch.ones(N, N, dtype=torch.bool, device=dev).triu_(1)
        ps = (1 - torch.mm(fs, fs.t()))[upper]
        pt = (1 - torch.mm(ft, ft.t()))[upper]
        return float(torch.corrcoef(torch.stack([pt, ps]))[0, 1])

    def torch_local():
        fs, ft = F.normalize(feat, p=2, dim=-1), F.normalize(teacher, p=2, dim=-1)
        ps = 1 - F.cosine_similarity(fs[src], fs[dst])
        pt = 1 - F.cosine_similarity(ft[src], ft[dst])
        return float(torch.corrcoef(torch.stack([pt, ps]))[0, 1])

    n_small = min(N, args.kcka_torch_n)
    feat_small, teacher_small = feat[:n_small], teacher[:n_small]

    def torch_kcka():
        def centred_rbf(x):
            f = F.normalize(x, p=2, dim=-1)
            G = torch.mm(f, f.t())
            sq = G.diagonal()
            D = (sq[:, None] + sq[None, :] - 2 * G).clamp_min_(0)
            upper = torch.ones(n_small, n_small, dtype=torch.bool, device=dev).triu_(1)
            K = torch.exp(D / (-2 * D[upper].median()))
            K.fill_diagonal_(1.0)
            return K - K.mean(0, keepdim=True) - K.mean(1, keepdim=True) + K.mean()
        Kc, Lc = centred_rbf(feat_small), centred_rbf(teacher_small)
        return float((Kc * Lc).sum() / torch.sqrt((Kc * Kc).sum() * (Lc * Lc).sum()))

    groups = {
        "global": {"global_fused": lambda: E.structural_correlation(feat, teacher), "global_torch": torch_global},
        "local": {"local_fused": lambda: E.local_structural_correlation(feat, teacher, edge_index), "local_torch": torch_local},
        "cka": {"cka_fused": lambda: E.linear_cka(feat, teacher)},
        "kcka": {"kcka_fused": lambda: E.kernel_cka(feat, teacher),
                 "kcka_fused_small": lambda: E.kernel_cka(feat_small, teacher_small), "kcka_torch_small": torch_kcka},
    }
    wanted = args.metrics.split(",")
    forms = {k: fn for m in wanted for k, fn in groups[m].items()}

    def run(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        with torch.no_grad():
            value = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), torch.cuda.max_memory_allocated() - base, value

    times, peaks, values = {k: [] for k in forms}, {}, {}
    for i in range(args.warmup + args.reps):                      # alternating; the first `warmup` rounds are not kept
        for k, fn in forms.items():
            ms, peak, value = run(fn)
            if i >= args.warmup:
                times[k].append(ms)
                peaks[k] = max(peaks.get(k, 0), peak)
                values[k] = value
    def global_float64(chunk=2048):
        xs, xt = F.normalize(feat.double(), dim=-1), F.normalize(teacher.double(), dim=-1)
        m = torch.zeros(5, dtype=torch.float64, device=dev)
        cols = torch.arange(N, device=dev)
        for r0 in range(0, N, chunk):
            rows = cols[r0:r0 + chunk]
            keep = cols[None, :] > rows[:, None]
            a, b = (xs[rows] @ xs.t())[keep], (xt[rows] @ xt.t())[keep]
            m += torch.stack([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()])
        return E.pearson_from_moments([N * (N - 1) / 2] + m.tolist())

    res = {"what": "similarity", "N": N, "Ds": Ds, "Dt": Dt, "edges": int(edge_index.shape[1]), "unit": "ms", "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "lib": E._lib.build_info()}
    for k in forms:
        res[k] = {"median": round(statistics.median(times[k]), 3), "min": round(min(times[k]), 3), "max": round(max(times[k]), 3),
                  "peak_bytes": int(peaks[k]), "value": values[k]}
    if "global" in wanted:
        with torch.no_grad():
            r64 = global_float64()
        res["global_float64"] = r64
        res["global_fused_dev_from_float64"] = abs(res["global_fused"]["value"] - r64)
        res["global_torch_dev_from_float64"] = abs(res["global_torch"]["value"] - r64)
    for m in ("global", "local"):
        if m in wanted:
            res[f"{m}_torch_over_fused"] = round(res[f"{m}_torch"]["median"] / res[f"{m}_fused"]["median"], 3)
            res[f"{m}_value_gap"] = abs(res[f"{m}_torch"]["value"] - res[f"{m}_fused"]["value"])
    if "kcka" in wanted:
        res["kcka_small_N"] = n_small
        res["kcka_small_torch_over_fused"] = round(res["kcka_torch_small"]["median"] / res["kcka_fused_small"]["median"], 3)
        res["kcka_small_value_gap"] = abs(res["kcka_torch_small"]["value"] - res["kcka_fused_small"]["value"])
    print(f"| metric (N = {N}, {Ds} / {Dt}) | fused ms | torch ops ms | fused peak MB | torch ops peak MB |")
    print("|---|---|---|---|---|")
    mb = lambda v: f"{v / 2 ** 20:.1f}"   # noqa: E731
    for m in ("global", "local"):
        if m in wanted:
            f, t = res[f"{m}_fused"], res[f"{m}_torch"]
            print(f"| {m} r | {f['median']} | {t['median']} | {mb(f['peak_bytes'])} | {mb(t['peak_bytes'])} |")
    if "cka" in wanted:
        f = res["cka_fused"]
        print(f"| linear CKA | {f['median']} | -- | {mb(f['peak_bytes'])} | -- |")
    if "kcka" in wanted:
        f, fs, t = res["kcka_fused"], res["kcka_fused_small"], res["kcka_torch_small"]
        print(f"| kernel CKA | {f['median']} | -- | {mb(f['peak_bytes'])} | -- |")
        print(f"| kernel CKA at N = {n_small} | {fs['median']} | {t['median']} | {mb(fs['peak_bytes'])} | {mb(t['peak_bytes'])} |")
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=29_799)
    ap.add_argument("--ds", type=int, default=256)
    ap.add_argument("--dt", type=int, default=750)
    ap.add_argument("--degree", type=int, default=8, help="average edges per row of the synthetic symmetric edge list")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--metrics", default="global,local,cka,kcka", help="comma-separated subset of global, local, cka, kcka")
    ap.add_argument("--kcka-torch-n", type=int, default=8192, help="rows of the kernel-CKA comparison with the torch-op form")
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    sys.exit(main(ap.parse_args()))
