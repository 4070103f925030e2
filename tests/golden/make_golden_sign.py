#!/usr/bin/env python3
"""Generate tests/golden/sign.npz by RUNNING THE REFERENCE'S OWN arxiv_dgl/sign.py (FeedForwardNet / SIGN / train / train_kd_and_aux /
test) on a tiny problem.

Run only in the build container (needs the reference checkout that make_golden.py reads):

    python tests/golden/make_golden_sign.py [--out DIR] [--search]

``dgl`` / ``ogb`` / ``torch_geometric`` come from make_golden.py's shims (sign.py's model and loops use none of them).  Dropout is
the only randomness of a training pass: every ``F.dropout`` call of the reference receives a mask of ``oracle.dropout.counter_mask``
under a recorded seed (``oracle.dropout.injected_dropout``), in the reference's call order -- input drop of hops 0..H-1; hop by hop,
that hop's hidden levels; the concatenation; ``project``'s hidden levels.  The HIP path, fed the same seeds in the same order,
recomputes the same masks in its kernels.

Problem: N = 96 nodes, F = 12, hidden 16, 5 classes, R = 2 (H = 3 hops), teacher width 17, proj_dim 8, dropout 0.5, input dropout
0.1; 70 train rows as batches of 40 and 30; eval batches of 40.  Recorded:
  * ``L<n>__init__*``: the state_dict right after ``torch.manual_seed(INIT_SEED + n)`` + construction, ff_layer n = 1, 2, 3;
  * ``L<n>__seeds / logits / out_feat / grad__* / eval_logits``: a train-mode forward + backward of sum(logits * w) on the first
    batch, and an eval-mode forward of the same rows;
  * ``kda_<mode>__*`` (six modes, ``train_kd_and_aux``) and ``tr_<mode>__*`` (supervised, nce; ``train``): initial parameters, the
    seeds, the returned means and the parameters after the epoch's two Adam steps (ff_layer 2);
  * ``test__logits / test__accs``: ``test()`` over the 96 rows.
The script asserts what the tests rely on: every mask drops and keeps something, and every PReLU argument of every recorded pass
has |z| > 1e-4 (a PReLU argument at rounding distance from 0 would make a gradient comparison meaningless; DATA_SEED is picked so
that this holds: ``--search`` prints the first seeds that do).  Deterministic: the archive carries no timestamps, so a second run
reproduces the file bit for bit.
"""
from __future__ import annotations

import argparse
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets dont_write_bytecode, puts the repository root on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.dropout import counter_mask, injected_dropout  # noqa: E402

N, F_IN, HIDDEN, CLASSES, R, T_DIM, PROJ = 96, 12, 16, 5, 2, 17, 8
H = R + 1
P_DROP, P_IN = 0.5, 0.1
INIT_SEED = 40
DATA_SEED = 27
MIN_ABS_Z = 1e-4
HP = dict(alpha=0.9, kd_T=4.0, beta=0.5, nce_T=0.075, max_samples=64, proj_dim=PROJ, kernel="rbf")
LR = 0.01
KDA_MODES = ("supervised", "kd", "fitnet", "at", "gpw", "nce")
TRAIN_MODES = ("supervised", "nce")


def load_reference():
    MG.install_shims()
    MG.install_dgl_shim()
    sys.modules["ogb.nodeproppred"].DglNodePropPredDataset = None
    return MG.load_ref("arxiv_dgl/sign.py", "ref_arxiv_dgl_sign")


def mask_shapes(B, L):
    """(rows, columns, p) of every dropout call of one training forward of SIGN(..., n_layers=L), in call order."""
    shapes = [(B, F_IN, P_IN)] * H
    shapes += [(B, HIDDEN, P_DROP)] * (H * (L - 1))
    shapes += [(B, H * HIDDEN, P_DROP)]
    shapes += [(B, HIDDEN, P_DROP)] * (L - 1)
    return shapes


def draw_masks(rs, B, L):
    seeds = [int(s) for s in rs.randint(0, 2 ** 62, size=len(mask_shapes(B, L)), dtype=np.int64)]
    masks = [counter_mask(s, n, c, p) for s, (n, c, p) in zip(seeds, mask_shapes(B, L))]
    for m in masks:
        assert bool((m == 0).any()) and bool((m != 0).any()), "a mask that drops nothing or everything"
    return seeds, masks


class ZWatch:
    """Forward pre-hooks on every nn.PReLU of a model: the smallest |pre-activation| seen."""

    def __init__(self):
        self.min_abs = float("inf")

    def watch(self, model):
        for m in model.modules():
            if isinstance(m, torch.nn.PReLU):
                m.register_forward_pre_hook(lambda mod, inp: self._see(inp[0]))
        return model

    def _see(self, z):
        self.min_abs = min(self.min_abs, float(z.detach().abs().min()))


def problem(data_seed):
    g = torch.Generator().manual_seed(1000 + data_seed)
    feats = [torch.randn(N, F_IN, generator=g) * 5.0 for _ in range(H)]
    labels = torch.randint(0, CLASSES, (N,), generator=g)
    perm = torch.randperm(N, generator=g)
    train_nid, val_nid, test_nid = perm[:70], perm[70:83], perm[83:]
    order = train_nid[torch.randperm(70, generator=g)]
    batches = [order[:40].clone(), order[40:].clone()]
    teacher_out_feat = torch.randn(N, T_DIM, generator=g)
    teacher_logits = torch.randn(N, CLASSES, generator=g) * 2.0
    w = torch.randn(40, CLASSES, generator=g)
    return dict(feats=feats, labels=labels, train_nid=train_nid, val_nid=val_nid, test_nid=test_nid, batches=batches,
                teacher_out_feat=teacher_out_feat, teacher_logits=teacher_logits, w=w)


def build(ref, data_seed):
    """(arrays of sign.npz, the smallest |PReLU argument| of all recorded passes)."""
    D = problem(data_seed)
    feats, labels, batches = D["feats"], D["labels"], D["batches"]
    out = {f"in_feat{h}": MG.t2n(f) for h, f in enumerate(feats)}
    out.update({"in_labels": MG.t2n(labels), "in_train": MG.t2n(D["train_nid"]), "in_val": MG.t2n(D["val_nid"]),
                "in_test": MG.t2n(D["test_nid"]), "in_batch0": MG.t2n(batches[0]), "in_batch1": MG.t2n(batches[1]),
                "in_teacher_out_feat": MG.t2n(D["teacher_out_feat"]), "in_teacher_logits": MG.t2n(D["teacher_logits"]),
                "in_w": MG.t2n(D["w"]),
                "hp": np.array([HP["alpha"], HP["kd_T"], HP["beta"], HP["nce_T"], HP["max_samples"], LR, P_DROP, P_IN], dtype=np.float64)})
    rs = np.random.RandomState(77 + data_seed)
    watch = ZWatch()

    # ---- initial values, one training forward + backward, one eval forward: ff_layer 1, 2, 3
    b0 = batches[0]
    for L in (1, 2, 3):
        tag = f"L{L}"
        torch.manual_seed(INIT_SEED + L)
        model = watch.watch(ref.SIGN(F_IN, HIDDEN, CLASSES, H, L, P_DROP, P_IN))
        for k, v in model.state_dict().items():
            out[f"{tag}__init__{k}"] = MG.t2n(v)
        seeds, masks = draw_masks(rs, b0.numel(), L)
        model.train()
        with injected_dropout(masks) as st:
            logits = model([x[b0] for x in feats])
        assert st.left() == 0, "the reference drew fewer masks than the stated order has"
        (logits * D["w"]).sum().backward()
        out[f"{tag}__seeds"] = np.array(seeds, dtype=np.int64)
        out[f"{tag}__logits"], out[f"{tag}__out_feat"] = MG.t2n(logits), MG.t2n(model.out_feat)
        for k, v in model.named_parameters():
            out[f"{tag}__grad__{k}"] = MG.t2n(v.grad)
        model.eval()
        with torch.no_grad():
            out[f"{tag}__eval_logits"] = MG.t2n(model([x[b0] for x in feats]))

    # ---- one epoch (two Adam steps) of the reference's own loops, ff_layer 2
    def epoch(tag, mode, fn, i):
        args = argparse.Namespace(training=mode, **HP)
        torch.manual_seed(INIT_SEED + 10 + i)
        model = watch.watch(ref.SIGN(F_IN, HIDDEN, CLASSES, H, 2, P_DROP, P_IN))
        sp = tp = None
        if mode in ("nce", "fitnet", "gpw"):
            sp = torch.nn.Sequential(torch.nn.Linear(HIDDEN * H, PROJ), torch.nn.BatchNorm1d(PROJ), torch.nn.ReLU())
            tp = torch.nn.Sequential(torch.nn.Linear(T_DIM, PROJ), torch.nn.BatchNorm1d(PROJ), torch.nn.ReLU())
            opt = torch.optim.Adam([{"params": model.parameters(), "lr": LR, "weight_decay": 0},
                                    {"params": sp.parameters(), "lr": LR, "weight_decay": 0},
                                    {"params": tp.parameters(), "lr": LR, "weight_decay": 0}])
        else:
            opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=0)
        mods = [("model", model)] + ([("sproj", sp), ("tproj", tp)] if sp is not None else [])
        for name, m in mods:
            for k, v in m.state_dict().items():
                out[f"{tag}__init__{name}.{k}"] = MG.t2n(v)
        seeds, masks = [], []
        for b in batches:
            s, m = draw_masks(rs, b.numel(), 2)
            seeds += s
            masks += m
        np.random.seed(0)   # (max_samples >= the batch size: the criteria draw nothing)
        with injected_dropout(masks) as st:
            means = fn(model, feats, labels, opt, batches, args, D["teacher_out_feat"], D["teacher_logits"], sp, tp)
        assert st.left() == 0
        out[f"{tag}__seeds"] = np.array(seeds, dtype=np.int64)
        out[f"{tag}__means"] = np.array(means, dtype=np.float64)
        for name, m in mods:
            for k, v in m.state_dict().items():
                out[f"{tag}__final__{name}.{k}"] = MG.t2n(v)
        return model

    assert HP["max_samples"] >= 40
    last = None
    for i, mode in enumerate(KDA_MODES):
        last = epoch(f"kda_{mode}", mode, ref.train_kd_and_aux, i)
    for i, mode in enumerate(TRAIN_MODES):
        epoch(f"tr_{mode}", mode, ref.train, 6 + i)

    # ---- test() of the model the last kd_and_aux epoch left (its parameters are kda_nce__final__model.*)
    loader = [torch.arange(N)[i:i + 40] for i in range(0, N, 40)]
    with torch.no_grad():
        logits, accs = ref.test(last, feats, labels, loader, ref.get_ogb_evaluator("ogbn-arxiv"), D["train_nid"], D["val_nid"],
                                D["test_nid"])
    out["test__logits"], out["test__accs"] = MG.t2n(logits), np.array(accs, dtype=np.float64)
    return out, watch.min_abs


def save_npz(path, arrays):
    """A compressed .npz without timestamps (np.savez stamps every member with the wall clock): the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE, help="directory that receives sign.npz")
    ap.add_argument("--search", action="store_true", help="print the data seeds below 40 for which the |z| condition holds; write nothing")
    a = ap.parse_args()
    ref = load_reference()
    if a.search:
        for s in range(40):
            print(s, build(ref, s)[1], flush=True)
        return
    out, min_abs = build(ref, DATA_SEED)
    assert min_abs > MIN_ABS_Z, f"a PReLU argument with |z| = {min_abs:g} <= {MIN_ABS_Z:g}: pick another DATA_SEED (--search)"
    path = os.path.join(a.out, "sign.npz")
    save_npz(path, out)
    print(f"sign.npz: {os.path.getsize(path)} bytes, {len(out)} arrays, min |PReLU argument| = {min_abs:.3g}")


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "needs the reference checkout (build container only)"
    torch.set_num_threads(1)
    main()
