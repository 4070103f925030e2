#!/usr/bin/env python3
"""Generate tests/golden/arxiv_gat_train.npz by RUNNING THE REFERENCE'S OWN arxiv_dgl/models.py (GATConv / GAT) IN TRAINING MODE.

Run only in the build container (needs the reference checkout that make_golden.py reads):

    python tests/golden/make_golden_arxiv_gat_train.py

The DGL message-passing built-ins come from make_golden.py's shim; ``edge_drop = 0.3`` is the only randomness (``attn_drop``,
``dropout`` and ``input_drop`` are 0): the kept edge ids of every layer call are captured by wrapping ``torch.randperm`` while the
reference runs, and recorded as bool masks over the edges.  The toy graph is stored in CSR order (edges grouped by destination,
sources ascending), so an edge id IS a CSR entry.  Recorded:
  * ``layer_<attn>_<norm>__*``: one GATConv (3 heads x 6, residual), output and the gradients of sum(out * w) for the four
    (use_attn_dst, use_symmetric_norm) combinations;
  * ``model__*``: the --use-norm --no-attn-dst GAT (3 layers x 5 x 3 heads: a width not divisible by 4), one training step of
    arxiv_dgl/gat.py:116-148 with one label-reuse round, restated inline (gat.py imports matplotlib / ogb at module top): the loss of
    gat.py:98-101, every parameter gradient and the state after one RMSprop step (lr 0.002).
"""
from __future__ import annotations

import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets dont_write_bytecode, puts the repository root on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


class _Randperm:
    """Wraps ``torch.randperm`` while the reference runs: every permutation drawn is kept."""

    def __enter__(self):
        self.drawn, self._orig = [], torch.randperm

        def randperm(*a, **k):
            p = self._orig(*a, **k)
            self.drawn.append(p.clone())
            return p
        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.randperm = self._orig

    def keep_masks(self, nnz, p):
        out = []
        for perm in self.drawn:
            assert perm.numel() == nnz
            m = torch.zeros(nnz, dtype=torch.bool)
            m[perm[int(nnz * p):]] = True
            out.append(m)
        return out


def toy_graph(g, n=96, density=0.05, hub=5, lone=17):
    """Bidirected, self loops replaced (gat.py:56-71), CSR order; row ``hub`` lists every node (> 64 entries); node ``lone`` keeps
    its self loop only, so edge_drop can leave it (and other short rows) without a kept entry."""
    a = torch.rand(n, n, generator=g) < density
    a[hub, :] = True
    a[lone, :] = False
    a = a | a.t()
    a[lone, :] = False
    a[:, lone] = False
    a.fill_diagonal_(True)
    dst, src = torch.nonzero(a, as_tuple=True)
    return src, dst


def main():
    MG.install_dgl_shim()
    models = MG.load_ref("arxiv_dgl/models.py", "ref_arxiv_dgl_models_train")
    g = torch.Generator().manual_seed(53)
    n, F_in, C, heads, p_edge = 96, 11, 6, 3, 0.3
    src, dst = toy_graph(g, n)
    nnz = src.numel()
    graph = MG._DGLGraph(src, dst, n)
    x = torch.randn(n, F_in, generator=g)
    out = {"in_src": MG.t2n(src), "in_dst": MG.t2n(dst), "in_x": MG.t2n(x), "edge_drop": np.float32(p_edge)}

    # ---- one layer, four configurations
    w = torch.randn(n, heads, 6, generator=g)
    out["layer_w"] = MG.t2n(w)
    for attn_dst in (False, True):
        for sym in (False, True):
            name = f"layer_{'attn' if attn_dst else 'noattn'}_{'norm' if sym else 'plain'}"
            torch.manual_seed(11)
            conv = models.GATConv(F_in, 6, num_heads=heads, edge_drop=p_edge, use_attn_dst=attn_dst, use_symmetric_norm=sym,
                                  residual=True).train()
            for k, v in conv.state_dict().items():
                out[f"{name}__param__{k}"] = MG.t2n(v)
            xr = x.clone().requires_grad_(True)
            with _Randperm() as rp:
                y = conv(graph, xr)
            (keep,) = rp.keep_masks(nnz, p_edge)
            (y * w).sum().backward()
            out[f"{name}__keep"], out[f"{name}__out"], out[f"{name}__d_x"] = MG.t2n(keep), MG.t2n(y), MG.t2n(xr.grad)
            for k, v in conv.named_parameters():
                out[f"{name}__grad__{k}"] = MG.t2n(v.grad)

    # ---- the --use-norm --no-attn-dst model: one training step with one label-reuse round (gat.py:116-148 restated)
    labels = torch.randint(0, C, (n, 1), generator=g)
    perm = torch.randperm(n, generator=g)
    train_idx, val_idx, test_idx = perm[:56], perm[56:76], perm[76:]
    mask = torch.rand(train_idx.shape, generator=g) < 0.5
    torch.manual_seed(13)
    model = models.GAT(F_in + C, C, 5, 3, heads, F.relu, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=p_edge,
                       use_attn_dst=False, use_symmetric_norm=True)
    with torch.no_grad():
        for bn in model.norms:
            bn.weight.uniform_(0.5, 1.5, generator=g)
            bn.bias.normal_(0, 0.2, generator=g)
        model.bias_last.bias.normal_(0, 0.5, generator=g)
    for k, v in model.state_dict().items():
        out[f"model__init__{k}"] = MG.t2n(v)
    opt = torch.optim.RMSprop(model.parameters(), lr=0.002, weight_decay=0)
    model.train()
    train_labels_idx, train_pred_idx = train_idx[mask], train_idx[~mask]
    onehot = torch.zeros([n, C])
    onehot[train_labels_idx, labels[train_labels_idx, 0]] = 1
    feat = torch.cat([x, onehot], dim=-1)
    opt.zero_grad()
    with _Randperm() as rp:
        pred = model(graph, feat)
        unlabel_idx = torch.cat([train_pred_idx, val_idx, test_idx])
        pred = pred.detach()
        feat[unlabel_idx, -C:] = F.softmax(pred[unlabel_idx], dim=-1)
        pred = model(graph, feat)
    keeps = rp.keep_masks(nnz, p_edge)
    assert len(keeps) == 6                                              # two forwards x three layers, in call order
    epsilon = 1 - math.log(2)
    ce = F.cross_entropy(pred[train_pred_idx], labels[train_pred_idx][:, 0], reduction="none")
    loss = torch.mean(torch.log(epsilon + ce) - math.log(epsilon))
    loss.backward()
    for k, v in model.named_parameters():
        out[f"model__grad__{k}"] = MG.t2n(v.grad)
    opt.step()
    for k, v in model.state_dict().items():
        out[f"model__final__{k}"] = MG.t2n(v)
    out.update({"model__keep": np.stack([MG.t2n(k) for k in keeps]), "model__loss": np.float64(loss.item()), "model__pred": MG.t2n(pred),
                "in_labels": MG.t2n(labels), "in_train": MG.t2n(train_idx), "in_val": MG.t2n(val_idx), "in_test": MG.t2n(test_idx),
                "in_mask": MG.t2n(mask)})
    path = os.path.join(HERE, "arxiv_gat_train.npz")
    np.savez_compressed(path, **out)
    deg = torch.bincount(dst, minlength=n)
    print(f"arxiv_gat_train.npz: {os.path.getsize(path)} bytes, n={n} nnz={nnz} max deg={int(deg.max())}, "
          f"layer x 4 configs + one model training step")


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "needs the reference checkout (build container only)"
    torch.set_num_threads(1)
    main()
