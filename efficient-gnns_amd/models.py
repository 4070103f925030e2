"""Student models and the train / eval step, mirroring the reference's L1/L2 code on the new operators.

``GCN`` / ``SAGE`` / ``ProjectionGCD`` follow /root/reference/arxiv_pyg/gnn.py:23-99 (same constructor
signatures, ``convs`` / ``bns`` state_dict keys, ``.out_feat`` side channel); ``train_step`` follows
``train()`` (:102-195) and the KD+aux rule of gnn_kd_and_aux.py:114-181; ``evaluate`` follows ``test()``
(:198-218).  The reference's own ``gnn.py`` also runs unchanged on top of ``efficient-gnns_amd/dropin``.
"""
from __future__ import annotations

import contextlib
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import _cache, _lib
from . import criterion as C
from . import ops
from .nn import (ATOM_DIMS, BOND_DIMS, CategoricalEncoder, DGLGATConv, GATConv, GCNConv, GINConv, GINEConv, RGCNConv, SAGEConv,
                 global_add_pool, global_max_pool, global_mean_pool)
from .sparse import SparseTensor


_EVAL_BN_FOLD = True   # (no environment switch any more; tests flip the attribute to compare the fold with the separate normalisation pass)
# Fusions measured in round 3 (profiles/r03_bench_line_r02_paths.json: all five off = 130.5 vs 144.3 epochs/s); module attributes, no
# environment switches -- tests flip them to compare each fused form with its composed one.
_TRAIN_ROWS = True        # [train_idx] row picks inside the CE / KD kernels
_FUSED_TAIL = True        # ops.bn_act_linear for the last hidden layer of a GCN


class _Student(nn.Module):
    def __init__(self, make_conv, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        dims = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.convs = nn.ModuleList(make_conv(a, b) for a, b in zip(dims[:-1], dims[1:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.dropout = dropout
        self.out_feat = None

    def reset_parameters(self):
        for m in list(self.convs) + list(self.bns):
            m.reset_parameters()

    # ---- the layer plan ---------------------------------------------------------------------------------------------------
    # Every hidden layer is conv -> BatchNorm -> ReLU -> dropout (gnn.py:47-50).  WHICH kernels run it depends on five facts that
    # hold for a whole forward pass (mode, grad mode, device, adjacency kind, module types); ``_layer_form`` names the pair
    # (conv form, activation form) of a layer and ``forward`` only executes it:
    #   conv form   "fold"   test(): eval-mode BatchNorm folded into the conv's weights, ReLU in the last kernel's store (no act.)
    #               "stats"  training GCNConv on a plain adjacency: BatchNorm statistics from the aggregation's store epilogue
    #               "plain"  conv(x, adj_t)
    #   act. form   "tail"       last hidden layer of a GCN: BN + ReLU + dropout + gradient tap + the output conv's h @ W as ONE op
    #               "tail_sync"  the same on node-range shards (dist.SyncBatchNorm1d: all-rank statistics)
    #               "bn_act"     fused BN + ReLU + dropout kernels (torch.nn.BatchNorm1d)
    #               "sync"       dist.SyncBatchNorm1d.fused_act
    #               "torch"      another norm module (CPU tensors: the gloo tests' stand-in switch only)
    def _layer_form(self, li, x, adj_t):
        conv, bn, last = self.convs[li], self.bns[li], self.convs[-1]
        training, grad, gpu = self.training, torch.is_grad_enabled(), x.is_cuda
        plain_adj, sharded_adj = isinstance(adj_t, SparseTensor), hasattr(adj_t, "gcn_normalized")
        gcn, torch_bn, sync_bn = isinstance(conv, GCNConv), isinstance(bn, nn.BatchNorm1d), hasattr(bn, "fused_act")
        if (_EVAL_BN_FOLD and not training and not grad and gcn and gpu and not conv._uses_memoised_input(x)
                and ((type(bn) is nn.BatchNorm1d and bn.track_running_stats and plain_adj) or (sharded_adj and sync_bn))):
            return "fold", None
        conv_form = "stats" if (gcn and torch_bn and gpu and training and plain_adj) else "plain"
        act = "bn_act" if (torch_bn and gpu) else ("sync" if sync_bn else "torch")
        if (li == len(self.bns) - 1 and _FUSED_TAIL and training and grad and gpu and isinstance(last, GCNConv)
                and last.in_channels >= last.out_channels):
            if plain_adj and not sharded_adj and type(bn) is nn.BatchNorm1d and last.out_channels <= 64 and last.in_channels % 64 == 0:
                act = "tail"
            elif sharded_adj and hasattr(bn, "fused_act_linear"):
                act = "tail_sync"
        return conv_form, act

    def forward(self, x, adj_t):
        for li, (conv, bn) in enumerate(zip(self.convs[:-1], self.bns)):
            conv_form, act = self._layer_form(li, x, adj_t)
            if conv_form == "fold":
                x = self.out_feat = conv(x, adj_t, eval_bn=bn)
                continue
            x = conv(x, adj_t, bn_stats_shift=bn.running_mean, want_bn_stats=True) if conv_form == "stats" else conv(x, adj_t)
            if act in ("tail", "tail_sync"):
                # (h, h @ W_out) in one op whose backward is one pass over the [N, hidden] tensors (ops._BnActLinear); None = the fused
                # kernels do not take this shape: the composed form below
                both = (ops.bn_act_linear(x, bn, self.convs[-1].weight, relu=True, p=self.dropout, training=True) if act == "tail"
                        else bn.fused_act_linear(x, self.convs[-1].weight, True, self.dropout, True))
                if both is not None:
                    self.out_feat, xw = both
                    return self.convs[-1](self.out_feat, adj_t, xw=xw)
                act = "bn_act" if act == "tail" else "sync"
            if act == "bn_act":
                x = ops.bn_act(x, bn, relu=True, p=self.dropout, training=self.training)
            elif act == "sync":
                x = bn.fused_act(x, True, self.dropout, self.training)
            else:                      # another norm module: torch's own operators (on the GPU)
                _lib.require_gpu(x)
                x = F.dropout(F.relu(bn(x)), p=self.dropout, training=self.training)
            self.out_feat = x
        if self.training and x.is_cuda:
            # the last hidden state has two consumers (the last conv and student_proj(out_feat[train_idx]), gnn.py:150): the projection's
            # row-compact input gradient is added into the conv's dense one instead of autograd's zero-fill + scatter + full-size add
            x = self.out_feat = ops.grad_tap(x)
        return self.convs[-1](x, adj_t)


class GCN(_Student):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, cached=True):
        super().__init__(lambda a, b: GCNConv(a, b, cached=cached), in_channels, hidden_channels, out_channels,
                         num_layers, dropout)


class SAGE(_Student):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, aggr="mean"):
        super().__init__(lambda a, b: SAGEConv(a, b, aggr=aggr), in_channels, hidden_channels, out_channels,
                         num_layers, dropout)


class ProjectionGCD(nn.Module):
    def __init__(self, hidden_channels, proj_dim):
        super().__init__()
        self.lin = nn.Linear(hidden_channels, proj_dim)
        self.conv = GCNConv(hidden_channels, proj_dim)
        self.bn = nn.BatchNorm1d(proj_dim)

    def forward(self, x, adj_t):
        return F.relu(self.bn(self.lin(x) + self.conv(x, adj_t)))


class ProjectionHead(nn.Sequential):
    """Linear + BatchNorm1d + ReLU (gnn.py:296-306) with the reference's Sequential state_dict keys (0.*, 1.*);
    the forward runs the MFMA GEMM and the fused BN + ReLU kernels."""

    def __init__(self, in_dim, proj_dim):
        super().__init__(nn.Linear(in_dim, proj_dim), nn.BatchNorm1d(proj_dim), nn.ReLU())

    def forward(self, x):
        lin, bn = self[0], self[1]
        if hasattr(bn, "fused_act"):                            # dist.SyncBatchNorm1d
            return bn.fused_act(ops.linear(x, lin.weight, lin.bias), True, 0.0, self.training)
        _lib.require_gpu(x)
        if not isinstance(bn, nn.BatchNorm1d):
            return super().forward(x)
        return ops.bn_act(ops.linear(x, lin.weight, lin.bias), bn, relu=True, p=0.0, training=self.training)

    def forward_rows(self, x, idx, pick=None, const_input=False):
        """``self(x[idx])`` for unique row ids: the gather is fused into the GEMM's operand load (gnn.py:150-156).
        ``pick`` (unique ids into ``idx``): ``self(x[idx])[pick]`` -- what a sampled criterion keeps of the head's output
        (criterion.py:62-65,134-137); the BatchNorm statistics span all of ``idx``, only the picked rows are normalised and stored."""
        lin, bn = self[0], self[1]
        y = ops.linear_rows(x, idx, lin.weight, lin.bias, const_input=const_input)   # const_input: see ops.linear_rows (the teacher head)
        if hasattr(bn, "fused_act"):                            # dist.SyncBatchNorm1d: all-rank statistics, only the picked rows formed
            return bn.fused_act(y, True, 0.0, self.training, pick=pick)
        if not isinstance(bn, nn.BatchNorm1d):
            y = self[2](bn(y))
            return y if pick is None else y[pick]
        return ops.bn_act(y, bn, relu=True, p=0.0, training=self.training, pick=pick)


def make_projection(in_dim, proj_dim):
    return ProjectionHead(in_dim, proj_dim)


_ROW_CACHE = _cache.TensorKeyedCache(capacity=8)
_CACHE_CONST_ROWS = os.environ.get("EGNN_CACHE_CONST_ROWS", "0") == "1"  # opt-in (the reference re-gathers every step)


def _const_rows(t, idx):
    """``t[idx]`` for a constant tensor (teacher artefacts): the reference re-gathers 273 MB every step (gnn.py:155);
    the rows do not change within a run, so (opt-in) the gather is done once per (tensor, index) identity + version."""
    if t.requires_grad or not _CACHE_CONST_ROWS:
        return t[idx]
    return _ROW_CACHE.get((t, idx), (), lambda: t[idx])


_GLOBAL_EDGES = _cache.TensorKeyedCache(capacity=8)


def _global_edges(edge_index, train_idx):
    """``train_idx[edge_index]``: the edge list of the train-induced subgraph (relabelled, gnn.py:274) in node ids of the full graph.
    Built once per (edge list, index) identity + version; the entry keeps both alive (_cache.py)."""
    return _GLOBAL_EDGES.get((edge_index, train_idx), (), lambda: train_idx[edge_index].contiguous())


def distill_loss(mode, model, out, labels, train_idx, teacher_out_feat, teacher_logits, hp,
                 student_proj=None, teacher_proj=None, edge_index=None, adj_t=None, kd_and_aux=False, rows=None):
    """``rows`` = None: ``out`` / ``labels`` are the compact train rows (gnn.py:109-110).  ``rows`` = train_idx: they are the FULL
    logits / labels and the criteria pick the rows inside their kernels (criterion.py's ``rows`` keyword)."""
    if mode == "supervised":
        loss = ops.cross_entropy(out, labels, rows)
        return loss, loss, loss * 0
    if rows is None and (mode == "kd" or kd_and_aux):      # the only modes that form a KD term: no gather launch in the others
        teacher_logits = _const_rows(teacher_logits, train_idx)
    f = t = None
    picked = False
    if mode in ("fitnet", "gpw", "nce"):
        if hasattr(student_proj, "forward_rows") and hasattr(teacher_proj, "forward_rows") and not _CACHE_CONST_ROWS:
            # the criterion's one host draw (criterion.py:62-65,134-137), made here: the heads then form only the sampled rows
            pick = C.presample(mode, train_idx.numel(), hp, model.out_feat.device)
            picked = pick is not None
            f = student_proj.forward_rows(model.out_feat, train_idx, pick=pick)   # proj(feat[train_idx]) without the copies
            t = teacher_proj.forward_rows(teacher_out_feat, train_idx, pick=pick, const_input=True)   # the teacher's features never change (gnn.py:155)
        else:
            f = student_proj(ops.take_rows(model.out_feat, train_idx))
            t = teacher_proj(_const_rows(teacher_out_feat, train_idx))
    elif mode == "lpw" and edge_index is not None:
        # LSP reads rows only through the edge list (criterion.py:100-104): the train-subgraph ids of gnn.py:274 are composed with
        # train_idx once, and the edge kernels then address the FULL feature tensors -- feat[train_idx] / teacher_feat[train_idx] (366 MB of
        # copies per step) and the zero-fill + scatter of their backward never exist; the loss is a mean over the same edges.
        f, t, edge_index = model.out_feat, teacher_out_feat, _global_edges(edge_index, train_idx)
    elif mode in ("at", "lpw"):
        f, t = ops.take_rows(model.out_feat, train_idx), _const_rows(teacher_out_feat, train_idx)
    elif mode == "gcd":
        f = student_proj(model.out_feat, adj_t)[train_idx]
        t = teacher_proj(teacher_out_feat, adj_t)[train_idx]
    return C.distill(mode, out, labels, f, t, hp, teacher_logits=teacher_logits, rows=rows, edge_index=edge_index, presampled=picked,
                     kd_and_aux=kd_and_aux)


_ONES: dict = {}


def _one_like(t):
    """A cached 0-dim 1.0 on ``t``'s device: ``loss.backward(gradient=...)`` without autograd's per-step ones_like fill launch.  Never
    evicted (4 bytes per device; captured graphs read it through a raw pointer)."""
    key = (str(t.device), t.dtype)
    one = _ONES.get(key)
    if one is None:
        one = _ONES[key] = torch.ones((), dtype=t.dtype, device=t.device)
    return one


def train_mode(model, student_proj=None, teacher_proj=None, teacher_model=None):
    """What every training loop sets before its first step: student and projection heads train, the frozen teacher evaluates."""
    model.train()
    for p in (student_proj, teacher_proj):
        if p is not None:
            p.train()
    if teacher_model is not None:
        teacher_model.eval()


def train_step_tensors(model, x, adj_t, y, train_idx, optimizer, mode, hp, teacher_out_feat=None, teacher_logits=None,
                       student_proj=None, teacher_proj=None, edge_index=None, kd_and_aux=False, out=None):
    """One full-graph optimisation step (gnn.py:102-195) WITHOUT the host reads: returns the device tensor
    [loss, loss_cls, loss_aux] (written into ``out`` -- float32 [3] -- when given).  (``train_step`` adds the reads; ``GraphedEpoch``
    captures this function.)"""
    train_mode(model, student_proj, teacher_proj)
    logits = model(x, adj_t)
    if _TRAIN_ROWS and logits.is_cuda and y.dim() == 2 and y.shape[1] == 1 and y.dtype == torch.int64:
        # gnn.py:109-110 `out = model(...)[train_idx]`, `y.squeeze(1)[train_idx]` (and `teacher_logits[train_idx]`): the row picks
        # happen inside the CE / KD kernels (the criteria's `rows` keyword), their backward writes the dense logits gradient
        loss, loss_cls, loss_aux = distill_loss(mode, model, logits, y.view(-1), train_idx, teacher_out_feat, teacher_logits, hp,
                                                student_proj, teacher_proj, edge_index, adj_t, kd_and_aux, rows=train_idx)
    else:
        picked = ops.take_rows(logits, train_idx)   # == model(...)[train_idx] (split ids are unique)
        labels = y.squeeze(1)[train_idx]
        loss, loss_cls, loss_aux = distill_loss(mode, model, picked, labels, train_idx, teacher_out_feat, teacher_logits, hp,
                                                student_proj, teacher_proj, edge_index, adj_t, kd_and_aux)
    optimizer.zero_grad()
    loss.backward(gradient=_one_like(loss) if loss.is_cuda and loss.dim() == 0 else None)
    optimizer.step()
    return torch.stack([loss.detach(), loss_cls.detach(), loss_aux.detach()], out=out)


def train_step(model, x, adj_t, y, train_idx, optimizer, mode, hp, teacher_out_feat=None, teacher_logits=None,
               student_proj=None, teacher_proj=None, edge_index=None, kd_and_aux=False):
    """One full-graph optimisation step (= one training epoch of the reference); the three losses as Python floats (the
    reference's three ``.item()`` reads, here one device->host copy)."""
    vals = train_step_tensors(model, x, adj_t, y, train_idx, optimizer, mode, hp, teacher_out_feat, teacher_logits,
                              student_proj, teacher_proj, edge_index, kd_and_aux)
    a, b, c = vals.tolist()
    return a, b, c


def accuracy(y_true, y_pred) -> float:
    """``ogb`` Evaluator('ogbn-arxiv')['acc'] = mean(y_true == y_pred); compared on the device, one scalar read."""
    return float((y_true == y_pred).float().mean())


@torch.no_grad()
def evaluate_tensors(model, x, adj_t, y, split_idx, accs_out=None):
    """``test()`` (gnn.py:198-218) without the host read: (logits, device tensor of the three accuracies -- ``accs_out``, float64 [3],
    when given)."""
    model.eval()
    out = model(x, adj_t)
    if y.dtype == torch.int64 and y.numel() == out.shape[0]:
        return out, ops.split_accuracy(out, y, split_idx, out=accs_out)   # argmax + the three Evaluator accuracies in one pass
    y_pred = out.argmax(dim=-1, keepdim=True)
    hit = (y_pred == y).view(-1).to(torch.float32)
    return out, torch.stack([hit[split_idx[k]].mean() for k in ("train", "valid", "test")])


@torch.no_grad()
def evaluate(model, x, adj_t, y, split_idx):
    _lib.require_gpu(x)
    out, accs = evaluate_tensors(model, x, adj_t, y, split_idx)   # the three Evaluator accuracies with ONE device->host read instead of three
    return out, tuple(accs.tolist())


@torch.no_grad()
def student_similarity(model, x, adj_t, teacher_out_feat, idx, edge_index=None, kernel_cka=False):
    """How much of the teacher's structure the student's hidden space keeps over the rows ``idx`` (arxiv_pyg/correlation.py:200-214):
    one eval-mode forward, then ``similarity.representation_similarity(model.out_feat, teacher_out_feat, idx, edge_index)`` --
    ``dict(global_=..., local=..., cka=...)``, plus ``kcka`` (RBF CKA, :70-75) with ``kernel_cka=True``.  The model comes back in the
    mode it was in; eval mode leaves the BatchNorm running statistics as they are."""
    from .similarity import representation_similarity
    _lib.require_gpu(x, teacher_out_feat)
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        model(x, adj_t)
        return representation_similarity(model.out_feat, teacher_out_feat, idx, edge_index, kernel_cka=kernel_cka)
    finally:
        for m, was_training in flags:
            m.training = was_training


class ReplayedEpoch:
    """An epoch captured ONCE as a hipGraph and replayed, with the per-step host randomness staged around the replays -- the part
    ``GraphedEpoch`` (one GPU) and ``dist.ShardedGraphedEpoch`` (a rank's shard) share.  The host draws of a step (the criterion's
    row sample, the dropout seed) go to pinned staging buffers and are uploaded stream-ordered into static device buffers the
    captured kernels read; the epoch's values are read back once per epoch.  A subclass supplies the capture hooks
    (``_installed``), the pick (``_draw_pick`` / ``_upload_pick``), the launch (``_launch``: the device tensor of the epoch's
    values), their decoding (``_decode``) and the structural graph check (``_check_graph``)."""

    capture_error_mode = "global"      # torch.cuda.graph's default

    def __init__(self, dev, n_pick: int, res_numel: int, res_dtype):
        self.n_pick = n_pick
        self._pick_dev = torch.zeros(max(n_pick, 1), dtype=torch.int64, device=dev)
        self._pick_host = torch.zeros(max(n_pick, 1), dtype=torch.int64).pin_memory()
        self._seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._seed_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self._uploaded = None             # event behind the last upload of the staging buffers
        # step_async: two pinned host slots for the epoch's values (shape and dtype of the ``_launch`` result)
        self._res_host = [torch.zeros(res_numel, dtype=res_dtype).pin_memory() for _ in range(2)]
        self._res_done = [None, None]
        self._pending = None              # slot of the epoch whose values have not been handed out yet
        self._k = 0
        self.replay_events = None         # set to a list to collect (start, end) HIP events around every launch of step_async (bench.py)

    def _capture(self, body, dev, warmup):
        """Warm-up, capture and instantiation of ``body``; returns what the captured ``body`` returned (its static outputs)."""
        from ._audit import CaptureAudit
        what = type(self).__name__
        # every cached structure the captured launches read through raw pointers (edge plans, composed edge lists, inverse row maps,
        # normalised adjacencies) stays alive with this object, whatever the caches evict later (_cache.pinning)
        with _cache.pinning() as self._pinned:
            # warm-up on a side stream (allocator, optimizer state, cached structures), as graph capture requires
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), self._installed():
                for i in range(warmup):
                    self._refresh(require_fit=True)
                    if i == warmup - 1:
                        # the step about to be captured must not contain a long torch reduction (see _audit.py: their semaphore memset
                        # node was seen not to take effect in replays -- outputs silently stale)
                        with CaptureAudit() as audit:
                            body()
                        audit.check(what)
                    else:
                        body()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            # The graph is KEPT after capture and read back through the HIP runtime before it is instantiated (``_check_graph``): a
            # memset / memcpy / host node is what an ATen operator with hidden scratch traffic leaves behind (the semaphore memset of
            # a long reduction, sort / index_add_ / bincount scratch, zero_() on some paths) -- the class of node that was seen not to
            # take effect in replays (_audit.py).  Structural and always on: it also catches operators CaptureAudit's name list does
            # not know.
            self.graph = torch.cuda.CUDAGraph(keep_graph=True)
            with self._installed():
                self._refresh(require_fit=True)
                torch.cuda.synchronize(dev)
                with torch.cuda.graph(self.graph, capture_error_mode=self.capture_error_mode):
                    outs = body()
            self.node_kinds = self._check_graph()
            self.graph.instantiate()
            torch.cuda.synchronize(dev)
            self._refresh()                                    # randomness of the first replay
        return outs

    def _draw(self, require_fit: bool = False):
        """The per-step host randomness (the reference's one ``np.random.choice`` per step, the dropout seed), drawn into
        pinned staging buffers.  ``require_fit``: warm-up / capture (see dist.ShardedGraphedEpoch._draw_pick)."""
        if self._uploaded is not None:
            self._uploaded.synchronize()     # the previous upload has read the pinned buffers (it sits in front of the replay: microseconds)
        self._draw_pick(require_fit)
        self._seed_host.random_()
        self._seed_host.bitwise_and_(0x3FFFFFFFFFFFFFFF)

    def _upload(self):
        """Staging buffers -> the static device buffers the captured kernels read (stream-ordered: after the last replay)."""
        self._upload_pick()
        self._seed_dev.copy_(self._seed_host, non_blocking=True)
        # only stream-ordered: ``_draw`` must not rewrite the pinned buffers before the DMA has read them
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()

    def _refresh(self, require_fit: bool = False):
        self._draw(require_fit)
        self._upload()

    def redraw(self):
        """Discard the randomness prepared for the next replay and draw it again (after re-seeding NumPy / torch)."""
        torch.cuda.current_stream().synchronize()
        self._refresh()

    def step(self):
        """Replay one epoch; returns ((loss, loss_cls, loss_aux), (train, valid, test accuracies) | None).  The host draw for
        the NEXT step (np.random.choice of 16 384 of 90 941 rows costs ~1 ms) runs while this replay executes."""
        if self._pending is not None:
            raise RuntimeError(f"{type(self).__name__}.step() after step_async(): call drain() first (an epoch's values are still in flight)")
        res = self._launch()
        self._draw()                                            # overlapped with the replay; uploaded after the read below
        vals = self._decode(res.cpu())                          # one device->host read per epoch
        self._upload()
        return vals

    # -- the loop without an idle GPU between epochs --------------------------------------------------------------------------------
    # ``step()`` reads the epoch's values right after its replay: the GPU idles from the end of replay k until the host has woken up,
    # uploaded the next draw and launched replay k + 1 (measured on the headline workload: 0.3-0.4 ms of a 7.2 ms epoch).  Nothing in
    # replay k + 1 depends on the VALUES of epoch k (the row sample and the dropout seed are host draws; gnn.py:333-340 only logs the
    # losses and accuracies), so ``step_async()`` launches replay k first and reads the values of epoch k - 1 afterwards: same
    # replays, same draws in the same order, every epoch's values still read by the host -- one call later.
    def _values(self, slot):
        self._res_done[slot].synchronize()
        return self._decode(self._res_host[slot])

    def step_async(self):
        """Launch one epoch and return the values of the PREVIOUS ``step_async`` epoch (None on the first call): the randomness of this
        replay was drawn during the previous one and is uploaded stream-ordered in front of it; its values travel to a pinned host
        slot behind it.  ``drain()`` hands out the values of the last epoch launched."""
        slot = self._k & 1
        self._k += 1
        if self.replay_events is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        res = self._launch()
        if self.replay_events is not None:
            e1.record()
            self.replay_events.append((e0, e1))
        self._res_host[slot].copy_(res, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._res_done[slot] = done
        self._draw()                      # host draw of the NEXT epoch, overlapped with this replay
        self._upload()                    # stream-ordered behind this replay: the static buffers change after it has read them
        prev, self._pending = self._pending, slot
        return None if prev is None else self._values(prev)

    def drain(self):
        """Values of the last epoch launched by ``step_async`` (None if they were handed out already)."""
        prev, self._pending = self._pending, None
        return None if prev is None else self._values(prev)


class GraphedEpoch(ReplayedEpoch):
    """One epoch of the reference loop (gnn.py:333-340: ``train()`` then ``test()``) captured ONCE as a hipGraph and
    replayed: the ~180 kernel launches of an epoch are enqueued by one call, the GPU never waits for the host between
    them.  Same kernels, same arithmetic, same RNG coupling as ``train_step`` + ``evaluate``:
      * the G-CRD / GSP row sample is still ONE ``np.random.choice`` per step on the host (criterion.py:63,135); it is
        uploaded into a static device buffer the captured kernels read (``criterion._ROW_SAMPLER``);
      * dropout masks change every replay: the kernels add a per-step seed that lives in device memory
        (``ops._DROPOUT_SEED_DEV``), drawn from torch's host generator like the eager path;
      * losses / accuracies are read back once per epoch from static output tensors.
    Needs ``torch.optim.Adam(..., capturable=True)`` (fused or not).  ``split_idx=None`` captures the train step only."""

    def __init__(self, model, x, adj_t, y, train_idx, optimizer, mode, hp, teacher_out_feat=None, teacher_logits=None,
                 student_proj=None, teacher_proj=None, edge_index=None, split_idx=None, kd_and_aux=False, warmup=3):
        if not x.is_cuda:
            raise ValueError("GraphedEpoch needs GPU tensors")
        self.mode, self.hp = mode, hp
        self.n_train = train_idx.numel()
        S = hp.get("max_samples", 0) if mode in ("nce", "gpw") else 0
        dev = x.device
        # the epoch's six scalars side by side in ONE 40-byte device buffer (three float32 losses at byte 0, three float64 accuracies at
        # byte 16), written by the kernels that produce them: one device->host copy per epoch, no gather launch
        super().__init__(dev, S if 0 < S < self.n_train else 0, 40, torch.uint8)
        args = (model, x, adj_t, y, train_idx, optimizer, mode, hp, teacher_out_feat, teacher_logits, student_proj, teacher_proj,
                edge_index, kd_and_aux)
        self._res_bytes = torch.zeros(40, dtype=torch.uint8, device=dev)
        res_losses, res_accs = self._res_bytes[:12].view(torch.float32), self._res_bytes[16:].view(torch.float64)

        def body():
            losses = train_step_tensors(*args, out=res_losses)
            if split_idx is None:
                return losses, None, None
            out, accs = evaluate_tensors(model, x, adj_t, y, split_idx, accs_out=res_accs)
            return losses, out, accs
        self._body = body
        self.losses, self.out, self.accs = self._capture(body, dev, warmup)

    def _check_graph(self):
        # the single-GPU epoch is a chain of kernel nodes only
        from ._audit import check_captured_graph
        return check_captured_graph(self.graph, "GraphedEpoch", kernels_only=True)

    @contextlib.contextmanager
    def _installed(self):
        prev = (C._ROW_SAMPLER, ops._DROPOUT_SEED_DEV)

        def sampler(n, S, device):
            if S >= n:
                return None
            if n != self.n_train or S != self.n_pick:
                raise RuntimeError(f"GraphedEpoch was captured for {self.n_pick} of {self.n_train} rows, the criterion asks for {S} of {n}")
            return self._pick_dev
        C._ROW_SAMPLER, ops._DROPOUT_SEED_DEV = sampler, self._seed_dev
        try:
            yield
        finally:
            C._ROW_SAMPLER, ops._DROPOUT_SEED_DEV = prev

    def _draw_pick(self, require_fit):
        if self.n_pick:
            import numpy as np
            self._pick_host.copy_(torch.from_numpy(np.random.choice(self.n_train, self.n_pick, replace=False)))

    def _upload_pick(self):
        if self.n_pick:
            self._pick_dev.copy_(self._pick_host, non_blocking=True)

    def _launch(self):
        self.graph.replay()
        return self._res_bytes

    def _decode(self, host_bytes):
        losses = tuple(host_bytes[:12].view(torch.float32).tolist())
        return (losses, None) if self.accs is None else (losses, tuple(host_bytes[16:].view(torch.float64).tolist()))


class GAT(nn.Module):
    """The PPI GAT model (/root/reference/ppi_pyg/gnn.py:86-117, ``--gnn gat``), run frozen inside the student step (:208-209)
    or trained: GATConv + linear skip per layer, ELU, dropout; the last layer averages its heads."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, heads=4):
        super().__init__()
        self.convs = nn.ModuleList([GATConv(in_channels, hidden_channels, heads=heads)])
        self.lins = nn.ModuleList([nn.Linear(in_channels, hidden_channels * heads)])
        for _ in range(num_layers - 2):
            self.convs.append(GATConv(heads * hidden_channels, hidden_channels, heads=heads))
            self.lins.append(nn.Linear(hidden_channels * heads, hidden_channels * heads))
        self.convs.append(GATConv(heads * hidden_channels, out_channels, heads=heads, concat=False))
        self.lins.append(nn.Linear(hidden_channels * heads, out_channels))
        self.dropout = dropout
        self.out_feat = None

    def reset_parameters(self):
        for m in list(self.convs) + list(self.lins):
            m.reset_parameters()

    def forward(self, x, adj_t):
        for conv, lin in zip(self.convs[:-1], self.lins[:-1]):
            x = conv(x, adj_t) + ops.linear(x, lin.weight, lin.bias)
            x = F.elu(x)
            x = F.dropout(x, p=self.dropout, training=self.training)
            self.out_feat = x
        return self.convs[-1](x, adj_t) + ops.linear(x, self.lins[-1].weight, self.lins[-1].bias)


class ElementWiseLinear(nn.Module):
    """/root/reference/arxiv_dgl/models.py:11-45 (state_dict keys ``weight`` / ``bias``)."""

    def __init__(self, size, weight=True, bias=True, inplace=False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(size)) if weight else None
        self.bias = nn.Parameter(torch.zeros(size)) if bias else None
        self.inplace = inplace

    def forward(self, x):
        if self.weight is not None:
            x = x * self.weight
        if self.bias is not None:
            x = x + self.bias
        return x


class ArxivGAT(nn.Module):
    """The arxiv GAT teacher (/root/reference/arxiv_dgl/models.py:239-313; ``gat.py`` builds it 3 layers x 250 x 3 heads,
    expt ``gat-3L250x3h``) on the kernels, for inference and (training mode, autograd on) for training -- same attribute names (``convs``, ``norms``, ``bias_last``), so the
    reference's ``checkpoints/<expt>/<seed>.pt['model_state_dict']`` loads.  ``self.feat`` = the last hidden features: the
    [N, 750] tensor the student reads as ``teacher_out_feat`` (arxiv_pyg/gnn.py:278)."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, n_heads, activation, dropout=0.0, input_drop=0.0, attn_drop=0.0,
                 edge_drop=0.0, use_attn_dst=True, use_symmetric_norm=False):
        super().__init__()
        self.in_feats, self.n_hidden, self.n_classes, self.n_layers, self.num_heads = in_feats, n_hidden, n_classes, n_layers, n_heads
        self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            in_hidden = n_heads * n_hidden if i > 0 else in_feats
            out_hidden = n_hidden if i < n_layers - 1 else n_classes
            num_heads = n_heads if i < n_layers - 1 else 1
            self.convs.append(DGLGATConv(in_hidden, out_hidden, num_heads=num_heads, attn_drop=attn_drop, edge_drop=edge_drop,
                                         use_attn_dst=use_attn_dst, use_symmetric_norm=use_symmetric_norm, residual=True))
            if i < n_layers - 1:
                self.norms.append(nn.BatchNorm1d(n_heads * out_hidden))
        self.bias_last = ElementWiseLinear(n_classes, weight=False, bias=True, inplace=True)
        self.input_drop, self.dropout, self.activation = nn.Dropout(input_drop), nn.Dropout(dropout), activation
        self.feat = None

    def forward(self, graph, feat):
        h = self.input_drop(feat)
        for i in range(self.n_layers):
            h = self.convs[i](graph, h)
            if i < self.n_layers - 1:
                h = h.flatten(1)
                bn = self.norms[i]
                fusable = h.is_cuda and ops.bn_shape_ok(h) and getattr(self.activation, "__name__", "") == "relu"
                if fusable and not self.training:
                    h = ops.bn_act(h, bn, relu=True, p=0.0, training=False)      # BatchNorm (running statistics) + ReLU fused
                elif fusable and torch.is_grad_enabled():
                    h = ops.bn_act(h, bn, relu=True, p=self.dropout.p, training=True)   # batch statistics + ReLU + dropout fused
                else:
                    h = self.dropout(self.activation(bn(h)))
                self.feat = h
        return self.bias_last(h.mean(1))


def add_labels(feat, labels, idx, n_classes):
    """gat.py:104-107: one-hot labels of ``idx`` appended to the features (zeros elsewhere)."""
    onehot = torch.zeros([feat.shape[0], n_classes], dtype=feat.dtype, device=feat.device)
    onehot[idx, labels[idx, 0]] = 1
    return torch.cat([feat, onehot], dim=-1)


ARXIV_GAT_EPSILON = 1 - math.log(2)


def arxiv_gat_loss(x, labels):
    """gat.py:98-101: mean of log(epsilon + CE) - log(epsilon) with epsilon = 1 - log 2 (``labels`` [n, 1])."""
    y = F.cross_entropy(x, labels[:, 0], reduction="none")
    return torch.mean(torch.log(ARXIV_GAT_EPSILON + y) - math.log(ARXIV_GAT_EPSILON))


def arxiv_gat_label_split(train_idx, mask_rate, mask=None):
    """gat.py:121-125: (train_labels_idx, train_pred_idx) -- the train nodes whose labels become input features (``rand < mask_rate``)
    and the rest, whose predictions carry the loss.  ``mask``: a recorded draw (bool, one per train node) instead of a fresh one."""
    if mask is None:
        mask = torch.rand(train_idx.shape) < mask_rate
    mask = mask.to(train_idx.device)
    return train_idx[mask], train_idx[~mask]


def arxiv_gat_adjust_learning_rate(optimizer, lr, epoch):
    """gat.py:110-113: linear warm-up over the first 50 epochs (epochs count from 1)."""
    if epoch <= 50:
        for group in optimizer.param_groups:
            group["lr"] = lr * epoch / 50


def arxiv_gat_train_step(model, graph, feat, labels, train_idx, val_idx, test_idx, optimizer, n_classes, use_labels=True,
                         n_label_iters=0, mask_rate=0.5, mask=None):
    """One teacher training step, gat.py:116-148: label masking by ``mask_rate``, the masked-in labels appended as input features
    (``add_labels``), ``n_label_iters`` label-reuse rounds (detached soft predictions written back for the unlabelled nodes, then
    another forward), the loss of gat.py:98-101 on the prediction rows, backward, optimizer step.  Returns (train accuracy, loss)."""
    model.train()
    if use_labels:
        train_labels_idx, train_pred_idx = arxiv_gat_label_split(train_idx, mask_rate, mask)
        feat = add_labels(feat, labels, train_labels_idx, n_classes)
    else:
        train_pred_idx = arxiv_gat_label_split(train_idx, mask_rate, mask)[0]
    optimizer.zero_grad()
    pred = model(graph, feat)
    if n_label_iters > 0:
        unlabel_idx = torch.cat([train_pred_idx, val_idx, test_idx])
        for _ in range(n_label_iters):
            pred = pred.detach()
            feat[unlabel_idx, -n_classes:] = F.softmax(pred[unlabel_idx], dim=-1)
            pred = model(graph, feat)
    loss = arxiv_gat_loss(pred[train_pred_idx], labels[train_pred_idx])
    loss.backward()
    optimizer.step()
    acc = (pred[train_idx].argmax(dim=-1, keepdim=True) == labels[train_idx]).float().mean()
    return float(acc), float(loss)


@torch.no_grad()
def teacher_evaluate(model, graph, feat, labels, train_idx, val_idx, test_idx, n_classes, use_labels=True, n_label_iters=0):
    """The producer of the teacher artefacts (gat.py:151-183 ``evaluate``): eval-mode forward with the train labels as input
    features and ``n_label_iters`` label-reuse rounds (soft predictions written back for the unlabelled nodes, :162-166).
    Returns (pred [N, C] -> ``logits/<expt>/<seed>.pt``, model.feat [N, heads * hidden] -> ``features/<expt>/<seed>.pt``;
    ``data.save_teacher_artifacts`` writes them in the reference's layout, gat.py:243-251)."""
    model.eval()
    if use_labels:
        feat = add_labels(feat, labels, train_idx, n_classes)
    pred = model(graph, feat)
    if n_label_iters > 0:
        unlabel_idx = torch.cat([val_idx, test_idx])
        for _ in range(n_label_iters):
            feat[unlabel_idx, -n_classes:] = F.softmax(pred[unlabel_idx], dim=-1)
            pred = model(graph, feat)
    return pred, model.feat


class TeacherNet(nn.Module):
    """The PPI teacher checkpointed by the reference (/root/reference/ppi_pyg/gnn.py:23-47, trained by ppi_pyg/train_teacher.py):
    4 x 256 GAT layers with linear skips, ELU, a 6-head averaging output layer; ``out_feat`` = second hidden.  Same attribute
    names (state_dict keys ``conv1.*``, ``lin1.*``, ...) so that the reference's ``checkpoint.pt`` loads."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = GATConv(in_channels, 256, heads=4)
        self.lin1 = nn.Linear(in_channels, 4 * 256)
        self.conv2 = GATConv(4 * 256, 256, heads=4)
        self.lin2 = nn.Linear(4 * 256, 4 * 256)
        self.conv3 = GATConv(4 * 256, out_channels, heads=6, concat=False)
        self.lin3 = nn.Linear(4 * 256, out_channels)
        self.out_feat = None

    def reset_parameters(self):
        for m in (self.conv1, self.conv2, self.conv3, self.lin1, self.lin2, self.lin3):
            m.reset_parameters()

    def forward(self, x, edge_index):
        x = F.elu(self.conv1(x, edge_index) + ops.linear(x, self.lin1.weight, self.lin1.bias))
        x = F.elu(self.conv2(x, edge_index) + ops.linear(x, self.lin2.weight, self.lin2.bias))
        self.out_feat = x
        return self.conv3(x, edge_index) + ops.linear(x, self.lin3.weight, self.lin3.bias)


class StudentNet(nn.Module):
    """The PPI GAT student (/root/reference/ppi_pyg/gnn.py:50-83, ``--gnn student``; the GAT-5L of the paper's PPI table): five
    GATConv layers of 2 heads x 68 with linear skips and ELU, the last one averaging its heads; ``out_feat`` = fourth hidden.
    Same attribute names (``conv1..5``, ``lin1..5``) and so the same state_dict keys as the reference."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = GATConv(in_channels, 68, heads=2)
        self.lin1 = nn.Linear(in_channels, 2 * 68)
        self.conv2 = GATConv(2 * 68, 68, heads=2)
        self.lin2 = nn.Linear(2 * 68, 2 * 68)
        self.conv3 = GATConv(2 * 68, 68, heads=2)
        self.lin3 = nn.Linear(2 * 68, 2 * 68)
        self.conv4 = GATConv(2 * 68, 68, heads=2)
        self.lin4 = nn.Linear(2 * 68, 2 * 68)
        self.conv5 = GATConv(2 * 68, out_channels, heads=2, concat=False)
        self.lin5 = nn.Linear(2 * 68, out_channels)
        self.out_feat = None

    def reset_parameters(self):
        for k in range(1, 6):
            getattr(self, f"conv{k}").reset_parameters()
        for k in range(1, 6):
            getattr(self, f"lin{k}").reset_parameters()

    def forward(self, x, edge_index):
        for k in range(1, 5):
            conv, lin = getattr(self, f"conv{k}"), getattr(self, f"lin{k}")
            x = F.elu(conv(x, edge_index) + ops.linear(x, lin.weight, lin.bias))
        self.out_feat = x
        return self.conv5(x, edge_index) + ops.linear(x, self.lin5.weight, self.lin5.bias)


class RGCN(nn.Module):
    """/root/reference/mag_pyg/gnn.py:71-168 on the kernels: ``forward`` on a (sampled) grouped subgraph through
    ``nn.RGCNConv``; ``inference`` full-batch, one rectangular mean-SpMM (``adj_t.matmul(x, reduce='mean')``, :151,162) and
    one GEMM per relation and layer.  The GraphSAINT sampler that feeds ``forward`` in the reference is ``saint.py``: its batches
    carry the per-relation structure (``batch.relations``), which ``forward(..., relations=)`` hands to every layer."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, num_nodes_dict, x_types, num_edge_types):
        super().__init__()
        self.in_channels, self.hidden_channels, self.out_channels = in_channels, hidden_channels, out_channels
        self.num_layers, self.dropout = num_layers, dropout
        node_types = list(num_nodes_dict.keys())
        self.num_node_types, self.num_edge_types = len(node_types), num_edge_types
        self.emb_dict = nn.ParameterDict({f"{key}": nn.Parameter(torch.empty(num_nodes_dict[key], in_channels))
                                          for key in sorted(set(node_types).difference(set(x_types)))})
        dims = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.convs = nn.ModuleList(RGCNConv(a, b, self.num_node_types, num_edge_types) for a, b in zip(dims[:-1], dims[1:]))
        self.out_feat = None
        self.reset_parameters()

    def reset_parameters(self):
        for emb in self.emb_dict.values():
            nn.init.xavier_uniform_(emb)
        for conv in self.convs:
            conv.reset_parameters()

    def group_input(self, x_dict, node_type, local_node_idx):
        from .optim import row_state
        if any([row_state(emb) is not None for emb in self.emb_dict.values()]):
            # tables under optim.LazyRowAdam: one gather launch that first catches the rows it reads up (their data is otherwise behind)
            sources = {int(k): x for k, x in x_dict.items()}
            sources.update((int(k), emb) for k, emb in self.emb_dict.items())
            return ops.group_input(sources, node_type, local_node_idx, self.in_channels)
        h = torch.zeros((node_type.size(0), self.in_channels), device=node_type.device)
        for key, x in x_dict.items():
            mask = node_type == key
            h[mask] = x[local_node_idx[mask]]
        for key, emb in self.emb_dict.items():
            mask = node_type == int(key)
            h[mask] = emb[local_node_idx[mask]]
        return h

    def forward(self, x_dict, edge_index, edge_type, node_type, local_node_idx, relations=None):
        x = self.group_input(x_dict, node_type, local_node_idx)
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index, edge_type, node_type, relations=relations)
            if i != self.num_layers - 1:
                x = F.dropout(F.relu(x), p=0.5, training=self.training)
                self.out_feat = x
        return x

    @torch.no_grad()
    def inference(self, x_dict, edge_index_dict, key2int):
        x_dict = dict(x_dict)
        for key, emb in self.emb_dict.items():
            from .optim import row_state
            rows = row_state(emb)
            if rows is not None:
                rows.flush()            # a table under optim.LazyRowAdam is read whole here: bring every row up to the current step
            x_dict[int(key)] = emb
        adj_t_dict = {}
        for key, (row, col) in edge_index_dict.items():
            n_dst, n_src = x_dict[key2int[key[-1]]].shape[0], x_dict[key2int[key[0]]].shape[0]
            adj_t_dict[key] = SparseTensor(row=col, col=row, sparse_sizes=(n_dst, n_src))   # unsorted constructor (mag:151)
        for i, conv in enumerate(self.convs):
            out_dict = {j: ops.linear(x, conv.root_lins[j].weight, conv.root_lins[j].bias) for j, x in x_dict.items()}
            for keys, adj_t in adj_t_dict.items():
                tmp = adj_t.matmul(x_dict[key2int[keys[0]]], reduce="mean")
                tgt = key2int[keys[-1]]
                out_dict[tgt] = out_dict[tgt] + ops.linear(tmp, conv.rel_lins[key2int[keys]].weight)
            if i != self.num_layers - 1:
                out_dict = {j: F.relu(v) for j, v in out_dict.items()}
            x_dict = out_dict
        return x_dict


PPI_MODES = ("supervised", "kd", "fitnet", "at", "gpw", "lpw", "nce")


def ppi_train_epoch(model, teacher_model, graphs, optimizer, mode, hp, student_proj=None, teacher_proj=None):
    """One PPI epoch (/root/reference/ppi_pyg/gnn.py:185-274): one optimisation step per batch graph; in every mode but
    ``supervised`` the frozen teacher's forward runs inside every step (:208-209).  ``graphs``: objects with x / edge_index / y.
    ``fitnet`` / ``nce`` pass ``model.out_feat`` and ``teacher_model.out_feat`` through ``student_proj`` / ``teacher_proj``
    (Linear + BatchNorm1d + ReLU, gnn.py:355-366: ``make_projection``); ``at`` / ``gpw`` / ``lpw`` compare them directly.
    ``hp``: alpha / kd_T (kd), beta, kernel (gpw / lpw), max_samples (gpw / nce), nce_T (nce).
    Returns the epoch means (loss, loss_cls, loss_aux) like the reference."""
    if mode not in PPI_MODES:
        raise NotImplementedError(mode)
    train_mode(model, student_proj, teacher_proj, teacher_model)
    tot = [0.0, 0.0, 0.0]
    for g in graphs:
        out = model(g.x, g.edge_index)
        if mode == "supervised":
            loss = F.binary_cross_entropy_with_logits(out, g.y)
            loss_cls, loss_aux = loss, loss * 0
        else:
            with torch.no_grad():
                teacher_out = teacher_model(g.x, g.edge_index)
                teacher_out_feat = teacher_model.out_feat
            f, t = model.out_feat, teacher_out_feat
            if mode in ("fitnet", "nce"):
                f, t = student_proj(f), teacher_proj(t)
            loss, loss_cls, loss_aux = C.distill(mode, out, g.y, f, t, hp, teacher_logits=teacher_out, edge_index=g.edge_index,
                                                 multilabel=True)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        for i, v in enumerate((loss, loss_cls, loss_aux)):
            tot[i] += v.detach().item()
    return tuple(v / max(1, len(graphs)) for v in tot)


@torch.no_grad()
def ppi_test(model, graphs):
    """Micro-F1 over all nodes and labels of ``graphs`` (/root/reference/ppi_pyg/gnn.py:277-288: predictions = logits > 0,
    sklearn ``f1_score(average='micro')``, 0 when nothing is predicted positive)."""
    model.eval()
    tp = fp = fn = 0.0
    for g in graphs:
        pred = (model(g.x, g.edge_index) > 0).float()
        y = g.y
        tp += float((pred * y).sum())
        fp += float((pred * (1 - y)).sum())
        fn += float(((1 - pred) * y).sum())
    if tp + fp == 0:
        return 0
    return 2 * tp / (2 * tp + fp + fn)


MAG_MODES = PPI_MODES


def mag_batch_loss(model, batch, x_dict, mode, hp, teacher_model=None, student_proj=None, teacher_proj=None):
    """``(loss, loss_cls, loss_aux)`` of one GraphSAINT batch: the loop body of /root/reference/mag_pyg/gnn.py:188-253.  Logits and
    labels on the rows ``batch.train_mask``; class-index cross entropy criteria (mag_pyg/criterion.py); in every mode but
    ``supervised`` the frozen teacher's forward runs under ``no_grad`` on the same batch, sharing ``batch.relations`` with the student.
    ``fitnet`` / ``nce`` pass the features through ``student_proj`` / ``teacher_proj`` (``make_projection``); ``at`` / ``gpw`` / ``lpw``
    compare ``out_feat`` directly (:226); ``lpw`` runs over the subgraph induced by the train rows (:237).  ``hp`` as in
    ``ppi_train_epoch``."""
    if mode not in MAG_MODES:
        raise NotImplementedError(mode)
    rel = getattr(batch, "relations", None)
    args = (x_dict, batch.edge_index, batch.edge_attr, batch.node_type, batch.local_node_idx)
    out = model(*args, relations=rel)
    rows = batch.train_mask.nonzero().view(-1)          # the rows [train_mask] of :191-192, picked inside the CE / KD kernels
    labels = batch.y.view(-1)
    if mode == "supervised":
        loss = ops.cross_entropy(out, labels, rows)
        return loss, loss, loss * 0
    with torch.no_grad():
        teacher_out = teacher_model(*args, relations=rel)
        teacher_feat = ops.take_rows(teacher_model.out_feat, rows)
    feat, edge_index = None, None
    if mode != "kd":
        feat = ops.take_rows(model.out_feat, rows)
    if mode in ("fitnet", "nce"):
        feat, teacher_feat = student_proj(feat), teacher_proj(teacher_feat)
    elif mode == "lpw":
        from .utils import subgraph
        edge_index = subgraph(rows, batch.edge_index, relabel_nodes=True, num_nodes=batch.num_nodes)[0]
    return C.distill(mode, out, labels, feat, teacher_feat, hp, teacher_logits=teacher_out, rows=rows, edge_index=edge_index)


def mag_accumulate_epoch(model, loader, x_dict, optimizer, mode, hp, teacher_model=None, student_proj=None, teacher_proj=None, accumulate=1,
                         seed=None):
    """``mag_train_epoch`` with ``accumulate`` consecutive batches per optimisation step, whose gradient is the MEAN of the batch-loss
    gradients (dense ones summed in ``.grad``, table rows as deposits of ``LazyRowAdam(duplicates="sum")``, both scaled by
    1 / (batches of the step); the last step of the epoch averages over the batches it has).  Needs an optimiser that takes several
    deposits per table: ``mag_optimizer(model, lr, duplicates="sum")`` or any dense optimiser; ``LazyRowAdam`` in its default mode
    raises before the first batch.  ``seed``: ``torch.manual_seed(seed + b)`` runs before the forward of batch number ``b`` of the
    epoch, so the dropout masks depend on the batch and not on how the batches are grouped.  ``accumulate=1, seed=None`` IS
    ``mag_train_epoch``.  Returns the epoch means weighted by train rows, like ``mag_train_epoch``."""
    from .optim import LazyRowAdam
    if mode not in MAG_MODES:
        raise NotImplementedError(mode)
    if int(accumulate) != accumulate or accumulate < 1:
        raise ValueError("mag_accumulate_epoch: accumulate must be a positive integer")
    if accumulate == 1 and seed is None:
        return mag_train_epoch(model, loader, x_dict, optimizer, mode, hp, teacher_model, student_proj, teacher_proj)
    train_mode(model, student_proj, teacher_proj, teacher_model)
    lazy_sum = isinstance(optimizer, LazyRowAdam) and optimizer.duplicates == "sum"
    if accumulate > 1 and isinstance(optimizer, LazyRowAdam) and not lazy_sum:
        raise ValueError("mag_accumulate_epoch: accumulate > 1 deposits several gradient lists per table and step; build the optimiser with "
                         "mag_optimizer(model, lr, duplicates='sum')")
    tot, examples = [0.0, 0.0, 0.0], 0
    dev = next(model.parameters()).device

    def step(k):
        scale = 1.0 / k
        if k > 1:
            grads = [p.grad for group in optimizer.param_groups for p in group["params"] if p.grad is not None]
            if grads:
                torch._foreach_mul_(grads, scale)           # one call for all dense gradients
        if lazy_sum:
            optimizer.step(grad_scale=scale)
        else:
            optimizer.step()

    pending = 0
    for b, batch in enumerate(loader):
        batch = batch.to(dev)
        if pending == 0:
            optimizer.zero_grad()
        if seed is not None:
            torch.manual_seed(seed + b)
        loss, loss_cls, loss_aux = mag_batch_loss(model, batch, x_dict, mode, hp, teacher_model, student_proj, teacher_proj)
        loss.backward()
        pending += 1
        if pending == accumulate:
            step(pending)
            pending = 0
        vals = torch.stack([loss.detach(), loss_cls.detach(), loss_aux.detach(), batch.train_mask.sum().to(loss.dtype)]).tolist()
        n = int(vals[3])
        for i in range(3):
            tot[i] += vals[i] * n
        examples += n
    if pending:
        step(pending)                   # the last step of the epoch averages over the batches it has
    flush = getattr(optimizer, "flush", None)
    if flush is not None:
        flush()
    return tuple(v / max(1, examples) for v in tot)


def mag_train_epoch(model, loader, x_dict, optimizer, mode, hp, teacher_model=None, student_proj=None, teacher_proj=None):
    """One MAG epoch (/root/reference/mag_pyg/gnn.py:174-268): one optimisation step per GraphSAINT batch of ``loader``
    (``saint.GraphSAINTRandomWalkSampler`` or any iterable of batches); returns the epoch means of (loss, loss_cls, loss_aux) weighted
    by the number of train rows of each batch, like the reference."""
    if mode not in MAG_MODES:
        raise NotImplementedError(mode)
    train_mode(model, student_proj, teacher_proj, teacher_model)
    tot, examples = [0.0, 0.0, 0.0], 0
    dev = next(model.parameters()).device
    for batch in loader:
        batch = batch.to(dev)
        loss, loss_cls, loss_aux = mag_batch_loss(model, batch, x_dict, mode, hp, teacher_model, student_proj, teacher_proj)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        vals = torch.stack([loss.detach(), loss_cls.detach(), loss_aux.detach(), batch.train_mask.sum().to(loss.dtype)]).tolist()
        n = int(vals[3])
        for i in range(3):
            tot[i] += vals[i] * n
        examples += n
    flush = getattr(optimizer, "flush", None)
    if flush is not None:
        flush()                         # optim.LazyRowAdam: after the epoch the tables are what dense Adam would hold
    return tuple(v / max(1, examples) for v in tot)


def mag_optimizer(model, lr, duplicates="refuse"):
    """The reference's ``torch.optim.Adam(model.parameters(), lr=lr)`` (mag_pyg/gnn.py:424) with the embedding tables stepped row-lazily
    (``optim.LazyRowAdam``): same parameters, but a step moves the ~55 k rows of the batch instead of all 1.2 M, and no dense table
    gradient is formed.  Between flushes ``emb.data`` holds rows that are behind; ``RGCN.forward`` / ``inference`` / ``mag_train_epoch``
    catch up or flush what they read.  ``duplicates="sum"``: a step takes the rows of several batches (``mag_accumulate_epoch``,
    ``dist.mag_dp_train_epoch``) and sums the gradient rows of a table row named more than once."""
    from .optim import LazyRowAdam
    return LazyRowAdam(model.parameters(), lr=lr, lazy=list(model.emb_dict.values()), duplicates=duplicates)


@torch.no_grad()
def mag_test(model, x_dict, edge_index_dict, key2int, y_paper, split_idx):
    """``test()`` of /root/reference/mag_pyg/gnn.py:271-294: full-batch ``model.inference``, argmax over the paper rows, the three
    accuracies (train, valid, test) through ``accuracy``.  ``split_idx``: {'train' | 'valid' | 'test': paper ids, or the reference's
    nested {'paper': ids}}."""
    model.eval()
    out = model.inference(x_dict, edge_index_dict, key2int)[key2int["paper"]]
    y_pred = out.argmax(dim=-1, keepdim=True)
    y_true = y_paper.to(y_pred.device).view(-1, 1)
    accs = []
    for k in ("train", "valid", "test"):
        idx = split_idx[k]
        idx = (idx["paper"] if isinstance(idx, dict) else idx).to(y_pred.device)
        accs.append(accuracy(y_true[idx], y_pred[idx]))
    return tuple(accs)


# ------------------------------------------------------------------------------------------------
# SIGN student (/root/reference/arxiv_dgl/sign.py): graph-agnostic MLP over pre-averaged hop features
# ------------------------------------------------------------------------------------------------
class FeedForwardNet(nn.Module):
    """sign.py:105-133: ``n_layers`` Linear layers with one shared PReLU + dropout between them (same constructor, attribute names,
    state_dict keys and initial values under a torch seed).  The forward runs the MFMA GEMM and the fused PReLU + dropout kernel."""

    def __init__(self, in_feats, hidden, out_feats, n_layers, dropout):
        super().__init__()
        self.layers = nn.ModuleList()
        self.n_layers = n_layers
        if n_layers == 1:
            self.layers.append(nn.Linear(in_feats, out_feats))
        else:
            self.layers.append(nn.Linear(in_feats, hidden))
            for i in range(n_layers - 2):
                self.layers.append(nn.Linear(hidden, hidden))
            self.layers.append(nn.Linear(hidden, out_feats))
        if self.n_layers > 1:
            self.prelu = nn.PReLU()
            self.dropout = nn.Dropout(dropout)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        for layer in self.layers:
            nn.init.xavier_uniform_(layer.weight, gain=gain)
            nn.init.zeros_(layer.bias)

    def forward(self, x):
        for layer_id, layer in enumerate(self.layers):
            x = ops.linear(x, layer.weight, layer.bias)
            if layer_id < self.n_layers - 1:
                x = ops.prelu_drop(x, [self.prelu.weight], x.shape[1], self.dropout.p, self.training)
        return x


class SIGN(nn.Module):
    """sign.py:136-162.  ``forward(feats)`` is the reference's call (a list of already-gathered [B, F] hop features);
    ``forward_rows(feats, batch)`` takes the full [N, F] hop features and the batch's row ids and never materialises ``x[batch]``.
    The level-l activations of ALL hops live in one [B, H*hidden] buffer: every hop's GEMM writes its column block, one
    ``ops.prelu_drop`` launch per level serves all hops, the last per-hop GEMMs write the concatenation itself (no torch.cat).
    Dropout seeds are drawn in the reference's dropout call order: input drop of hops 0..H-1; hop by hop, that hop's hidden levels
    in layer order; the concatenation; ``project``'s hidden levels."""

    def __init__(self, in_feats, hidden, out_feats, num_hops, n_layers, dropout, input_drop):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.prelu = nn.PReLU()
        self.inception_ffs = nn.ModuleList()
        self.input_drop = nn.Dropout(input_drop)
        for hop in range(num_hops):
            self.inception_ffs.append(FeedForwardNet(in_feats, hidden, hidden, n_layers, dropout))
        self.project = FeedForwardNet(num_hops * hidden, hidden, out_feats, n_layers, dropout)

    def reset_parameters(self):
        for ff in self.inception_ffs:
            ff.reset_parameters()
        self.project.reset_parameters()

    def forward(self, feats):
        return self.forward_rows(feats, None)

    def forward_rows(self, feats, batch):
        """``self([x[batch] for x in feats])``.  ``batch``: int64 row ids on the device, a ``range`` (contiguous rows: a slice), or
        None (every row).  Training with ``input_drop > 0``: gather + input dropout of all hops in one launch
        (``ops.sign_gather_drop``); otherwise the first GEMM of every hop gathers in its operand load and no gather pass runs."""
        feats = list(feats)
        ffs = list(self.inception_ffs)
        H = len(ffs)
        if len(feats) != H:
            raise ValueError(f"SIGN: expected {H} hop feature matrices, got {len(feats)}")
        _lib.require_gpu(*feats)
        training = self.training
        if training and self.input_drop.p > 0:
            if batch is None or isinstance(batch, range):
                lo, hi = (0, feats[0].shape[0]) if batch is None else (batch.start, batch.stop)
                batch = torch.arange(lo, hi, dtype=torch.int64, device=feats[0].device)
            x, rows = ops.sign_gather_drop(feats, batch, self.input_drop.p, True), None
        else:
            x, rows = feats, batch
        L = ffs[0].n_layers
        drop = training and L > 1 and ffs[0].dropout.p > 0
        seeds = [[ops._draw_dropout_seed() for _ in range(L - 1)] for _ in range(H)] if drop else None
        cat_seed = [ops._draw_dropout_seed()] if training and self.dropout.p > 0 else None
        for l in range(L):
            z = ops.linear_blocks(x, [ff.layers[l].weight for ff in ffs], [ff.layers[l].bias for ff in ffs], rows)
            rows = None
            if l < L - 1:
                x = ops.prelu_drop(z, [ff.prelu.weight for ff in ffs], z.shape[1] // H, ffs[0].dropout.p, training,
                                   seeds=[s[l] for s in seeds] if drop else None)
        self.out_feat = ops.prelu_drop(z, [self.prelu.weight], z.shape[1], self.dropout.p, training, seeds=cat_seed)
        return self.project(self.out_feat)


def make_sign_projections(num_hidden, num_hops, proj_dim, teacher_dim=750):
    """(student_proj, teacher_proj) of sign.py:421-432: Linear + BatchNorm1d + ReLU heads over the concatenated hop features
    (``num_hidden * num_hops`` wide) and over the teacher's features; same construction order, so the same values under a torch seed."""
    return ProjectionHead(num_hidden * num_hops, proj_dim), ProjectionHead(teacher_dim, proj_dim)


SIGN_MODES = ("supervised", "kd", "fitnet", "at", "gpw", "nce")


def sign_batch_loss(model, feats, labels, batch, mode, hp, teacher_out_feat=None, teacher_logits=None, student_proj=None,
                    teacher_proj=None, kd_and_aux=True):
    """``(loss, loss_cls, loss_aux)`` of one mini-batch: the loop body of sign.py:307-369 (``kd_and_aux``: the KD loss plus
    ``beta * loss_aux``, what ``run`` calls) or of :235-277.  ``loss_cls`` / ``loss_aux`` are None where the reference leaves them so."""
    if mode not in SIGN_MODES:
        raise NotImplementedError(mode)
    logits = model.forward_rows(feats, batch)
    y = labels.view(-1)[batch]
    if mode == "supervised":
        return ops.cross_entropy(logits, y), None, None
    f = t = None
    if mode == "at":
        f, t = model.out_feat, teacher_out_feat[batch]
    elif mode != "kd":
        f = student_proj(model.out_feat)
        t = teacher_proj.forward_rows(teacher_out_feat, batch) if hasattr(teacher_proj, "forward_rows") else teacher_proj(teacher_out_feat[batch])
    kd_term = mode == "kd" or kd_and_aux
    return C.distill(mode, logits, y, f, t, hp, teacher_logits=teacher_logits[batch] if kd_term else None, kd_and_aux=kd_and_aux)


def sign_train_epoch(model, feats, labels, optimizer, batches, mode, hp, teacher_out_feat=None, teacher_logits=None,
                     student_proj=None, teacher_proj=None, kd_and_aux=True):
    """One SIGN training epoch: one optimisation step per index tensor of ``batches`` (the reference's ``train_loader``).
    ``kd_and_aux=True``: ``train_kd_and_aux`` (sign.py:293-382, what ``run`` calls); False: ``train`` (:221-290).  Returns the
    reference's three means over the steps (unweighted; ``loss_cls`` / ``loss_aux`` count as 0 where the reference leaves them None).
    The per-step scalars stay on the device and are read once, at the end of the epoch."""
    if mode not in SIGN_MODES:
        raise NotImplementedError(mode)
    train_mode(model, student_proj, teacher_proj)
    dev = labels.device
    _lib.require_gpu(labels, *feats)
    steps = []
    for batch in batches:
        batch = batch.to(dev)
        loss, loss_cls, loss_aux = sign_batch_loss(model, feats, labels, batch, mode, hp, teacher_out_feat, teacher_logits,
                                                   student_proj, teacher_proj, kd_and_aux)
        optimizer.zero_grad()
        loss.backward(gradient=_one_like(loss))
        optimizer.step()
        zero = loss.detach() * 0
        steps.append(torch.stack([loss.detach(), zero if loss_cls is None else loss_cls.detach(),
                                  zero if loss_aux is None else loss_aux.detach()]))
    if not steps:
        raise ValueError("sign_train_epoch: `batches` is empty")
    a, b, c = torch.stack(steps).double().mean(0).tolist()
    return a, b, c


def _as_range(batch):
    """``range(start, stop)`` for a HOST index tensor that lists consecutive rows (the reference's test_loader over ``torch.arange``:
    checked on the host, no device read), else None."""
    if torch.is_tensor(batch) and not batch.is_cuda and batch.dim() == 1 and batch.numel() > 0:
        start, n = int(batch[0]), batch.numel()
        if int(batch[-1]) == start + n - 1 and bool((batch[1:] - batch[:-1] == 1).all()):
            return range(start, start + n)
    return None


@torch.no_grad()
def sign_test(model, feats, labels, eval_batches, train_nid, val_nid, test_nid):
    """``test()`` of sign.py:385-401: batch-wise eval-mode forward over ``eval_batches`` (the reference's ``test_loader``, which covers
    rows 0..N-1 in order; a batch of consecutive rows is read as a slice), the logits written batch by batch into one [N, classes]
    tensor, then argmax + the three accuracies in one pass (``ops.split_accuracy``).  Returns ``(logits, (train, val, test))``."""
    model.eval()
    dev = labels.device
    _lib.require_gpu(labels, *feats)
    parts = []
    for batch in eval_batches:
        rng = batch if isinstance(batch, range) else _as_range(batch)
        parts.append(model.forward_rows(feats, rng if rng is not None else batch.to(dev)))
    logits = torch.cat(parts, dim=0)
    split = {"train": train_nid.to(dev), "valid": val_nid.to(dev), "test": test_nid.to(dev)}
    accs = ops.split_accuracy(logits, labels.view(-1), split)
    return logits, tuple(accs.tolist())


# ------------------------------------------------------------------------------------------------
# graph classification on batches of molecule-sized graphs (the README's fourth benchmark; mol_pyg holds a README only, so the
# layer stack restates OGB's public mol example [ext])
# ------------------------------------------------------------------------------------------------
MOL_MODES = ("supervised", "kd")
_MOL_POOLS = {"mean": global_mean_pool, "add": global_add_pool, "sum": global_add_pool, "max": global_max_pool}


class MolGNN(nn.Module):
    """GIN / GIN-E student for molecule batches [ext]: an atom encoder, ``num_layers`` x (conv -> BatchNorm1d -> relu (not after the last
    layer) -> dropout), a graph-level pool and ``Linear(emb_dim, 1)``.  ``conv="gine"``: ``nn.GINEConv`` on a per-layer bond
    embedding (one fused gather-add-relu-aggregate walk per layer); ``conv="gin"``: ``nn.GINConv``, the bonds' attributes unread.
    Each conv's MLP is Linear(emb, 2 emb) -> BatchNorm1d -> ReLU -> Linear(2 emb, emb).  State_dict keys: ``atom_encoder.*``,
    ``bond_encoders.l.*`` (gine), ``convs.l.nn.*`` / ``convs.l.eps``, ``bns.l.*``, ``graph_pred_linear.*``.  ``forward(batch)`` takes a
    ``saint.Batch`` (x [N, 9] and edge_attr [E, 3] int64, edge_index, batch, num_graphs) and returns logits [G, 1]; the pooled graph
    embedding stays in ``out_feat``, the side channel the criteria read."""

    def __init__(self, conv: str = "gin", num_layers: int = 5, emb_dim: int = 300, dropout: float = 0.5, pool: str = "mean",
                 atom_dims=ATOM_DIMS, bond_dims=BOND_DIMS):
        super().__init__()
        if conv not in ("gin", "gine"):
            raise ValueError(f"MolGNN: conv must be 'gin' or 'gine', got {conv!r}")
        if pool not in _MOL_POOLS:
            raise ValueError(f"MolGNN: pool must be one of {sorted(_MOL_POOLS)}, got {pool!r}")
        if num_layers < 1:
            raise ValueError("MolGNN: num_layers must be at least 1")
        self.conv, self.num_layers, self.emb_dim, self.dropout, self.pool = conv, int(num_layers), int(emb_dim), float(dropout), pool
        self.atom_encoder = CategoricalEncoder(atom_dims, emb_dim)
        if conv == "gine":
            self.bond_encoders = nn.ModuleList(CategoricalEncoder(bond_dims, emb_dim) for _ in range(num_layers))
        mlp = lambda: nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.BatchNorm1d(2 * emb_dim), nn.ReLU(),   # noqa: E731
                                    nn.Linear(2 * emb_dim, emb_dim))
        layer = GINEConv if conv == "gine" else GINConv
        self.convs = nn.ModuleList(layer(mlp()) for _ in range(num_layers))
        self.bns = nn.ModuleList(nn.BatchNorm1d(emb_dim) for _ in range(num_layers))
        self.graph_pred_linear = nn.Linear(emb_dim, 1)
        self.out_feat = None

    def reset_parameters(self):
        self.atom_encoder.reset_parameters()
        for m in list(getattr(self, "bond_encoders", [])) + list(self.convs) + list(self.bns) + [self.graph_pred_linear]:
            m.reset_parameters()

    def forward(self, batch):
        h = self.atom_encoder(batch.x)
        for l, (conv, bn) in enumerate(zip(self.convs, self.bns)):
            if self.conv == "gine":
                h = conv(h, batch.edge_index, self.bond_encoders[l](batch.edge_attr))
            else:
                h = conv(h, batch.edge_index)
            h = bn(h)
            if l != self.num_layers - 1:
                h = F.relu(h)
            h = F.dropout(h, p=self.dropout, training=self.training)
        self.out_feat = _MOL_POOLS[self.pool](h, batch.batch, batch.num_graphs)
        return self.graph_pred_linear(self.out_feat)


def mol_batch_loss(model, batch, mode, hp, teacher_logits=None):
    """``(loss, loss_cls, loss_aux)`` of one batch of graphs: ``supervised`` (mean BCE-with-logits on ``batch.y`` [G, 1]) and ``kd``
    (the multi-label KD of ``dropin/ppi_pyg/criterion.py``: ``hp`` alpha / kd_T, ``teacher_logits`` [G, 1]).  Other modes:
    ``NotImplementedError(mode)``."""
    if mode not in MOL_MODES:
        raise NotImplementedError(mode)
    if mode == "kd" and teacher_logits is None:
        raise ValueError("mol_batch_loss: mode 'kd' needs `teacher_logits`")
    out = model(batch)
    y = batch.y.to(out.dtype).view(out.shape)
    if mode == "supervised":
        loss = F.binary_cross_entropy_with_logits(out, y)
        return loss, loss, loss * 0
    return C.ppi_kd_criterion(out, y, teacher_logits.view(out.shape), hp["alpha"], hp["kd_T"])
