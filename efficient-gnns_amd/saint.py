"""``torch_geometric.data.GraphSAINTRandomWalkSampler`` formed on the device (/root/reference/mag_pyg/gnn.py:361-366).

The reference samples in DataLoader workers on the CPU (``torch_sparse::random_walk``, ``SparseTensor.saint_subgraph``) and ships
every batch over PCIe; here the grouped graph lives on the GPU and a batch is a handful of launches of ``csrc/saint.hip``:
random walk -> flag scan / ascending node list -> induced sub-matrix of the (row, col)-sorted parent (entries in parent order, so
the result equals ``saint_subgraph``) -> attribute gather.  The same induced-sub-matrix kernels over a second, relation-major copy
of the graph give the per-edge-type CSRs ``nn.RGCNConv`` aggregates over (``batch.relations``), which ``RGCNConv._relations`` would
otherwise rebuild with one ``nonzero`` + one sort per edge type and batch.

One device->host read per batch: ``(n_sub, e_sub, per-relation entry offsets, per-node-type row bounds)`` in one small copy, taken
after both count passes are enqueued and before the outputs are allocated (``sample``: the ``.tolist()``).
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from .sparse import SparseTensor, _ind2ptr

_BATCH_KEY_STEP = 1 << 32   # own draws: batch k hashes under the key seed + (k << 32), i.e. k enters the hash's high seed word


class Data:
    """Attribute container with the constructor of ``torch_geometric.data.Data`` (mag_pyg/gnn.py:349-357)."""

    def __init__(self, **kwargs):
        self.num_nodes = None
        for k, v in kwargs.items():
            setattr(self, k, v)

    def to(self, device):
        for k, v in list(vars(self).items()):
            if isinstance(v, Tensor):
                setattr(self, k, v.to(device))
        return self


class Batch(Data):
    """``torch_geometric.data.Batch`` for graph-level tasks: many small graphs as ONE disconnected graph."""

    @classmethod
    def from_data_list(cls, graphs):
        """``x`` / ``edge_attr`` / ``y`` concatenated, every graph's ``edge_index`` offset by the nodes before it, ``batch`` [N] int64
        (the graph id of every node, ascending), ``ptr`` [G + 1] (node offsets) and ``num_graphs``.  Plain torch ops on whatever
        device the graphs are on; a graph without edges or without nodes is legal (its id then owns no node).  A graph's node count is
        ``x.shape[0]``, else its ``num_nodes``.  An attribute is kept only when every graph has it."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("Batch.from_data_list: an empty list of graphs")

        def nodes(g):
            x = getattr(g, "x", None)
            if isinstance(x, Tensor):
                return int(x.shape[0])
            n = getattr(g, "num_nodes", None)
            if n is None:
                raise ValueError("Batch.from_data_list: a graph has neither `x` nor `num_nodes`")
            return int(n)

        sizes = [nodes(g) for g in graphs]
        offsets = [0]
        for n in sizes:
            offsets.append(offsets[-1] + n)
        first = next((getattr(g, k) for g in graphs for k in ("edge_index", "x", "y") if isinstance(getattr(g, k, None), Tensor)), None)
        device = first.device if first is not None else torch.device("cpu")
        out = cls()
        for key in ("x", "edge_attr", "y"):
            parts = [getattr(g, key, None) for g in graphs]
            if all(isinstance(p, Tensor) for p in parts):
                setattr(out, key, torch.cat(parts, dim=0))
        edges = [getattr(g, "edge_index", None) for g in graphs]
        if all(isinstance(e, Tensor) for e in edges):
            out.edge_index = torch.cat([e + off for e, off in zip(edges, offsets)], dim=1)
        out.ptr = torch.tensor(offsets, dtype=torch.int64, device=device)
        out.batch = torch.repeat_interleave(torch.arange(len(graphs), dtype=torch.int64, device=device),
                                            torch.tensor(sizes, dtype=torch.int64, device=device), output_size=offsets[-1])
        out.num_graphs, out.num_nodes = len(graphs), offsets[-1]
        return out


class SaintBatch:
    """One sampled subgraph: the fields ``train()`` of the reference reads (mag_pyg/gnn.py:187-192) plus ``node_idx`` / ``edge_idx``
    (ids in the parent graph) and ``relations`` (what ``RGCNConv._relations`` returns for this batch; None when the parent has
    no ``edge_attr`` / ``node_type``)."""

    _TENSORS = ("edge_index", "edge_attr", "node_type", "local_node_idx", "y", "train_mask", "node_idx", "edge_idx")

    def __init__(self, **kw):
        self.relations = None
        self.walks = None
        for k in self._TENSORS:
            setattr(self, k, None)
        for k, v in kw.items():
            setattr(self, k, v)

    def to(self, device, *_, **__):
        device = torch.device(device)
        here = self.node_idx.device
        if device == here or (device.type == here.type and device.index is None):
            return self
        out = SaintBatch(num_nodes=self.num_nodes)
        for k in self._TENSORS + ("walks",):
            v = getattr(self, k)
            setattr(out, k, None if v is None else v.to(device))
        if self.relations is not None:
            adjs, rows = self.relations
            out.relations = ([None if a is None else a.to(device) for a in adjs], [r.to(device) for r in rows])
        return out


class GraphSAINTRandomWalkSampler:
    """``GraphSAINTRandomWalkSampler(data, batch_size, walk_length, num_steps, sample_coverage=0)``: iterating yields ``num_steps``
    ``SaintBatch`` objects, each the subgraph induced by the nodes of ``batch_size`` random walks of ``walk_length`` steps.

    ``data``: ``edge_index`` [2, E], ``num_nodes`` and, optionally, ``edge_attr`` [E] (edge type), ``node_type`` / ``local_node_idx``
    [N], ``y`` [N] or [N, 1] (int64) and ``train_mask`` [N] (bool), on a GPU (or moved to ``device``).  ``save_dir`` / ``log`` and
    further keywords of PyG's loader are accepted and ignored; ``sample_coverage > 0`` (the normalisation statistics) is not offered.
    ``seed``: the sampler's own draws are a counter hash of (seed, batch number, walk, step) -- two samplers with the same seed
    yield the same batches.  ``sample(start, rand)`` forms one batch from injected draws instead (test harnesses).
    ``num_edge_types`` / ``num_node_types``: sizes of ``relations`` (default: largest id + 1).
    ``rank`` / ``world``: iterating yields the batches ``rank, rank + world, ...`` of the SAME stream of ``num_steps`` batches that
    ``world=1`` yields (no walk runs for another rank's batch; ``iter()`` takes the epoch's ``num_steps`` stream positions at once, so
    every rank's next epoch starts at the same position whether or not the iterator was run to its end); ``len()`` is this rank's
    share and ``global_steps`` the length of the whole stream."""

    def __init__(self, data, batch_size, walk_length, num_steps=1, sample_coverage=0, save_dir=None, log=True, seed=0,
                 device=None, num_edge_types=None, num_node_types=None, rank=0, world=1, **kwargs):
        if world < 1 or not 0 <= rank < world:
            raise ValueError("the sampler needs world >= 1 and 0 <= rank < world")
        self.rank, self.world = int(rank), int(world)
        if sample_coverage > 0:
            raise NotImplementedError("sample_coverage > 0 (GraphSAINT normalisation) is not offered; the reference passes 0")
        if walk_length < 1 or batch_size < 1:
            raise ValueError("batch_size and walk_length must be positive")
        ei = data.edge_index
        dev = torch.device(device) if device is not None else ei.device
        ei = ei.to(dev, torch.int64)
        N = int(data.num_nodes) if getattr(data, "num_nodes", None) is not None else (int(ei.max()) + 1 if ei.numel() else 0)
        E = ei.shape[1]
        if not 0 < N < 2 ** 31:
            raise ValueError("the sampler needs 0 < num_nodes < 2^31")
        if E and (int(ei.min()) < 0 or int(ei.max()) >= N):
            raise ValueError("edge_index holds a node id outside [0, num_nodes)")
        self.N, self.E, self.device = N, E, dev
        self.batch_size, self.walk_length, self.num_steps = int(batch_size), int(walk_length), int(num_steps)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._key_dev = torch.zeros(1, dtype=torch.int64, device=dev)    # batch number << 32, kept on the device
        self._key_pos = 0          # the batch number ``_key_dev`` holds (host mirror: no device read)
        self._pos = 0              # stream position of the next batch ``sample()`` draws
        # parent 1: SparseTensor(row, col, value=arange(E)) -- sorted by (row, col), stable, value = original edge id
        row, col = ei[0], ei[1]
        perm = torch.argsort(row * N + col, stable=True)
        self._rowptr = _ind2ptr(row[perm].contiguous(), N)
        self._col = col[perm].contiguous()
        self._val = perm.contiguous()

        def node_attr(name):
            v = getattr(data, name, None)
            return None if v is None else v.to(dev).contiguous()
        self._edge_attr = node_attr("edge_attr")
        self._node_type, self._local_idx = node_attr("node_type"), node_attr("local_node_idx")
        self._y, self._train_mask = node_attr("y"), node_attr("train_mask")
        for name, v, n in (("edge_attr", self._edge_attr, E), ("node_type", self._node_type, N), ("local_node_idx", self._local_idx, N),
                           ("y", self._y, N)):
            if v is not None and (v.dtype != torch.int64 or v.numel() != n):
                raise ValueError(f"data.{name} must be an int64 tensor with {n} entries (one per {'edge' if name == 'edge_attr' else 'node'})")
        if self._train_mask is not None and (self._train_mask.dtype != torch.bool or self._train_mask.numel() != N):
            raise ValueError("data.train_mask must be a bool tensor with one entry per node")
        # parent 2 (relation-major): edges sorted by (edge type, destination, source); row (t, v) = t * N + v, T * N + 1 pointers
        self._rel = None
        if self._edge_attr is not None and self._node_type is not None and E:
            et = self._edge_attr
            if int(et.min()) < 0 or int(self._node_type.min()) < 0:
                raise ValueError("edge / node types must be non-negative")
            T = int(num_edge_types) if num_edge_types is not None else int(et.max()) + 1
            NT = int(num_node_types) if num_node_types is not None else int(self._node_type.max()) + 1
            if int(et.max()) >= T or int(self._node_type.max()) >= NT or T * N >= 2 ** 31:
                raise ValueError("edge / node type ids do not fit num_edge_types / num_node_types (or T * N >= 2^31)")
            rrow = et * N + col                                  # by destination
            rperm = torch.argsort(rrow * N + row)
            rel_rowptr = _ind2ptr(rrow[rperm].contiguous(), T * N)
            nt = self._node_type
            types_sorted = bool((nt[1:] >= nt[:-1]).all()) if N > 1 else True
            # node types laid out one after the other (group_hetero_graph): the batch's per-type row lists are index ranges
            bounds = torch.searchsorted(nt, torch.arange(NT + 1, dtype=torch.int64, device=dev)) if types_sorted else None
            self._rel = (T, NT, rel_rowptr, row[rperm].contiguous(), bounds)
        self._flag = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._ws = {}

    @property
    def global_steps(self) -> int:
        return self.num_steps

    def __len__(self):
        return (self.num_steps - self.rank + self.world - 1) // self.world

    def __iter__(self):
        if self.world == 1:
            return (self.sample() for _ in range(self.num_steps))
        # a rank's slice: the epoch's ``num_steps`` stream positions are taken HERE, when the iterator is made, and every own batch is
        # drawn at its absolute position -- so the next epoch starts at the same position on every rank however far (or with how many
        # ``next()`` calls) this iterator is consumed; another rank's batch costs nothing (the draws are a hash of the batch number)
        base = self._pos
        self._pos = base + self.num_steps
        return (self.sample(_at=base + b) for b in range(self.rank, self.num_steps, self.world))

    def _seek(self, pos: int) -> None:
        if pos != self._key_pos:
            self._key_dev.fill_(pos * _BATCH_KEY_STEP)
            self._key_pos = pos

    def _workspace(self, items):
        ws = self._ws.get(items)
        if ws is None:
            ws = self._ws[items] = torch.empty(_lib.load().egnn_saint_scan_ws_bytes(items), dtype=torch.uint8, device=self.device)
        return ws

    def sample(self, start: Tensor | None = None, rand: Tensor | None = None, _at: int | None = None) -> SaintBatch:
        """One batch.  ``start`` [B] int64 and ``rand`` [B, walk_length] fp32 in [0, 1): the walks' draws (both or neither).  (``_at``:
        the stream position to draw at instead of the next one; the rank-sliced iterator's.)"""
        _lib.require_gpu(self._rowptr)
        if (start is None) != (rand is None):
            raise ValueError("pass both start and rand, or neither")
        lib, st, dev, N, L, p = _lib.load(), _lib.stream(), self.device, self.N, self.walk_length, _lib.ptr
        B = self.batch_size
        if start is not None:
            start, rand = start.to(dev, torch.int64).contiguous(), rand.to(dev, torch.float32).contiguous()
            B = start.numel()
            if B < 1 or tuple(rand.shape) != (B, L) or int(start.min()) < 0 or int(start.max()) >= N:
                raise ValueError("start must hold B >= 1 node ids and rand must be [B, walk_length]")
        if start is None:
            self._seek(self._pos if _at is None else _at)
        cap = min(N, B * (L + 1))                                 # n_sub can never exceed it: sizes everything before the host knows n_sub
        flag = self._flag.zero_()
        walks = torch.empty((B, L + 1), dtype=torch.int64, device=dev)
        _lib.check(lib.egnn_saint_random_walk_i64(p(self._rowptr), p(self._col), N, self.E, B, L, p(start), p(rand), self.seed,
                                                  None if start is not None else p(self._key_dev), p(walks), p(flag), st),
                   "egnn_saint_random_walk_i64")
        if start is None:
            self._key_dev += _BATCH_KEY_STEP
            self._key_pos += 1
            if _at is None:
                self._pos += 1
        relabel = torch.empty(N + 1, dtype=torch.int64, device=dev)
        node_buf = torch.empty(cap, dtype=torch.int64, device=dev)
        ws_n = self._workspace(N)
        _lib.check(lib.egnn_saint_select_i64(p(flag), N, p(relabel), p(node_buf), cap, p(ws_n), ws_n.numel(), st), "egnn_saint_select_i64")
        n_dev = relabel[N:]                                       # [1]: n_sub on the device
        counts = torch.empty(cap, dtype=torch.int64, device=dev)
        eptr = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        ws_c = self._workspace(cap)
        _lib.check(lib.egnn_saint_induced_count_i64(p(self._rowptr), p(self._col), p(node_buf), cap, p(n_dev), 1, 0, N, p(flag), p(counts),
                                                    p(eptr), p(ws_c), ws_c.numel(), st), "egnn_saint_induced_count_i64")
        sizes = [n_dev, eptr[cap:]]
        if self._rel is not None:
            T, NT, rel_rowptr, rel_col, bounds = self._rel
            rcounts = torch.empty(T * cap, dtype=torch.int64, device=dev)
            rptr = torch.empty(T * cap + 1, dtype=torch.int64, device=dev)
            ws_r = self._workspace(T * cap)
            _lib.check(lib.egnn_saint_induced_count_i64(p(rel_rowptr), p(rel_col), p(node_buf), cap, p(n_dev), T, N, N, p(flag), p(rcounts),
                                                        p(rptr), p(ws_r), ws_r.numel(), st), "egnn_saint_induced_count_i64")
            sizes.append(rptr[::cap])                             # T + 1 offsets: where each relation's entries start
            if bounds is not None:
                sizes.append(relabel[bounds])                     # NT + 1: rows of the batch below each node type's first id
        sizes = torch.cat(sizes).tolist()                         # THE device->host read of this batch
        n_sub, e_sub = sizes[0], sizes[1]
        node_idx = node_buf[:n_sub]
        edge_index = torch.empty((2, e_sub), dtype=torch.int64, device=dev)
        edge_idx = torch.empty(e_sub, dtype=torch.int64, device=dev)
        _lib.check(lib.egnn_saint_induced_fill_i64(p(self._rowptr), p(self._col), p(self._val), p(node_buf), cap, p(n_dev), 1, 0, N, p(flag),
                                                   p(relabel), p(eptr), e_sub, p(edge_index[0]), p(edge_index[1]), p(edge_idx), st),
                   "egnn_saint_induced_fill_i64")
        relations = None
        if self._rel is not None:
            offs = sizes[2:2 + T + 1]
            rcol = torch.empty(offs[T], dtype=torch.int64, device=dev)
            _lib.check(lib.egnn_saint_induced_fill_i64(p(rel_rowptr), p(rel_col), None, p(node_buf), cap, p(n_dev), T, N, N, p(flag),
                                                       p(relabel), p(rptr), offs[T], None, p(rcol), None, st), "egnn_saint_induced_fill_i64")
            # row pointers of relation t: entries [t * cap, t * cap + n_sub] of the scan, rebased to the relation's first entry
            rps = rptr.as_strided((T, n_sub + 1), (cap, 1)) - rptr[::cap][:T].view(T, 1)
            adjs = [None if offs[t + 1] == offs[t] else
                    SparseTensor(rowptr=rps[t], col=rcol[offs[t]:offs[t + 1]], sparse_sizes=(n_sub, n_sub)) for t in range(T)]
        batch = SaintBatch(num_nodes=n_sub, node_idx=node_idx, edge_index=edge_index, edge_idx=edge_idx, walks=walks)
        out = {}
        for name, src in (("node_type", self._node_type), ("local_node_idx", self._local_idx), ("y", self._y)):
            out[name] = None if src is None else torch.empty((n_sub,) + tuple(src.shape[1:]), dtype=torch.int64, device=dev)
        mask = self._train_mask
        out["train_mask"] = None if mask is None else torch.empty(n_sub, dtype=torch.bool, device=dev)
        out["edge_attr"] = None if self._edge_attr is None else torch.empty(e_sub, dtype=torch.int64, device=dev)
        _lib.check(lib.egnn_saint_gather_i64(p(node_idx), n_sub, p(self._node_type), p(self._local_idx), p(self._y), p(mask),
                                             p(out["node_type"]), p(out["local_node_idx"]), p(out["y"]), p(out["train_mask"]),
                                             p(edge_idx), e_sub, p(self._edge_attr), p(out["edge_attr"]), st), "egnn_saint_gather_i64")
        for k, v in out.items():
            setattr(batch, k, v)
        if self._rel is not None:
            if bounds is not None:
                b = sizes[2 + T + 1:]
                rows = [torch.arange(b[i], b[i + 1], dtype=torch.int64, device=dev) for i in range(NT)]
            else:   # node types interleaved in the parent: one nonzero (and host read) per node type, as RGCNConv._relations
                rows = [torch.nonzero(batch.node_type == i).view(-1) for i in range(NT)]
            relations = (adjs, rows)
        batch.relations = relations
        return batch
