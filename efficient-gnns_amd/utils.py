"""``torch_geometric.utils.{softmax, subgraph, to_undirected}`` and ``utils.hetero.group_hetero_graph`` stand-ins
(/root/reference/arxiv_pyg/criterion.py:5,103-113; /root/reference/arxiv_pyg/gnn.py:14,249; SURVEY 9.7, 9.8;
/root/reference/mag_pyg/gnn.py:14,16,333,346)."""
from __future__ import annotations

import torch
from torch import Tensor


def subgraph(subset: Tensor, edge_index: Tensor, edge_attr=None, relabel_nodes: bool = False, num_nodes: int | None = None):
    """Edges with both endpoints in ``subset`` (original order); ids relabelled to positions in ``subset``.
    Integer preprocessing (once per process in the reference); runs on the device the indices live on."""
    dev = edge_index.device
    if num_nodes is None:
        num_nodes = int(max(int(edge_index.max()) + 1 if edge_index.numel() else 0,
                            (int(subset.max()) + 1 if subset.dtype != torch.bool else subset.numel()) if subset.numel() else 0))
    if subset.dtype == torch.bool:
        in_set, idx = subset, torch.nonzero(subset).view(-1)
    else:
        in_set = torch.zeros(num_nodes, dtype=torch.bool, device=dev)
        in_set[subset] = True
        idx = subset
    mask = in_set[edge_index[0]] & in_set[edge_index[1]]
    ei = edge_index[:, mask]
    ea = edge_attr[mask] if edge_attr is not None else None
    if relabel_nodes:
        relabel = torch.zeros(num_nodes, dtype=torch.int64, device=dev)
        relabel[idx] = torch.arange(idx.numel(), dtype=torch.int64, device=dev)
        ei = relabel[ei]
    return ei, ea


def softmax(src: Tensor, index: Tensor | None = None, ptr=None, num_nodes: int | None = None, dim: int = 0) -> Tensor:
    """Softmax over entries grouped by ``index`` (any order): exp(src - max) / (sum + 1e-16), per trailing element.

    A 1-D ``src`` with an ``index`` takes the sorted-segment path of the LSP loss (``ops_edge.segment_softmax``).  ``src`` of two or
    more dimensions -- the [E, heads] scores of an attention conv -- goes to ``ops.scatter_softmax`` over the run keys of a
    ``rows_plan``: the running ``propagate`` call's own plan when ``index`` is that call's target-side endpoint tensor (the ``index``
    that ``message`` receives), else a deferred plan over ``num_nodes`` rows (no host read), else ``num_nodes = index.max() + 1`` (one
    host read, as PyG).  ``index=None`` with ``ptr``: the groups are the consecutive ranges ``ptr[i]:ptr[i+1]``.  The node axis is 0."""
    from . import _lib, ops
    src = _lib.real(src)
    if dim not in (0, -src.dim()):
        raise NotImplementedError(f"softmax: `dim` must be 0 (or {-src.dim()}): the entries are grouped along the first axis, got {dim}")
    if index is None:
        if ptr is None:
            raise ValueError("softmax: one of `index` and `ptr` is needed")
        _lib.require_gpu(src, ptr)
        counts = ptr[1:] - ptr[:-1]
        index = torch.repeat_interleave(torch.arange(counts.numel(), dtype=torch.int64, device=ptr.device), counts, output_size=src.shape[0])
        if num_nodes is None:
            num_nodes = counts.numel()
    if src.dim() == 1:
        from .ops_edge import segment_softmax
        return segment_softmax(src, index, num_nodes)
    _lib.require_gpu(src, index)
    from .nn import running_plan
    found = running_plan(index, num_nodes)
    if found is not None:
        plan, num_nodes = found
    else:
        if num_nodes is None:
            num_nodes = int(index.max()) + 1 if index.numel() else 0
        plan = ops.rows_plan(index.contiguous(), num_nodes, check="deferred") if num_nodes > 0 else None
    return ops.scatter_softmax(src, index, num_nodes, plan=plan, eps=1e-16)


def dgl_bidirected_with_self_loops(adj_t):
    """The message graph of the arxiv GAT teacher (/root/reference/arxiv_dgl/gat.py:56-71 ``preprocess``):
    ``dgl.to_bidirected`` (union with the reversed edges, duplicates merged), ``remove_self_loop().add_self_loop()`` (exactly
    one loop per node) -- as a ``SparseTensor`` whose row i lists the sources of the edges into i, columns ascending."""
    import torch
    from .sparse import SparseTensor
    sym = adj_t.to_symmetric()
    rowptr, col, _ = sym.csr()
    n = sym.sparse_size(0)
    row = sym.storage.row()
    keep = row != col
    loops = torch.arange(n, dtype=col.dtype, device=col.device)
    r, c = torch.cat([row[keep], loops]), torch.cat([col[keep], loops])
    return SparseTensor(row=r, col=c, sparse_sizes=(n, n))   # sorted by (row, col) in the constructor


def to_undirected(edge_index: Tensor, num_nodes: int | None = None) -> Tensor:
    """Union of the edges with their reverses, sorted by (row, col), duplicates merged (/root/reference/mag_pyg/gnn.py:333: the
    paper-cites-paper relation).  Integer preprocessing, once per run; runs on the device the indices live on."""
    row, col = edge_index[0], edge_index[1]
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1 if edge_index.numel() else 0
    keys = torch.unique(torch.cat([row * num_nodes + col, col * num_nodes + row]))   # sorted ascending
    if keys.numel() == 0:
        return edge_index.new_zeros((2, 0))
    return torch.stack([torch.div(keys, num_nodes, rounding_mode="floor"), keys % num_nodes])


def group_hetero_graph(edge_index_dict, num_nodes_dict=None):
    """One homogeneous graph out of a heterogeneous one, with PyG's semantics (/root/reference/mag_pyg/gnn.py:346): node types are
    numbered in ``num_nodes_dict`` order and laid out one after the other (cumulative offsets), edge types are numbered in
    ``edge_index_dict`` order; an edge of key ``keys`` has its endpoints shifted by the offsets of ``keys[0]`` and ``keys[-1]``.
    Returns ``(edge_index, edge_type, node_type, local_node_idx, local2global, key2int)``: ``local2global`` is keyed by the node
    type's name and by its integer, ``key2int`` holds the node keys and the edge-key tuples.  ``num_nodes_dict`` = None: every
    node type that appears in an edge key, sized by the largest id seen."""
    as_ei = lambda v: v if isinstance(v, Tensor) else torch.stack(list(v))   # noqa: E731  (a (row, col) pair is accepted too)
    edge_index_dict = {k: as_ei(v) for k, v in edge_index_dict.items()}
    if num_nodes_dict is None:
        num_nodes_dict = {}
        for keys, ei in edge_index_dict.items():
            for key, ids in ((keys[0], ei[0]), (keys[-1], ei[1])):
                num_nodes_dict[key] = max(num_nodes_dict.get(key, 0), int(ids.max()) + 1 if ids.numel() else 0)
    first = next(iter(edge_index_dict.values()))
    dev = first.device
    key2int, offset, local2global = {}, {}, {}
    node_types, local_ids = [], []
    total = 0
    for i, (key, n) in enumerate(num_nodes_dict.items()):
        key2int[key] = i
        node_types.append(torch.full((n,), i, dtype=torch.int64, device=dev))
        local_ids.append(torch.arange(n, dtype=torch.int64, device=dev))
        offset[key] = total
        local2global[key] = local2global[i] = local_ids[-1] + total
        total += n
    edge_indices, edge_types = [], []
    for i, (keys, ei) in enumerate(edge_index_dict.items()):
        key2int[keys] = i
        inc = torch.tensor([[offset[keys[0]]], [offset[keys[-1]]]], dtype=torch.int64, device=dev)
        edge_indices.append(ei.to(torch.int64) + inc)
        edge_types.append(torch.full((ei.shape[1],), i, dtype=torch.int64, device=dev))
    return (torch.cat(edge_indices, dim=1), torch.cat(edge_types), torch.cat(node_types), torch.cat(local_ids), local2global, key2int)
