"""``torch_geometric.nn.{GCNConv, SAGEConv}`` stand-ins on the gfx950 kernels.

Same constructor / forward signatures, parameter names and layouts as PyG <=1.7, which is what the
reference's ``state_dict`` files hold (/root/reference/arxiv_pyg/gnn.py:13,28-35,61-67,92;
/root/reference/ppi_pyg/gnn.py:125-132,158-164).
"""
from __future__ import annotations

import inspect
import math

import torch
from torch import Tensor, nn

from . import ops
import os

from . import _lib, ops_edge
from .sparse import SparseTensor, _ind2ptr, csr_from_coo, gcn_norm, gcn_norm_weighted_csr

# opt-in: the headline bench keeps the reference's per-step work (aggregate every layer every step)
_MEMOISE_AX = os.environ.get("EGNN_GCN_MEMOISE_AX", "0") == "1"
_SAGE_FUSED = True          # SAGEConv as one autograd node with accumulating stores (ops._SageLayer); tests compare with the composed form
_SAGE_NARROW_FIRST = True   # SAGEConv aggregates lin_l(x) when out < in (r03: SAGE + LSP 124.6 -> 136.1 epochs/s)


def _adj_from_edge_index(edge_index: Tensor, n: int, value: Tensor | None = None) -> SparseTensor:
    """edge_index = (source, target) -> CSR with rows = targets, stable in edge order (PPI path)."""
    src, dst = edge_index[0], edge_index[1]
    perm = torch.argsort(dst, stable=True)
    return SparseTensor(rowptr=_ind2ptr(dst[perm].contiguous(), n), col=src[perm],
                        value=None if value is None else value[perm], sparse_sizes=(n, n))


def _gcn_norm_edge_index(edge_index: Tensor, n: int) -> SparseTensor:
    """PyG <=1.7 ``gcn_norm`` on an edge_index (ppi_pyg/gnn.py:125-132): add_remaining_self_loops, then
    D^-1/2 A D^-1/2 with in-degrees by target.  Every loop carries weight 1, so the result equals the
    SparseTensor branch applied to the target-major CSR with duplicates kept (with unit weights only: given an
    ``edge_weight`` an existing loop keeps its own weight here, ``_gcn_norm_edge_index_weighted``, while the SparseTensor
    branch replaces it by 1)."""
    src, dst = edge_index[0], edge_index[1]
    keep = src != dst
    loops = torch.arange(n, dtype=torch.int64, device=edge_index.device)
    src2, dst2 = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
    w = torch.ones(src2.numel(), dtype=torch.float32, device=edge_index.device)
    deg = torch.zeros(n, dtype=torch.float32, device=edge_index.device).index_add_(0, dst2, w)
    dinv = deg.pow(-0.5)
    dinv.masked_fill_(dinv == float("inf"), 0.0)
    val = dinv[src2] * w * dinv[dst2]
    return _adj_from_edge_index(torch.stack([src2, dst2]), n, val)


def _gcn_norm_edge_index_weighted(edge_index: Tensor, edge_weight: Tensor, n: int) -> SparseTensor:
    """PyG <=1.7 ``gcn_norm`` on (edge_index, edge_weight) (edge-index branch): ``add_remaining_self_loops(edge_index, w, 1.0,
    n)`` -- an existing loop KEEPS its weight, a node without one gets 1.0 -- then deg = scatter_add(w, target) and
    norm = dinv[src] * w * dinv[dst], on the target-major CSR.  Differentiable in ``edge_weight`` (the loops' own weights included).
    Several loops on one node are undefined in PyG (the last write wins) and are not checked for here either."""
    if edge_weight.dim() != 1 or edge_weight.numel() != edge_index.shape[1] or edge_weight.dtype != torch.float32:
        raise ValueError("GCNConv: edge_weight is a float32 vector with one weight per edge")
    src, dst = edge_index[0], edge_index[1]
    keep = src != dst
    loops = torch.arange(n, dtype=torch.int64, device=edge_index.device)
    loop_w = torch.ones(n, dtype=torch.float32, device=edge_index.device).index_put((src[~keep],), edge_weight[~keep])
    src2, dst2 = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
    w2 = torch.cat([edge_weight[keep], loop_w])
    return gcn_norm_weighted_csr(_adj_from_edge_index(torch.stack([src2, dst2]), n, w2))


from ._cache import TensorKeyedCache as _TensorKeyedCache  # noqa: E402  (LRU, pins entries a captured graph reads: _cache.py)


_GCN_NORM_CACHE = _TensorKeyedCache(capacity=64)


class GCNConv(nn.Module):
    """out = A^ (x W) + b;  W [in,out] glorot, b zeros;  ``cached=True`` keeps A^ until reset_parameters().

    The aggregation runs on the narrower side of W: A^ (x W) when in >= out (the reference's order, gnn.py:47) and
    (A^ x) W when in < out -- the same product, re-associated so that the HBM-bound gather moves `in` instead of `out`
    floats per neighbour (ogbn-arxiv layer 1: 128 instead of 256), and a constant input needs no aggregation at all in
    the backward (dW = (A^ x)^T dOut)."""

    def __init__(self, in_channels: int, out_channels: int, cached: bool = False, bias: bool = True, **_):
        super().__init__()
        self.in_channels, self.out_channels, self.cached = in_channels, out_channels, cached
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self._cached_adj_t = None
        self._cached_ax = None  # (key, A^ x) for a constant input tensor, see forward()
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))
        with torch.no_grad():
            self.weight.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()
        self._cached_adj_t = None
        self._cached_ax = None

    def forward(self, x: Tensor, edge_index, edge_weight=None, bn_stats_shift: Tensor | None = None, want_bn_stats: bool = False,
                eval_bn=None, xw: Tensor | None = None) -> Tensor:
        """``bn_stats_shift`` / ``want_bn_stats`` (extension, off by default): the caller applies a BatchNorm to the result next
        and wants its column statistics formed in the aggregation's epilogue (``ops.spmm``).
        ``eval_bn`` (extension, no autograd): an eval-mode ``BatchNorm1d`` that follows, with a ReLU behind it (gnn.py:47-49 under
        ``model.eval()``): returns ``relu(eval_bn(conv(x)))`` with the BatchNorm folded into W / b (``ops.bn_fold``) and the ReLU
        in the last kernel's store -- the separate normalisation pass disappears from ``test()``.
        ``xw`` (extension): ``x @ self.weight`` when the caller has it already (``ops.bn_act_linear`` forms it together with x); only
        taken on the transform-first order of a plain SparseTensor adjacency."""
        sharded = hasattr(edge_index, "gcn_normalized")
        if edge_weight is not None:
            if sharded:
                raise NotImplementedError("GCNConv: edge_weight on a node-range shard (dist.ShardedAdj) is not offered")
            if isinstance(edge_index, SparseTensor):
                raise ValueError("GCNConv: a SparseTensor carries its weights as values (adj_t.set_value(w)); edge_weight goes with an edge_index")
            edge_weight = _lib.real(edge_weight)
            _lib.require_gpu(x, edge_index, edge_weight)
        # learnable weights (edge_weight, or the values of a SparseTensor): A^ changes with every step and carries a graph, so nothing
        # derived from it is kept -- neither by cached=True nor by the edge-index memo nor by the memoised A^ x
        weights = edge_weight if edge_weight is not None else (edge_index._value if isinstance(edge_index, SparseTensor) else None)
        learnable = weights is not None and weights.requires_grad
        agg_first = self.in_channels < self.out_channels
        if eval_bn is not None:
            if torch.is_grad_enabled() or eval_bn.training or not (isinstance(edge_index, SparseTensor) or sharded) or not x.is_cuda:
                raise ValueError("eval_bn: inference only (no_grad, BatchNorm in eval mode, SparseTensor / sharded adjacency on the GPU)")
            if sharded:   # node-range shard: the same fold, bias + ReLU in the store of the aggregation's last piece
                w, b = ops.bn_fold(self.weight, self.bias, eval_bn)
                if agg_first:
                    return ops.gemm_raw(edge_index.gcn_normalized().aggregate(x, "sum"), w, False, False, b, relu=True)
                return edge_index.gcn_normalized().aggregate(ops.gemm_raw(x, w), "sum", bias=b, relu=True)
            norm = None if learnable else self._cached_adj_t
            if norm is None:
                norm = gcn_norm(edge_index)
                if self.cached and not learnable:
                    self._cached_adj_t = norm
            w, b = ops.bn_fold(self.weight, self.bias, eval_bn)
            if agg_first:
                return ops.gemm_raw(ops.spmm_raw(norm, x, "sum")[0], w, False, False, b, relu=True)
            return ops.spmm_raw(norm, ops.gemm_raw(x, w), "sum", bias=b, relu=True)[0]
        if hasattr(edge_index, "gcn_normalized"):  # node-range shard (dist.ShardedAdj): halo exchange + local rows of A^
            if agg_first:
                return ops.matmul(edge_index.gcn_normalized().aggregate(x, "sum"), self.weight, self.bias)
            return edge_index.gcn_normalized().aggregate(ops.matmul(x, self.weight) if xw is None else xw, "sum", bias=self.bias)
        norm = None if learnable else self._cached_adj_t
        if norm is None:
            if isinstance(edge_index, SparseTensor):
                norm = gcn_norm(edge_index)
            elif edge_weight is not None:
                n_nodes = x.shape[0]
                if learnable:
                    norm = _gcn_norm_edge_index_weighted(edge_index, edge_weight, n_nodes)
                else:   # constant weights: memoised like the value-less edge list, keyed on the weight tensor too (identity + version)
                    norm = _GCN_NORM_CACHE.get((edge_index, edge_weight), (n_nodes,),
                                               lambda: _gcn_norm_edge_index_weighted(edge_index, edge_weight, n_nodes))
            else:
                # ``cached=False`` (PPI: one batch graph per step, ppi_pyg/gnn.py:125) re-normalises on every call in PyG.
                # The result only depends on the integer edge list, so it is memoised on that tensor's identity: the 20
                # training graphs come back every epoch, in every layer, and building A^ costs a device->host read.
                n_nodes = x.shape[0]
                norm = _GCN_NORM_CACHE.get((edge_index,), (n_nodes,), lambda: _gcn_norm_edge_index(edge_index, n_nodes))
            if self.cached and not learnable:
                self._cached_adj_t = norm
        if (self.cached and _MEMOISE_AX and not learnable and not x.requires_grad and self.in_channels <= self.out_channels
                and isinstance(edge_index, SparseTensor)):
            # constant input (the first layer's node features): A^ (x W) == (A^ x) W, and A^ x does not change between
            # steps, so it is kept next to the cached A^ (same lifetime) and the per-step aggregation disappears from
            # forward, backward (dW = (A^ x)^T dOut, no dX needed) and eval.  Keyed on the tensor's identity + version.
            key = (x.data_ptr(), x._version, tuple(x.shape), id(norm))
            if self._cached_ax is None or self._cached_ax[0] != key:
                with torch.no_grad():
                    self._cached_ax = (key, ops.spmm_raw(norm, x, "sum")[0], x)   # holds x: its address cannot be reused meanwhile
            out = ops.matmul(self._cached_ax[1], self.weight)
            return ops.add_bias(out, self.bias)
        if agg_first:
            return ops.matmul(ops.spmm(norm, x, "sum"), self.weight, self.bias)
        return ops.spmm(norm, ops.matmul(x, self.weight) if xw is None else xw, "sum", bias=self.bias,  # bias added in the kernel's store
                        bn_stats_shift=bn_stats_shift, want_bn_stats=want_bn_stats)

    def _uses_memoised_input(self, x: Tensor) -> bool:
        """True when forward() would take the opt-in memoised ``A^ x`` route for this input (EGNN_GCN_MEMOISE_AX)."""
        return bool(self.cached and _MEMOISE_AX and not x.requires_grad and self.in_channels <= self.out_channels)

    def __repr__(self):
        return f"GCNConv({self.in_channels}, {self.out_channels})"


class SAGEConv(nn.Module):
    """out = lin_l(aggr_{j in N(i)} x_j) + lin_r(x_i); ``aggr`` in {mean (reference), sum, max}."""

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean", **_):
        super().__init__()
        if aggr == "add":
            aggr = "sum"
        if aggr not in ("mean", "sum", "max"):
            raise ValueError(f"unsupported aggregation '{aggr}'")
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.lin_l = nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x: Tensor, edge_index) -> Tensor:
        if hasattr(edge_index, "aggregate"):  # node-range shard (dist.ShardedAdj)
            if _SAGE_FUSED and hasattr(edge_index, "sage_layer"):
                # one autograd node with accumulating stores and (out < in) the narrow-first order, as on one GPU (ops._SageLayer)
                out = edge_index.sage_layer(x, self.lin_l, self.lin_r, self.aggr, _SAGE_NARROW_FIRST and self.out_channels < self.in_channels)
                if out is not None:
                    return out
            agg = edge_index.aggregate(x, self.aggr, valueless=True)
            # lin_l(agg) + lin_r(x): the second product is added in the first GEMM's store (ops.linear_add)
            return ops.linear_add(agg, self.lin_l.weight, self.lin_l.bias, ops.linear(x, self.lin_r.weight, None))
        adj = edge_index if isinstance(edge_index, SparseTensor) else _adj_from_edge_index(edge_index, x.shape[0])
        if (_SAGE_FUSED and self.aggr in ("mean", "sum") and x.is_cuda and x.dim() == 2 and self.lin_r.bias is None
                and adj.nnz() > 0 and adj.sparse_size(0) == adj.sparse_size(1)):
            # lin_l(aggr(x)) + lin_r(x) with both sums formed in kernel stores (ops._SageLayer): no element-wise pass forward or backward
            narrow = _SAGE_NARROW_FIRST and self.out_channels < self.in_channels
            return ops.sage_layer(x, adj.set_value(None), self.lin_l, self.lin_r, self.aggr, narrow)
        if _SAGE_NARROW_FIRST and self.out_channels < self.in_channels and self.aggr in ("mean", "sum") and x.is_cuda:
            # mean / sum are linear: aggr_j(x_j) W^T == aggr_j(x_j W^T).  On the output layer (256 -> 40 classes, gnn.py:84) the HBM-bound
            # gather then moves `out` instead of `in` floats per neighbour, forward and backward -- the re-association GCNConv makes.
            # The bias goes in after the aggregation (a row without neighbours gets lin_l(0) = bias either way).
            return ops.spmm(adj.set_value(None), ops.linear(x, self.lin_l.weight, None), self.aggr, bias=self.lin_l.bias) \
                + ops.linear(x, self.lin_r.weight, None)
        agg = ops.spmm(adj.set_value(None), x, self.aggr)
        return ops.linear(agg, self.lin_l.weight, self.lin_l.bias) + ops.linear(x, self.lin_r.weight, None)

    def __repr__(self):
        return f"SAGEConv({self.in_channels}, {self.out_channels}, aggr={self.aggr})"


_GAT_STRUCT_CACHE = _TensorKeyedCache(capacity=64)


class GATConv(nn.Module):
    """PyG <=1.7 ``GATConv``: the frozen GAT teacher that the PPI / MAG train loops run inside every student step
    (/root/reference/ppi_pyg/gnn.py:86-117,208-209), and the layer of the PPI GAT student and teacher in training
    (gnn.py:50-83 ``StudentNet``, :23-47 ``TeacherNet``, ppi_pyg/train_teacher.py).  Same parameters and ``state_dict`` keys as
    PyG 1.6/1.7 (``lin_l.weight`` shared with ``lin_r``, ``att_l`` / ``att_r`` [1,H,C], ``bias``).

    Forward on the gfx950 kernels: x W on the fp32 MFMA, the 2H attention logits per node as one more small GEMM
    (``ops_edge.gat_logits``), scores + LeakyReLU + per-target softmax fused in one launch (``ops_edge.gat_coefficients``: no [E,H]
    gathers or scatter-softmax temporaries), one valued SpMM per head written straight into its column block
    (``ops_edge.gat_aggregate``).  In training mode with autograd on, the same three steps are one autograd node
    (``ops_edge.gat_attention``) whose backward -- the one ``DGLGATConv`` runs too -- takes three HIP launches for all heads
    (``egnn_gat_layer_bwd_f32``, csrc/gat.hip).  In eval mode a call that would need gradients raises: the eval forward is the
    frozen teacher's."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, bias: bool = True, **_):
        super().__init__()
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops = negative_slope, dropout, add_self_loops
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_r = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for t in (self.lin_l.weight, self.att_l, self.att_r):
                a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))  # glorot
                t.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()

    def _structure(self, adj, n: int) -> SparseTensor:
        """CSR by target with the self loops replaced (remove_self_loops + add_self_loops), built on the device.
        Integer preprocessing, memoised on the identity of the index tensor (the PPI teacher meets the same 20 batch
        graphs every epoch, in each of its three layers; PyG rebuilds the loops per call)."""
        keys = (adj._col, adj._rowptr) if isinstance(adj, SparseTensor) else (adj,)
        return _GAT_STRUCT_CACHE.get(keys, (n, self.add_self_loops), lambda: self._build_structure(adj, n))

    def _build_structure(self, adj, n: int) -> SparseTensor:
        if isinstance(adj, SparseTensor):
            src, dst = adj._col, adj._row()
        else:
            src, dst = adj[0], adj[1]
        if self.add_self_loops:
            keep = src != dst
            loops = torch.arange(n, dtype=src.dtype, device=src.device)
            src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
        rowptr, col = csr_from_coo(dst.contiguous(), src.contiguous(), n, symmetric=False)
        return SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n))

    def forward(self, x: Tensor, edge_index) -> Tensor:
        x = _lib.real(x)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if not self.training:
                raise NotImplementedError("GATConv in eval mode runs the frozen teacher (torch.no_grad() / requires_grad_(False)); "
                                          "train it in training mode (.train())")
            return self._forward_train(x, edge_index)
        _lib.require_gpu(x)
        n, H, C = x.shape[0], self.heads, self.out_channels
        xl = ops.linear(x, self.lin_l.weight)                                   # [n, H*C]
        alpha = ops_edge.gat_logits(xl, self.att_l.detach(), self.att_r.detach(), H, C)   # [n, 2H]
        a_src, a_dst = alpha[:, :H].contiguous(), alpha[:, H:].contiguous()
        adj = self._structure(edge_index, n)
        att = ops_edge.gat_coefficients(adj, a_src, a_dst, self.negative_slope)
        if self.training and self.dropout > 0:
            att = torch.nn.functional.dropout(att, p=self.dropout, training=True)
        out = ops_edge.gat_aggregate(adj, att, xl, C)
        if not self.concat:
            out = out.view(n, H, C).mean(dim=1)
        return ops.add_bias(out, self.bias)

    def _forward_train(self, x: Tensor, edge_index) -> Tensor:
        """The differentiable forward (training mode, autograd on): x W^T through ``ops.linear``, attention + aggregation through
        ``ops_edge.gat_attention`` (HIP backward, csrc/gat.hip), the bias through ``ops.add_bias``.  Attention dropout draws its
        mask with torch's RNG as one ``torch.rand(heads, nnz)`` per call (kept where >= p, scaled by 1 / (1 - p)), on the
        entries of the cached structure."""
        _lib.require_gpu(x)
        n = x.shape[0]
        xl = ops.linear(x, self.lin_l.weight)                                   # [n, H*C]
        adj = self._structure(edge_index, n)
        mult = None
        if self.dropout > 0:
            keep = torch.rand(self.heads, adj.nnz(), dtype=torch.float32, device=x.device) >= self.dropout
            mult = keep.to(torch.float32).mul_(1.0 / (1.0 - self.dropout) if self.dropout < 1 else 0.0)
        out = ops_edge.gat_attention(xl, self.att_l, self.att_r, adj, self.heads, self.concat, self.negative_slope, mult)
        return ops.add_bias(out, self.bias)

    def __repr__(self):
        return f"GATConv({self.in_channels}, {self.out_channels}, heads={self.heads})"


class DGLGATConv(nn.Module):
    """The arxiv GAT teacher's layer (/root/reference/arxiv_dgl/models.py:95-236 -- the reference's own module over DGL
    message passing) for INFERENCE on the gfx950 kernels: the producer of the ``features/`` / ``logits/`` artefacts the
    student path reads (gat.py:243-258).  Same parameter names and initialisation as the reference
    (``fc``, ``attn_l``, ``attn_r`` (absent with ``use_attn_dst=False``), ``res_fc``), so its checkpoints load.

    ``forward(adj, feat)``: ``adj`` = ``SparseTensor`` whose row i lists the sources of the edges j -> i (the DGL graph after
    gat.py:56-71 ``preprocess``: ``utils.dgl_bidirected_with_self_loops``).  The steps of ``GATConv``'s forward through the same
    helpers of ``ops_edge`` (``el`` / ``er`` = the logits GEMM, ``u_add_v`` + LeakyReLU + ``edge_softmax`` = the coefficients,
    ``u_mul_e`` + ``sum`` = one valued SpMM per head over head blocks padded to 16 bytes); symmetric normalisation (out-degree^-1/2 on the sources, in-degree^1/2 on the result) and the
    residual projection as in the reference.  Returns [N, H, F].  In training mode with autograd on the layer is differentiable
    (``_forward_train``: one fused launch for all heads forward, ``GATConv``'s three backward; ``edge_drop`` / ``attn_drop`` /
    ``feat_drop`` act there).  In eval mode a call that would need gradients raises: the eval forward is the frozen teacher's."""

    def __init__(self, in_feats, out_feats, num_heads=1, feat_drop=0.0, attn_drop=0.0, edge_drop=0.0, negative_slope=0.2,
                 use_attn_dst=True, residual=False, activation=None, allow_zero_in_degree=False, use_symmetric_norm=False):
        super().__init__()
        self._num_heads, self._in_feats, self._out_feats = num_heads, in_feats, out_feats
        self._allow_zero_in_degree, self._use_symmetric_norm = allow_zero_in_degree, use_symmetric_norm
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        if use_attn_dst:
            self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        else:
            self.register_buffer("attn_r", None)
        self.feat_drop_p, self.attn_drop_p, self.edge_drop = feat_drop, attn_drop, edge_drop
        self.negative_slope = negative_slope
        if residual:
            self.res_fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
        else:
            self.register_buffer("res_fc", None)
        self._activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        if isinstance(self.attn_r, nn.Parameter):
            nn.init.xavier_normal_(self.attn_r, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    @staticmethod
    def _degrees(adj: SparseTensor):
        """(in-degree^1/2, out-degree^-1/2) of the message graph, both clamped at 1 (models.py:183-186,219-223); cached."""
        st = adj._struct
        if "dgl_norm" not in st:
            rowptr, col, _ = adj.csr()
            n = adj.sparse_size(0)
            in_deg = (rowptr[1:] - rowptr[:-1]).to(torch.float32).clamp(min=1)
            out_deg = torch.bincount(col, minlength=adj.sparse_size(1)).to(torch.float32).clamp(min=1)
            st["dgl_norm"] = (in_deg.pow(0.5).view(n, 1), out_deg.pow(-0.5).view(-1, 1), bool((rowptr[1:] == rowptr[:-1]).any()))
        return st["dgl_norm"]

    def forward(self, adj: SparseTensor, feat: Tensor) -> Tensor:
        feat = _lib.real(feat)
        if torch.is_grad_enabled() and (feat.requires_grad or any(p.requires_grad for p in self.parameters())):
            if not self.training:
                raise NotImplementedError("DGLGATConv in eval mode runs the frozen teacher (torch.no_grad() / requires_grad_(False)); "
                                          "train it in training mode (.train())")
            return self._forward_train(adj, feat)
        if self.training and (self.edge_drop > 0 or self.attn_drop_p > 0 or self.feat_drop_p > 0):
            raise NotImplementedError("training-mode edge / attention / feature drop act in the differentiable forward only "
                                      "(autograd on); use .eval() for inference")
        _lib.require_gpu(feat)
        n, H, F_ = feat.shape[0], self._num_heads, self._out_feats
        in_sqrt, out_rsqrt, has_isolated = self._degrees(adj)
        if has_isolated and not self._allow_zero_in_degree:
            raise AssertionError("zero in-degree node (arxiv_dgl/models.py:167-169)")
        feat_src = ops.linear(feat, self.fc.weight)                               # [n, H*F]
        alpha = ops_edge.gat_logits(feat_src, self.attn_l.detach(), None if self.attn_r is None else self.attn_r.detach(), H, F_)
        el, er = alpha[:, :H].contiguous(), alpha[:, H:].contiguous()             # er = 0 without attn_r (copy_u)
        if self._use_symmetric_norm:
            # the reference scales the SOURCE features (and with them el) by out-degree^-1/2 but forms er from the unscaled
            # destination features (models.py:178-200: feat_dst is bound before the scaling)
            feat_src = feat_src * out_rsqrt
            el = el * out_rsqrt
        att = ops_edge.gat_coefficients(adj, el, er, self.negative_slope)
        Fp = (F_ + 3) // 4 * 4                                                      # head blocks on 16-byte boundaries (F = 250 -> 252)
        src_heads = feat_src if Fp == F_ else torch.nn.functional.pad(feat_src.view(n, H, F_), (0, Fp - F_)).reshape(n, H * Fp)
        plain = adj.set_value(None) if adj.has_value() else adj
        out = ops_edge.gat_aggregate(plain, att, src_heads, Fp)
        rst = out.view(n, H, Fp)[:, :, :F_]
        if self._use_symmetric_norm:
            rst = rst * in_sqrt.view(n, 1, 1)
        if self.res_fc is not None:
            rst = rst + ops.linear(feat, self.res_fc.weight).view(n, -1, F_)
        if self._activation is not None:
            rst = self._activation(rst)
        return rst

    def _draw_edge_keep(self, nnz: int, device) -> Tensor:
        """The entries edge_drop keeps in this call, as a bool [nnz] mask over the CSR entries: ``nnz - int(nnz * edge_drop)`` of
        them chosen uniformly (models.py:207-212: ``randperm(E)[int(E * edge_drop):]``).  Overridable: a test injects a recorded set."""
        keep = torch.zeros(nnz, dtype=torch.bool, device=device)
        keep[torch.randperm(nnz, device=device)[int(nnz * self.edge_drop):]] = True
        return keep

    def _forward_train(self, adj: SparseTensor, feat: Tensor) -> Tensor:
        """The differentiable forward (training mode, autograd on; models.py:154-236): ``feat_drop`` through ``F.dropout``, ``fc`` /
        ``res_fc`` through ``ops.linear``, scores + edge softmax over the kept edges + aggregation + both symmetric-norm scales as one
        autograd node (``ops_edge.dgl_gat_attention``: one HIP launch forward, three backward, csrc/gat.hip).  ``attn_drop`` draws one
        [heads, nnz] multiplier per call (kept where >= p, scaled by 1 / (1 - p)), ``edge_drop`` one kept-entry set (``_draw_edge_keep``)."""
        _lib.require_gpu(feat)
        n, H, F_ = feat.shape[0], self._num_heads, self._out_feats
        in_sqrt, out_rsqrt, has_isolated = self._degrees(adj)
        if has_isolated and not self._allow_zero_in_degree:
            raise AssertionError("zero in-degree node (arxiv_dgl/models.py:167-169)")
        h = torch.nn.functional.dropout(feat, self.feat_drop_p, True) if self.feat_drop_p > 0 else feat
        feat_src = ops.linear(h, self.fc.weight)                                  # [n, H*F], unscaled
        nnz = adj.nnz()
        keep = self._draw_edge_keep(nnz, feat.device) if self.edge_drop > 0 else None
        mult = None
        if self.attn_drop_p > 0:
            kept = torch.rand(H, nnz, dtype=torch.float32, device=feat.device) >= self.attn_drop_p
            mult = kept.to(torch.float32).mul_(1.0 / (1.0 - self.attn_drop_p) if self.attn_drop_p < 1 else 0.0)
        r, q = (out_rsqrt, in_sqrt) if self._use_symmetric_norm else (None, None)
        rst = ops_edge.dgl_gat_attention(feat_src, self.attn_l, self.attn_r, adj, H, self.negative_slope, keep=keep, mult=mult,
                                         src_scale=r, dst_scale=q)                # [n, H, F]
        if self.res_fc is not None:
            rst = rst + ops.linear(h, self.res_fc.weight).view(n, -1, F_)
        if self._activation is not None:
            rst = self._activation(rst)
        return rst

    def __repr__(self):
        return f"DGLGATConv({self._in_feats}, {self._out_feats}, heads={self._num_heads})"


_RGCN_REL_CACHE = _TensorKeyedCache(capacity=8)


class RGCNConv(nn.Module):
    """The reference's own R-GCN layer (/root/reference/mag_pyg/gnn.py:25-68, a ``MessagePassing(aggr='mean')`` subclass) on
    the kernels: per edge type i, ``mean_{j -> t, type i} rel_lins[i](x_j)`` is computed as ``rel_lins[i](mean x_j)`` (the
    linear map has no bias, so it commutes with the mean) -- one mean-SpMM over the type's edges and one MFMA GEMM
    instead of a GEMM over every message; ``root_lins[node type]`` through the fused row-gather GEMM.  Same parameter
    names as the reference (``rel_lins.*``, ``root_lins.*``); differentiable (SpMM / GEMM autograd)."""

    def __init__(self, in_channels, out_channels, num_node_types, num_edge_types):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_node_types, self.num_edge_types = num_node_types, num_edge_types
        self.rel_lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(num_edge_types)])
        self.root_lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=True) for _ in range(num_node_types)])

    def reset_parameters(self):
        for lin in list(self.rel_lins) + list(self.root_lins):
            lin.reset_parameters()

    def _relations(self, edge_index: Tensor, edge_type: Tensor, node_type: Tensor, n: int):
        """Per-type CSR (by target) and per-node-type row lists; integer preprocessing, cached on the tensors' identity."""
        def build():
            adjs = []
            for i in range(self.num_edge_types):
                sel = torch.nonzero(edge_type == i).view(-1)
                if sel.numel() == 0:
                    adjs.append(None)
                    continue
                src, dst = edge_index[0, sel].contiguous(), edge_index[1, sel].contiguous()
                rowptr, col = csr_from_coo(dst, src, n, symmetric=False)
                adjs.append(SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n)))
            rows = [torch.nonzero(node_type == i).view(-1) for i in range(self.num_node_types)]
            return adjs, rows
        return _RGCN_REL_CACHE.get((edge_index, edge_type, node_type), (n, self.num_edge_types, self.num_node_types), build)

    def forward(self, x: Tensor, edge_index: Tensor, edge_type: Tensor, node_type: Tensor, relations=None) -> Tensor:
        """``relations``: what ``_relations`` would return for these arguments, built elsewhere (``saint.SaintBatch.relations``: the
        sampler forms it with the batch); None = build (and memoise) it here."""
        x = _lib.real(x)
        _lib.require_gpu(x, edge_index)
        n = x.shape[0]
        adjs, rows = relations if relations is not None else self._relations(edge_index, edge_type, node_type, n)
        out = torch.zeros(n, self.out_channels, dtype=torch.float32, device=x.device)
        for i, adj in enumerate(adjs):
            if adj is not None:
                out = out + ops.linear(ops.spmm(adj, x, "mean"), self.rel_lins[i].weight)
        for i, idx in enumerate(rows):
            if idx.numel():
                lin = self.root_lins[i]
                out = out.index_add(0, idx, ops.linear_rows(x, idx, lin.weight, lin.bias))
        return out

    def __repr__(self):
        return f"RGCNConv({self.in_channels}, {self.out_channels}, node_types={self.num_node_types}, edge_types={self.num_edge_types})"


# ------------------------------------------------------------------------------------------------
# user-defined convs in PyG's own idiom: gather x_j / x_i, message, aggregate by target, update
# ------------------------------------------------------------------------------------------------
_MP_AGGRS = ("add", "sum", "mean", "max", "min")
_MP_FLOWS = ("source_to_target", "target_to_source")
_MP_SPECIAL = ("edge_index", "edge_index_i", "edge_index_j", "index", "size", "size_i", "size_j", "dim_size", "ptr", "adj_t")
_MP_EMPTY = inspect.Parameter.empty
_MP_RUNNING: list = []     # (the _Propagation, its target side) of every propagate call in progress, innermost last


def running_plan(index, n=None, what: str = "num_nodes"):
    """``(plan, node count)`` of the running ``propagate`` call whose TARGET-side endpoint tensor ``index`` is (identity, innermost call
    first), None when there is none: how ``utils.softmax`` and the ``torch_scatter`` shim share the plan of the lift and the
    aggregation.  A node count the call has not settled yet is taken from ``n`` (``num_nodes`` / ``dim_size``), else read off
    ``index`` (one host read, as PyG)."""
    for call, i in reversed(_MP_RUNNING):
        if call.ends[i] is not None and index is call.ends[i]:
            if n is not None:
                call.see(i, n, what)
            elif call.size[i] is None:
                call.size[i] = int(index.max()) + 1 if index.numel() else 0
            return call.plan(i), call.size[i]
    return None


def running_end_plan(index, n, what: str = "num_nodes"):
    """The plan of the running ``propagate`` call that has the tensor ``index`` as EITHER endpoint (identity, innermost call first) over
    ``n`` nodes, None when there is none: how ``ops.gather_scatter`` on a call's own ``edge_index[0]`` / ``edge_index[1]`` walks the
    keys the lift, the softmax and the aggregation share."""
    for call, _ in reversed(_MP_RUNNING):
        for end in (0, 1):
            if call.ends[end] is not None and index is call.ends[end]:
                call.see(end, n, what)
                return call.plan(end)
    return None


class _Propagation:
    """One ``propagate`` call: the two endpoint id vectors (0: source side, 1: target side of ``edge_index``), the node counts seen so
    far, and AT MOST ONE deferred ``ops.rows_plan`` per endpoint, built when first asked for and shared by the lift (``x_j`` / ``x_i``),
    the lift's backward, a softmax over ``index`` inside ``message`` (``running_plan``) and the aggregation."""

    def __init__(self, ends, size, ptr=None, edge_index=None, adj_t=None):
        self.ends, self.size, self.ptr, self.edge_index, self.adj_t = ends, size, ptr, edge_index, adj_t
        self.plans = [None, None]

    def see(self, end: int, n: int, what: str) -> None:
        if self.size[end] is None:
            self.size[end] = int(n)
        elif self.size[end] != int(n):
            raise ValueError(f"MessagePassing.propagate: `{what}` has {int(n)} rows, but side {end} of the graph has {self.size[end]} nodes")

    def plan(self, end: int):
        if self.plans[end] is None:
            self.plans[end] = ops.rows_plan(self.ends[end].contiguous(), self.size[end], check="deferred")
        return self.plans[end]

    def lift(self, t, end: int, node_dim: int, what: str):
        from . import lazy
        t = _lib.real(t)
        if not isinstance(t, Tensor):
            raise TypeError(f"MessagePassing.propagate: `{what}` must be a tensor, a (source, target) pair of tensors or None")
        if node_dim == -2 and t.dim() > 2:
            raise NotImplementedError("MessagePassing: node_dim=-2 is supported for node tensors of at most 2 dimensions (the node axis is 0)")
        self.see(end, t.shape[0], what)
        _lib.require_gpu(t)
        idx = self.ends[end]
        if lazy.ACCEL_ACTIVE and t.dtype == torch.float32 and idx.numel() > 0 and (
                t.dim() == 2 or (ops.FUSE_LAZY_ROWS and t.dim() == 3 and node_dim == 0 and t.is_contiguous())):
            # under accel: not gathered yet -- a Linear in `message` runs the gather-fused GEMM (ops.linear_rows), a per-edge weight and
            # the aggregation run as one walk (ops.gather_scatter; [N, H, D] too: the heads of an attention conv), anything else forms the rows
            return lazy.LazyRows(t, idx, plan=lambda: self.plan(end))
        return ops.take_rows(t, self.plan(end))


class MessagePassing(nn.Module):
    """``torch_geometric.nn.MessagePassing`` (PyG <= 1.7) on the package's kernels, for convs written in PyG's own idiom::

        class MyConv(MessagePassing):
            def __init__(self): super().__init__(aggr="mean")
            def forward(self, x, edge_index, w): return self.propagate(edge_index, x=x, w=w)
            def message(self, x_i, x_j, w): return w.view(-1, 1) * (x_j - x_i)
            def update(self, aggr_out, x): return aggr_out + x

    ``propagate(edge_index, size=None, **kwargs)`` reads the parameter names of ``message`` / ``aggregate`` / ``update`` /
    ``message_and_aggregate`` (``inspect``, once per class).  With ``(j, i) = (0, 1)`` for ``flow="source_to_target"`` and ``(1, 0)``
    otherwise, a message parameter ``name_j`` / ``name_i`` receives ``kwargs[name]`` lifted to the edges by ``edge_index[j]`` /
    ``edge_index[i]`` (None stays None; of a ``(source, target)`` pair -- source_to_target only -- element 0 / 1); every other
    parameter receives ``kwargs[name]`` as it is (an int such as ``edge_type``, a per-edge tensor such as ``edge_weight``).  Special
    names: ``edge_index``, ``edge_index_i``, ``edge_index_j``, ``index`` (= ``edge_index[i]``), ``size``, ``size_i``, ``size_j``,
    ``dim_size`` (the target side), ``ptr`` (None for an edge list) and ``adj_t``.  Node counts come from ``size`` or from the node
    tensors.  Defaults: ``message(x_j) -> x_j``, ``aggregate`` = ``ops.scatter`` by ``index`` with the class's ``aggr``, ``update`` =
    identity.  A ``SparseTensor`` (the transposed adjacency, source_to_target only) goes to ``message_and_aggregate`` when the subclass
    defines it, and is otherwise taken apart (row -> i, col -> j, ``ptr`` = rowptr).

    The lift is ``ops.take_rows`` and the aggregation ``ops.scatter``, both over ONE ``ops.rows_plan(check="deferred")`` per endpoint
    and call: no host read per fresh ``edge_index[:, mask]``; an id out of range is dropped and counted (``ops.rows_oob``), not
    raised.  ``utils.softmax(alpha, index, ptr, size_i)`` on [E, heads] scores inside ``message`` (and the ``torch_scatter`` softmax
    functions) finds the running call through ``running_plan`` and walks the target side's plan: no plan of its own, no host read.
    Under ``accel`` a lifted 2-D fp32 tensor is handed out as ``lazy.LazyRows``: ``self.lin(x_j)`` runs as the gather-fused
    ``ops.linear_rows``.  With the default ``message`` and ``aggregate`` and ``aggr`` add / sum / mean, lift and aggregation are ONE walk
    (``ops.gather_scatter``, bit-equal to the two steps); under ``accel`` so are ``edge_weight.view(-1, 1) * x_j`` and, on [N, H, D] node
    tensors (``node_dim=0``), ``x_j * alpha.unsqueeze(-1)`` (``lazy.LazyWeightedRows``): no [E, C] tensor forward or backward.  GPU only,
    like every operator of the package."""

    def __init__(self, aggr: str = "add", flow: str = "source_to_target", node_dim: int = -2):
        super().__init__()
        if aggr not in _MP_AGGRS:
            raise ValueError(f"MessagePassing: aggr must be one of {_MP_AGGRS}, got {aggr!r}")
        if flow not in _MP_FLOWS:
            raise ValueError(f"MessagePassing: flow must be one of {_MP_FLOWS}, got {flow!r}")
        if node_dim not in (0, -2):
            raise NotImplementedError(f"MessagePassing: node_dim must be 0 or -2 (the node axis is the first one), got {node_dim!r}")
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim
        self._mp_call = None

    # ---- what a subclass overrides -------------------------------------------------------------
    def message(self, x_j):
        return x_j

    def aggregate(self, inputs, index, ptr=None, dim_size=None):
        call = self._mp_call
        plan = None
        if call is not None:
            i = 1 if self.flow == "source_to_target" else 0
            if index is call.ends[i]:
                if dim_size is not None:
                    call.see(i, dim_size, "dim_size")
                elif call.size[i] is None:
                    call.size[i] = int(index.max()) + 1 if index.numel() else 0     # (no node tensor was seen: one host read, as PyG)
                plan, dim_size = call.plan(i), call.size[i]
        if plan is None:
            if dim_size is None:
                dim_size = int(index.max()) + 1 if index.numel() else 0
            plan = ops.rows_plan(index.contiguous(), dim_size, check="deferred")
        return ops.scatter(inputs, index, dim_size, reduce=self.aggr, plan=plan)

    def message_and_aggregate(self, adj_t):
        raise NotImplementedError

    def update(self, inputs):
        return inputs

    # ---- propagate -----------------------------------------------------------------------------
    @classmethod
    def _mp_params(cls):
        """{function name: [(parameter name, has a default)]}, read once per class (``aggregate`` / ``update`` without their first,
        positional, parameter)."""
        got = cls.__dict__.get("_mp_params_cache")
        if got is None:
            got = {}
            for fn, skip in (("message", 1), ("aggregate", 2), ("update", 2), ("message_and_aggregate", 2)):
                ps = list(inspect.signature(getattr(cls, fn)).parameters.values())[skip:]
                got[fn] = [(p.name, p.default is not _MP_EMPTY) for p in ps if p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]
            cls._mp_params_cache = got
        return got

    def _mp_collect(self, fn: str, call: _Propagation, kwargs: dict, lifted: dict) -> dict:
        j, i = (0, 1) if self.flow == "source_to_target" else (1, 0)
        params = self._mp_params()[fn]
        if fn == "message":
            # the lifts first: they settle the node counts the special names report
            for name, has_default in params:
                if name in _MP_SPECIAL or not name.endswith(("_i", "_j")):
                    continue
                base = name[:-2]
                if base not in kwargs:
                    if has_default:
                        continue
                    raise TypeError(f"MessagePassing.propagate: `message` needs `{name}`, but no `{base}` was given")
                data = kwargs[base]
                if isinstance(data, (tuple, list)):
                    if self.flow != "source_to_target":
                        raise NotImplementedError("MessagePassing: (source, target) pairs are supported for flow='source_to_target' only")
                    if len(data) != 2:
                        raise ValueError(f"MessagePassing.propagate: `{base}` must be a (source, target) pair")
                    data = data[0 if name.endswith("_j") else 1]
                lifted[name] = None if data is None else call.lift(data, j if name.endswith("_j") else i, self.node_dim, base)
            for e in (0, 1):     # a side no node tensor settled: the other side's count, as PyG does for a single node set
                if call.size[e] is None:
                    call.size[e] = call.size[1 - e]
        special = {"edge_index": call.edge_index, "edge_index_i": call.ends[i], "edge_index_j": call.ends[j], "index": call.ends[i],
                   "size": call.size, "size_i": call.size[i], "size_j": call.size[j], "dim_size": call.size[i], "ptr": call.ptr,
                   "adj_t": call.adj_t}
        out = {}
        for name, has_default in params:
            if name in special:
                out[name] = special[name]
            elif name in lifted:
                out[name] = lifted[name]
            elif name in kwargs:
                out[name] = kwargs[name]
            elif not has_default:
                raise TypeError(f"MessagePassing.propagate: `{fn}` needs `{name}`, which was not given")
        return out

    def _mp_default_fused(self, call: _Propagation, kwargs: dict):
        """The default ``message`` (``x_j``) under the default ``aggregate`` with a summing ``aggr``: lift and aggregation as ONE walk
        (``ops.gather_scatter``, bit-equal to ``ops.scatter(ops.take_rows(...))``), no [E, C] tensor.  None: the general path runs (and
        raises what it raises for operands it does not take)."""
        cls = type(self)
        if not (ops.FUSE_LAZY_ROWS and cls.message is MessagePassing.message and cls.aggregate is MessagePassing.aggregate
                and self.aggr in ("add", "sum", "mean") and "x" in kwargs):
            return None
        j, i = (0, 1) if self.flow == "source_to_target" else (1, 0)
        data = kwargs["x"]
        if isinstance(data, (tuple, list)):
            if self.flow != "source_to_target" or len(data) != 2:
                return None
            data = data[0]
        t = _lib.real(data)
        if not (isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 1 and (self.node_dim == 0 or t.dim() <= 2)):
            return None
        call.see(j, t.shape[0], "x")
        for e in (0, 1):     # a side no node tensor settled: the other side's count, as PyG does for a single node set
            if call.size[e] is None:
                call.size[e] = call.size[1 - e]
        return ops.gather_scatter(t, call.plan(j), call.plan(i), call.size[i], None, self.aggr)

    def propagate(self, edge_index, size=None, **kwargs):
        size = [None, None] if size is None else [None if s is None else int(s) for s in size]
        if len(size) != 2:
            raise ValueError("MessagePassing.propagate: `size` is None or a pair (sources, targets)")
        if isinstance(edge_index, SparseTensor):
            if self.flow != "source_to_target":
                raise NotImplementedError("MessagePassing: a SparseTensor adjacency is supported for flow='source_to_target' only")
            _lib.require_gpu(edge_index._col)
            if type(self).message_and_aggregate is not MessagePassing.message_and_aggregate:
                call = _Propagation((None, None), [edge_index.sparse_size(1), edge_index.sparse_size(0)], edge_index._rowptr, None, edge_index)
                out = self.message_and_aggregate(edge_index, **self._mp_collect("message_and_aggregate", call, kwargs, {}))
                return self.update(out, **self._mp_collect("update", call, kwargs, {}))
            row, col, _ = edge_index.coo()
            call = _Propagation((col, row), [edge_index.sparse_size(1), edge_index.sparse_size(0)], edge_index._rowptr, None, edge_index)
        else:
            if not (isinstance(edge_index, Tensor) and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.shape[0] == 2):
                raise TypeError("MessagePassing.propagate: `edge_index` must be an int64 tensor [2, E] or a SparseTensor")
            _lib.require_gpu(edge_index)
            call = _Propagation((edge_index[0], edge_index[1]), size, None, edge_index, None)
        outer, self._mp_call = self._mp_call, call
        _MP_RUNNING.append((call, 1 if self.flow == "source_to_target" else 0))
        try:
            lifted: dict = {}
            out = self._mp_default_fused(call, kwargs)
            if out is not None:
                return self.update(out, **self._mp_collect("update", call, kwargs, lifted))
            msg_kwargs = self._mp_collect("message", call, kwargs, lifted)
            out = self.message(**msg_kwargs)
            out = self.aggregate(out, **self._mp_collect("aggregate", call, kwargs, lifted))
            return self.update(out, **self._mp_collect("update", call, kwargs, lifted))
        finally:
            _MP_RUNNING.pop()
            self._mp_call = outer

    def __repr__(self):
        return f"{type(self).__name__}()"


# ------------------------------------------------------------------------------------------------
# graph classification: GIN / GINE convs, categorical encoders, graph-level readout (PyG <= 1.7 definitions [ext]: the reference's
# mol_pyg holds a README only)
# ------------------------------------------------------------------------------------------------
def _reset(module) -> None:
    """PyG's ``inits.reset``, with a module's own ``reset_parameters`` preferred at every level: a module that has one resets itself
    (and whatever it holds, by its own rule); a plain container hands the call to its children."""
    if hasattr(module, "reset_parameters"):
        module.reset_parameters()
    else:
        for child in module.children():
            _reset(child)


class _GINBase(MessagePassing):
    """What ``GINConv`` and ``GINEConv`` share: ``nn`` (the MLP applied to the combined row), ``eps`` (a buffer, or a ``Parameter``
    with ``train_eps``) and ``out = nn((1 + eps) * x_r + aggregated messages)``; state_dict keys ``nn.*`` and ``eps``."""

    def __init__(self, nn_module, eps: float = 0.0, train_eps: bool = False, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        self.nn = nn_module
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = nn.Parameter(torch.empty(1))
        else:
            self.register_buffer("eps", torch.empty(1))
        self.reset_parameters()

    def reset_parameters(self):
        _reset(self.nn)
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    @staticmethod
    def _node_pair(x, who: str):
        """``x`` as a ``(source, target)`` pair of REAL tensors: a deferred activation (``lazy.py``: what a ``BatchNorm1d`` hands out
        under ``accel``) is formed first -- it is no ``Tensor``, and indexing it like a pair would pick rows 0 and 1."""
        if isinstance(x, (tuple, list)):
            if len(x) != 2:
                raise ValueError(f"{who}: `x` must be a tensor or a (source, target) pair")
            pair = tuple(None if t is None else _lib.real(t) for t in x)
        else:
            x = _lib.real(x)
            pair = (x, x)
        if not isinstance(pair[0], Tensor) or not (pair[1] is None or isinstance(pair[1], Tensor)):
            raise TypeError(f"{who}: `x` must be a tensor or a (source, target) pair of tensors")
        return pair

    def _combine(self, out: Tensor, x_r) -> Tensor:
        if x_r is not None:
            out = out + (1 + self.eps) * x_r
        return self.nn(out)

    def __repr__(self):
        return f"{type(self).__name__}(nn={self.nn})"


class GINConv(_GINBase):
    """``torch_geometric.nn.GINConv`` (PyG <= 1.7 [ext]): ``out = nn((1 + eps) * x_r + sum_j x_j)``.  The default ``message`` under
    ``aggr="add"``: lift and sum are one walk (``ops.gather_scatter``).  ``x`` may be a ``(source, target)`` pair."""

    def forward(self, x, edge_index, size=None) -> Tensor:
        x = self._node_pair(x, "GINConv")
        return self._combine(self.propagate(edge_index, x=x, size=size), x[1])


class GINEConv(_GINBase):
    """``torch_geometric.nn.GINEConv`` (PyG <= 1.7 [ext]): ``out = nn((1 + eps) * x_r + sum_j relu(x_j + edge_attr_j))``;
    ``edge_attr`` [E, C] has the width of ``x``.  While ``message`` and ``aggregate`` are the class's own, lift, add, relu and sum are
    ONE walk over the call's two deferred plans (``ops.gather_add_scatter``: no [E, C] message tensor); a subclass that overrides
    ``message`` takes ``propagate``'s general path."""

    def forward(self, x, edge_index, edge_attr, size=None) -> Tensor:
        x = self._node_pair(x, "GINEConv")
        edge_attr = _lib.real(edge_attr)
        if not isinstance(edge_attr, Tensor):
            raise TypeError("GINEConv: `edge_attr` must be a tensor [E, C]")
        if edge_attr.dim() != 2 or edge_attr.shape[1] != x[0].shape[-1]:
            raise ValueError(f"GINEConv: node and edge feature widths do not match: x has {x[0].shape[-1]} columns, edge_attr is "
                             f"{list(edge_attr.shape)}")
        out = self._fused(x[0], x[1], edge_index, edge_attr, size)
        if out is None:
            out = self.propagate(edge_index, x=x, edge_attr=edge_attr, size=size)
        return self._combine(out, x[1])

    def message(self, x_j, edge_attr):
        return (x_j + edge_attr).relu()

    def _fused(self, x_src, x_dst, edge_index, edge_attr, size):
        """The class's own message and aggregation as one ``ops.gather_add_scatter`` (``_mp_default_fused``'s shape); None: the
        general path runs (and raises what it raises for operands it does not take)."""
        cls = type(self)
        if not (ops.FUSE_EDGE_ROWS and cls.message is GINEConv.message and cls.aggregate is MessagePassing.aggregate
                and cls.update is MessagePassing.update and self.aggr in ("add", "sum", "mean")
                and isinstance(edge_index, Tensor) and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.shape[0] == 2
                and edge_index.is_cuda and isinstance(x_src, Tensor) and x_src.is_cuda and x_src.dtype == torch.float32 and x_src.dim() == 2
                and isinstance(edge_attr, Tensor) and edge_attr.is_cuda and edge_attr.dtype == torch.float32
                and edge_attr.shape[0] == edge_index.shape[1]):
            return None
        j, i = (0, 1) if self.flow == "source_to_target" else (1, 0)
        if j != 0 and x_dst is not x_src:
            return None
        size = [None, None] if size is None else [None if s is None else int(s) for s in size]
        if len(size) != 2:
            return None
        call = _Propagation((edge_index[0], edge_index[1]), size, None, edge_index, None)
        call.see(j, x_src.shape[0], "x")
        if x_dst is not None:
            call.see(i, x_dst.shape[0], "x")
        for e in (0, 1):
            if call.size[e] is None:
                call.size[e] = call.size[1 - e]
        return ops.gather_add_scatter(x_src, call.plan(j), call.plan(i), call.size[i], edge_attr, "relu", self.aggr)


ATOM_DIMS = (119, 4, 12, 12, 10, 6, 6, 2, 2)     # [ext] the cardinalities of OGB's nine atom feature columns (ogb.utils.features)
BOND_DIMS = (5, 6, 2)                             # [ext] and of its three bond feature columns


class CategoricalEncoder(nn.Module):
    """``out = sum_k table_k[attr[:, k]]`` for integer attributes ``attr`` [n, K]: what OGB's ``AtomEncoder`` / ``BondEncoder`` compute
    [ext], with the cardinalities as arguments (``ATOM_DIMS`` / ``BOND_DIMS``).  Tables ``embeddings.k.weight`` [cardinality, emb_dim],
    xavier-uniform.  Each lookup is ``ops.take_rows(..., duplicates="sum")``: a table row named by many nodes gets the deterministic
    run-sum as its gradient, and an id outside its table raises ``IndexError``."""

    def __init__(self, cardinalities, emb_dim: int):
        super().__init__()
        cards = [int(c) for c in cardinalities]
        if not cards or any(c < 1 for c in cards):
            raise ValueError(f"CategoricalEncoder: cardinalities must be a non-empty list of positive sizes, got {list(cardinalities)!r}")
        if int(emb_dim) < 1:
            raise ValueError(f"CategoricalEncoder: emb_dim must be positive, got {emb_dim!r}")
        self.cardinalities, self.emb_dim = tuple(cards), int(emb_dim)
        self.embeddings = nn.ModuleList(nn.Embedding(c, self.emb_dim) for c in cards)
        self.reset_parameters()

    def reset_parameters(self):
        for emb in self.embeddings:
            nn.init.xavier_uniform_(emb.weight.data)

    def forward(self, attr: Tensor) -> Tensor:
        if not isinstance(attr, Tensor) or attr.dtype != torch.int64 or attr.dim() != 2 or attr.shape[1] != len(self.cardinalities):
            raise ValueError(f"CategoricalEncoder: `attr` must be an int64 tensor [n, {len(self.cardinalities)}]")
        _lib.require_gpu(attr, self.embeddings[0].weight)
        if attr.shape[0] == 0:
            return self.embeddings[0].weight.new_zeros((0, self.emb_dim))
        out = None
        for k, emb in enumerate(self.embeddings):
            rows = ops.take_rows(emb.weight, attr[:, k].contiguous(), duplicates="sum")
            out = rows if out is None else out + rows
        return out


def _global_pool(x: Tensor, batch: Tensor, size, reduce: str) -> Tensor:
    x = _lib.real(x)
    if not (isinstance(batch, Tensor) and batch.dtype == torch.int64 and batch.dim() == 1):
        raise TypeError("global pool: `batch` must be a 1-D int64 tensor with the graph id of every node")
    if not isinstance(x, Tensor) or x.dim() < 1 or x.shape[0] != batch.numel():
        raise ValueError("global pool: `x` needs one row per entry of `batch`")
    _lib.require_gpu(x, batch)
    if size is None:
        size = int(batch.max()) + 1 if batch.numel() else 0          # (one host read, as PyG)
        return ops.scatter(x, batch, size, reduce)
    size = int(size)
    if size == 0 or batch.numel() == 0:
        return x.new_zeros((size,) + tuple(x.shape[1:]))
    return ops.scatter(x, None, size, reduce, plan=ops.rows_plan(batch.contiguous(), size, check="deferred"))


def global_add_pool(x: Tensor, batch: Tensor, size=None) -> Tensor:
    """``torch_geometric.nn.global_add_pool``: ``out[g] = sum of x[n] over batch[n] == g`` -> [size, ...] (``ops.scatter``: no float
    atomics).  ``size`` given: a deferred plan, no host read; None: ``batch.max() + 1`` is read once, as PyG does.  A graph id that
    owns no node gives a zero row."""
    return _global_pool(x, batch, size, "sum")


def global_mean_pool(x: Tensor, batch: Tensor, size=None) -> Tensor:
    """``torch_geometric.nn.global_mean_pool``; see ``global_add_pool``."""
    return _global_pool(x, batch, size, "mean")


def global_max_pool(x: Tensor, batch: Tensor, size=None) -> Tensor:
    """``torch_geometric.nn.global_max_pool``; see ``global_add_pool`` (a graph id that owns no node gives a zero row)."""
    return _global_pool(x, batch, size, "max")
