"""Deferred activations for the reference's UNMODIFIED model code (dropin/accel.py).

``arxiv_pyg/gnn.py:47-51`` spells a hidden layer as four calls of its own::

    x = conv(x, adj_t); x = self.bns[i](x); x = F.relu(x); x = F.dropout(x, p=self.dropout, training=self.training)

and ``gnn.py:150`` reads ``student_proj(model.out_feat[train_idx])``.  The package's own loop runs each of these groups as ONE
launch (``ops.bn_act`` / ``ops.bn_act_linear`` / ``ops.linear_rows``); the script calls them by name, one at a time.  Under
``accel.enable()`` the re-pointed ``BatchNorm1d.forward`` therefore does the part that must happen NOW (batch statistics + the
module's running-statistics update) and returns a ``LazyBnAct``: a tensor-like object (``__torch_function__`` protocol) that

  * absorbs a following ``F.relu`` and ``F.dropout`` (any other torch function, method or operator materialises it first and then
    runs on the real tensor -- nothing is ever silently skipped);
  * is materialised by its first real consumer with ONE fused launch -- by the next ``GCNConv`` together with its narrow ``h @ W``
    (``ops.bn_act_linear``) when the shapes allow, by a sampled criterion as only the sampled rows (``pick``);
  * answers ``lazy[idx]`` for a 1-D int64 index with a ``LazyRows`` that a following ``Linear`` turns into the gather-fused GEMM
    (``ops.linear_rows``: no ``[N_tr, 256]`` copy forward, no zero-fill + scatter backward).

``nn.MessagePassing`` hands out a lifted ``x_j`` as a ``LazyRows`` too; times a per-edge weight it becomes a ``LazyWeightedRows``, which
``ops.scatter`` (sum / add / mean) runs as ONE ``ops.gather_scatter`` -- lift, weight and aggregation without an [E, C] tensor.  Plus a
per-edge ROW (``x_j + edge_attr``, then ``relu``) it becomes a ``LazyEdgeRows``, which ``ops.scatter`` runs as ONE ``ops.gather_add_scatter``.

Inference (``model.eval()`` under ``no_grad``): a ``GCNConv`` that has been SEEN feeding a ``BatchNorm1d`` (``accel`` learns the association
from the first forward; it only decides what is deferred) hands out a ``LazyConv``; the eval-mode BatchNorm turns it into a ``LazyFold``
that absorbs the ReLU and is formed as ONE pass -- the BatchNorm folded into the conv's weights, the ReLU in the last kernel's store.
In training the same association gives the BatchNorm its statistics out of the aggregation's epilogue.

Same arithmetic as ``models.train_step`` (the kernels are the same); dropout masks come from the same counter hash (one host seed per
materialised dropout).  Consumers inside the package ask through ``materialise(x)`` / the ``_egnn_materialise`` attribute.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _cache, ops


ACCEL_ACTIVE = False   # set by dropin/accel.py's enable() / disable(): torch.nn.Linear.forward consumes a LazyRows
_MUL_FUNCS = (torch.mul, torch.multiply, torch.Tensor.mul, torch.Tensor.multiply, torch.Tensor.__mul__, torch.Tensor.__rmul__)
_ADD_FUNCS = (torch.add, torch.Tensor.add, torch.Tensor.__add__, torch.Tensor.__radd__)
_RELU_FUNCS = (F.relu, torch.relu, torch.Tensor.relu)


def _on_gpu(t) -> bool:
    return t.is_cuda


def materialise(x, pick=None):
    """``x`` as a real tensor (``x[pick]`` when ``pick`` is given): deferred objects are formed now, tensors pass through."""
    m = getattr(x, "_egnn_materialise", None)
    if m is not None:
        return m(pick=pick)
    return x if pick is None else x[pick]


class _TensorLike:
    """Everything a consumer might do with a tensor that this module does not defer: materialise, then delegate."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = cls._absorb(func, args, kwargs)
        if out is not NotImplemented:
            return out
        real = lambda v: v._egnn_materialise() if isinstance(v, _TensorLike) else v   # noqa: E731
        args = tuple(type(a)(real(v) for v in a) if isinstance(a, (list, tuple)) else real(a) for a in args)
        kwargs = {k: real(v) for k, v in kwargs.items()}
        return func(*args, **kwargs)

    @classmethod
    def _absorb(cls, func, args, kwargs):
        return NotImplemented

    def __getattr__(self, name):       # methods / attributes of the real tensor (.t(), .sum(), .requires_grad, ...)
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._egnn_materialise(), name)

    def __len__(self):
        return self.shape[0]

    def __iter__(self):
        return iter(self._egnn_materialise())

    def __repr__(self):
        return f"{type(self).__name__}(shape={tuple(self.shape)}, deferred={self._value is None})"

    def dim(self):
        return len(self.shape)

    def size(self, d=None):
        return torch.Size(self.shape) if d is None else self.shape[d]

    dtype = torch.float32
    is_cuda = True


def _binary(name):
    def op(self, other):
        return getattr(self._egnn_materialise(), name)(materialise(other))
    op.__name__ = name
    return op


for _n in ("__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__rtruediv__", "__matmul__", "__rmatmul__",
           "__pow__", "__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__"):
    setattr(_TensorLike, _n, _binary(_n))
_TensorLike.__neg__ = lambda self: -self._egnn_materialise()
_TensorLike.__hash__ = object.__hash__


class LazyBnAct(_TensorLike):
    """``dropout(relu?(bn(x)), p)`` with the statistics already taken; see the module docstring."""

    def __init__(self, src, relu=False, p=0.0):
        self._src, self._relu, self._p, self._value = src, relu, p, None

    @staticmethod
    def from_bn(bn, x, training):
        """The part of ``BatchNorm1d.forward`` that cannot wait: statistics (or the producing aggregation's), running-statistics update.
        None when the fused kernels do not take the shape (the caller falls back to torch's forward)."""
        prep = ops._bn_prepare(x, bn, 0.0, training)
        if prep is None:
            return None
        xr, mean, var, use_batch, _, _ = prep
        return LazyBnAct(dict(x=xr, bn=bn, mean=mean, var=var, use_batch=use_batch, training=training))

    shape = property(lambda self: self._src["x"].shape)
    device = property(lambda self: self._src["x"].device)

    @classmethod
    def _absorb(cls, func, args, kwargs):
        x = args[0] if args else None
        if not isinstance(x, LazyBnAct) or x._value is not None:
            return NotImplemented
        if func in (F.relu, torch.relu) and not kwargs.get("inplace", False) and len(args) == 1 and x._p == 0.0:
            return x if x._relu else LazyBnAct(x._src, True, 0.0)
        if func is F.dropout and not kwargs.get("inplace", False) and len(args) <= 3:
            p = args[1] if len(args) > 1 else kwargs.get("p", 0.5)
            training = args[2] if len(args) > 2 else kwargs.get("training", True)
            if not training or p == 0.0:
                return x                          # F.dropout outside training is the identity
            if x._p == 0.0 and 0.0 < p < 1.0:
                return LazyBnAct(x._src, x._relu, float(p))
        return NotImplemented

    def _args(self):
        s = self._src
        drop = self._p if (s["training"] and self._p > 0) else 0.0
        seed = ops._draw_dropout_seed() if drop > 0 else 0
        return s["x"], s["bn"].weight, s["bn"].bias, s["mean"], s["var"], s["bn"].eps, self._relu, drop, seed, s["use_batch"]

    def _egnn_materialise(self, pick=None):
        if self._value is None:
            if pick is not None:   # only the rows a sampled criterion keeps (not cached: the full tensor was never asked for)
                return ops._BnAct.apply(*self._args(), pick)
            v = ops._BnAct.apply(*self._args(), None)
            # two consumers are the rule for the last hidden state (the next conv, and student_proj(out_feat[train_idx])): the
            # row-compact gradient of the second joins the dense one of the first (ops.grad_tap)
            self._value = ops.grad_tap(v) if self._src["training"] else v
        return self._value if pick is None else self._value[pick]

    def materialise_with_linear(self, w):
        """(h, h @ w) in one op for a narrow ``w`` (``ops.bn_act_linear``'s kernels); None when they do not take the shape."""
        s = self._src
        x = s["x"]
        if self._value is not None or not (torch.is_grad_enabled() and s["training"] and s["use_batch"] and type(s["bn"]) is torch.nn.BatchNorm1d
                                           and w.dim() == 2 and w.shape[0] == x.shape[1] and w.shape[1] <= 64 and x.shape[1] % 64 == 0):
            return None
        box = ops._TapBox()
        h, xw = ops._BnActLinear.apply(*self._args(), w, box)
        h._egnn_tap = box
        self._value = h
        return h, xw

    def __getitem__(self, idx):
        if isinstance(idx, torch.Tensor) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_cuda:
            return LazyRows(self, idx)
        return self._egnn_materialise()[idx]


class LazyConv(_TensorLike):
    """``conv(x, adj_t)`` of an inference forward (``model.eval()``, ``no_grad``), not run yet.  Only handed out by a ``GCNConv`` that has
    been SEEN to feed a ``BatchNorm1d`` (the association is learned from the first forward, and only decides what is deferred -- any
    consumer forms the same values): the BatchNorm turns it into a ``LazyFold``; everything else runs the conv now."""

    def __init__(self, conv, x, adj_t, run):
        self._conv, self._x, self._adj, self._run, self._value = conv, x, adj_t, run, None

    shape = property(lambda self: torch.Size((self._x.shape[0], self._conv.out_channels)))
    device = property(lambda self: self._x.device)

    def _egnn_materialise(self, pick=None):
        if self._value is None:
            self._value = self._run(self._conv, self._x, self._adj)
            self._value._egnn_producer = self._conv
        return self._value if pick is None else self._value[pick]

    def __getitem__(self, idx):
        return self._egnn_materialise()[idx]


class LazyFold(_TensorLike):
    """``bn(conv(x, adj_t))`` in eval mode, deferred: with a following ``F.relu`` absorbed it is formed by ONE pass -- the BatchNorm folded
    into the conv's weights and bias, the ReLU in the last kernel's store (``GCNConv.forward(eval_bn=)``: what ``models.evaluate`` runs;
    gnn.py:47-49 under ``model.eval()``) -- instead of conv + a normalisation pass + a ReLU pass."""

    def __init__(self, lazy_conv, bn, relu=False):
        self._lc, self._bn, self._relu, self._value = lazy_conv, bn, relu, None

    shape = property(lambda self: self._lc.shape)
    device = property(lambda self: self._lc.device)

    @classmethod
    def _absorb(cls, func, args, kwargs):
        x = args[0] if args else None
        if not isinstance(x, LazyFold) or x._value is not None:
            return NotImplemented
        if func in (F.relu, torch.relu) and not kwargs.get("inplace", False) and len(args) == 1:
            return x if x._relu else LazyFold(x._lc, x._bn, True)
        if func is F.dropout and not kwargs.get("inplace", False) and len(args) <= 3:
            training = args[2] if len(args) > 2 else kwargs.get("training", True)
            p = args[1] if len(args) > 1 else kwargs.get("p", 0.5)
            if not training or p == 0.0:
                return x
        return NotImplemented

    def _egnn_materialise(self, pick=None):
        if self._value is None:
            lc, bn = self._lc, self._bn
            if self._relu and lc._value is None and not torch.is_grad_enabled() and not bn.training:
                self._value = lc._run(lc._conv, lc._x, lc._adj, eval_bn=bn)   # fold + ReLU in the last kernel's store
            else:
                y = ops.bn_act(lc._egnn_materialise(), bn, relu=self._relu, p=0.0, training=False)
                self._value = y
        return self._value if pick is None else self._value[pick]

    def __getitem__(self, idx):
        if isinstance(idx, torch.Tensor) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_cuda:
            return LazyRows(self, idx)
        return self._egnn_materialise()[idx]


_COMPOSED = _cache.TensorKeyedCache(capacity=16)     # (idx, idx2) -> idx[idx2]: one tensor, hence one ops.rows_plan, per pair and not per step


class LazyRows(_TensorLike):
    """``base[idx]`` (1-D int64 ids of unknown provenance: they may repeat rows, be negative or out of range) not gathered yet: a ``Linear``
    consumes it as ``ops.linear_rows(base, idx, W, b)``.  Every gather passes ``duplicates="sum"``: torch's ``x[idx]`` rules (ops.rows_plan;
    unique ids take the same kernels as before).  A ``torch.Tensor`` base is read when the rows are formed, not when they were asked for:
    its version is recorded, and a base changed in place in between raises instead of handing out the changed rows."""

    def __init__(self, base, idx, const_base=False, base_version=None, plan=None):
        # ``plan``: a callable returning the ready ``ops.RowsPlan`` of ``idx`` (nn.MessagePassing shares one per endpoint: the gather,
        # its backward and the aggregation walk the same keys); None: the host-checked plan of ``idx`` is built (and cached)
        self._base, self._idx, self._value, self._const, self._plan = base, idx, None, const_base, plan
        self._base_version = base_version if base_version is not None else (base._version if isinstance(base, torch.Tensor) else None)

    shape = property(lambda self: torch.Size((self._idx.numel(),) + tuple(self._base.shape[1:])))
    device = property(lambda self: self._idx.device)

    def _formed_base(self):
        base = self._base
        if self._base_version is not None and base._version != self._base_version:
            raise RuntimeError(f"one of the variables needed for a deferred row gather has been modified by an inplace operation: the indexed "
                               f"tensor {list(base.shape)} is at version {base._version}; expected version {self._base_version} instead "
                               f"(x[idx] under accel is formed by its first consumer: clone x before changing it in place)")
        return materialise(base)

    def _egnn_materialise(self, pick=None):
        if self._value is None:
            base = self._formed_base()
            if pick is not None:
                return self._take(base, self._composed(pick))
            self._value = self._take(base, self._idx if self._plan is None else self._plan())
        return self._value if pick is None else self._value[pick]

    @staticmethod
    def _take(base, idx):
        # (accel only defers GPU indices; rows of a CPU tensor are torch's own indexing, which has x[idx]'s rules by definition)
        return ops.take_rows(base, idx, duplicates="sum") if isinstance(idx, ops.RowsPlan) or idx.is_cuda else base[idx]

    def _edge_weight(self, other):
        """True when ``rows * other`` is a per-edge weight ``ops.gather_scatter`` takes: a float32 GPU tensor [E, 1] (2-D rows), [E, H, 1]
        or [E, 1, 1] (rows [E, H, D]) -- the shapes torch broadcasts along the edges -- a 0-dim one or a Python number."""
        if self._value is not None or not ops.FUSE_LAZY_ROWS or not isinstance(self._base, torch.Tensor) or self._base.dim() not in (2, 3):
            return False
        if isinstance(other, (int, float)) and not isinstance(other, bool):
            return _on_gpu(self._base)
        if not (type(other) in (torch.Tensor, torch.nn.Parameter) and other.dtype == torch.float32 and _on_gpu(other) and _on_gpu(self._base)):
            return False
        E, rest = self._idx.numel(), tuple(self._base.shape[1:])
        if other.dim() == 0:
            return True
        if len(rest) == 1:
            return tuple(other.shape) == (E, 1)
        return tuple(other.shape) in ((E, rest[0], 1), (E, 1, 1))

    def __mul__(self, other):
        if self._edge_weight(other):
            return LazyWeightedRows(self, other)
        return self._egnn_materialise() * materialise(other)

    __rmul__ = __mul__

    def _edge_rows(self, other):
        """True when ``rows + other`` is the per-edge row ``ops.gather_add_scatter`` takes: unformed 2-D rows and a float32 GPU tensor
        of exactly their shape [E, C] (anything torch would broadcast, a scalar or another dtype forms the rows)."""
        if self._value is not None or not (ops.FUSE_EDGE_ROWS and ops.FUSE_LAZY_ROWS) or not isinstance(self._base, torch.Tensor):
            return False
        if self._base.dim() != 2 or type(other) not in (torch.Tensor, torch.nn.Parameter):
            return False
        return other.dtype == torch.float32 and _on_gpu(other) and _on_gpu(self._base) and tuple(other.shape) == tuple(self.shape)

    def __add__(self, other):
        if self._edge_rows(other):
            return LazyEdgeRows(self, other)
        return self._egnn_materialise() + materialise(other)

    __radd__ = __add__

    @classmethod
    def _absorb(cls, func, args, kwargs):
        if func in _ADD_FUNCS and len(args) == 2 and not kwargs:
            a, b = args
            if isinstance(b, LazyRows) and not isinstance(a, _TensorLike):
                a, b = b, a
            if isinstance(a, LazyRows) and not isinstance(b, _TensorLike) and a._edge_rows(b):
                return LazyEdgeRows(a, b)
        if func in _MUL_FUNCS and len(args) == 2 and not kwargs:
            a, b = args
            if isinstance(b, LazyRows) and not isinstance(a, _TensorLike):
                a, b = b, a
            if isinstance(a, LazyRows) and not isinstance(b, _TensorLike) and a._edge_weight(b):
                return LazyWeightedRows(a, b)
        return NotImplemented

    def _egnn_gather_scatter(self, dst, dim_size, reduce, weight=None):
        """``ops.scatter`` of these rows (times ``weight``) as one ``ops.gather_scatter``; None when the rows exist already or the
        base is not a float32 GPU tensor (the caller then forms them)."""
        if self._value is not None or not (isinstance(self._idx, torch.Tensor) and _on_gpu(self._idx)):
            return None
        base = self._formed_base()
        if not (isinstance(base, torch.Tensor) and _on_gpu(base) and base.dtype == torch.float32 and base.dim() >= 2):
            return None
        E = self._idx.numel()
        if isinstance(weight, (int, float)):
            weight = torch.full((E,), float(weight), dtype=torch.float32, device=base.device)
        elif weight is not None and weight.dim() == 0:
            weight = weight.expand(E)
        elif weight is not None and weight.dim() == 3 and weight.shape[1] == 1:
            weight = weight.reshape(E)
        return ops.gather_scatter(base, self._idx if self._plan is None else self._plan(), dst, dim_size, weight, reduce)

    def linear(self, weight, bias):
        if len(self.shape) != 2:          # rows [E, H, D]: F.linear acts on the last axis of the formed rows
            return F.linear(self._egnn_materialise(), weight, bias)
        base = self._formed_base()
        # ``const_base``: the gathered-from tensor is a leaf outside autograd (accel's deferred constant gather): its rows as once-cut planes
        const = bool(self._const and not base.requires_grad and base.grad_fn is None)
        return ops.linear_rows(base, self._idx if self._plan is None else self._plan(), weight, bias, const_input=const, duplicates="sum")

    def _composed(self, idx2):
        """``idx[idx2]``, memoised on the pair: a script composes it anew every step, its plan is built once."""
        idx = self._idx
        if not (isinstance(idx2, torch.Tensor) and idx2.dtype == torch.int64 and idx2.dim() == 1):
            return idx[idx2]
        return _COMPOSED.get((idx, idx2), (), lambda: idx[idx2])

    def __getitem__(self, idx):
        if isinstance(idx, torch.Tensor) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_cuda and self._value is None:
            return LazyRows(self._base, self._composed(idx), self._const, self._base_version)
        return self._egnn_materialise()[idx]


class LazyWeightedRows(_TensorLike):
    """``rows * weight`` for an unformed ``LazyRows`` and a per-edge weight (``LazyRows._edge_weight``), not multiplied yet: the
    messages of a GCN-style (``edge_weight.view(-1, 1) * x_j``) or attention (``x_j * alpha.unsqueeze(-1)``) conv.  ``ops.scatter`` with
    a summing reduce consumes it as ONE ``ops.gather_scatter`` -- no [E, C] tensor forward or backward; every other consumer (a second
    multiply included) gets exactly ``take_rows(...) * weight``."""

    def __init__(self, rows, weight):
        self._rows, self._weight, self._value = rows, weight, None

    shape = property(lambda self: self._rows.shape)
    device = property(lambda self: self._rows.device)

    def _egnn_materialise(self, pick=None):
        if self._value is None:
            self._value = self._rows._egnn_materialise() * self._weight
        return self._value if pick is None else self._value[pick]

    def _egnn_gather_scatter(self, dst, dim_size, reduce):
        if self._value is not None:
            return None
        return self._rows._egnn_gather_scatter(dst, dim_size, reduce, self._weight)

    def __getitem__(self, idx):
        return self._egnn_materialise()[idx]


class LazyEdgeRows(_TensorLike):
    """``rows + edge`` (then ``relu``) for an unformed 2-D ``LazyRows`` and a per-edge row tensor of its shape (``LazyRows._edge_rows``),
    not added yet: the message ``F.relu(x_j + edge_attr)`` of an edge-feature conv.  ``ops.scatter`` with a summing reduce consumes it
    as ONE ``ops.gather_add_scatter`` -- no [E, C] tensor forward, ``edge``'s gradient the only one backward; every other consumer (a
    second add, a second relu, an in-place relu included) gets exactly ``take_rows(...) + edge`` (then ``relu``).  ``edge`` is read
    when the rows are consumed: its version is recorded, and an ``edge`` changed in place in between raises, as a changed base does."""

    def __init__(self, rows, edge, act=None, edge_version=None):
        self._rows, self._edge, self._act, self._value = rows, edge, act, None
        self._edge_version = edge._version if edge_version is None else edge_version

    def _current_edge(self):
        edge = self._edge
        if edge._version != self._edge_version:
            raise RuntimeError(f"one of the variables needed for a deferred message has been modified by an inplace operation: the edge "
                               f"rows {list(edge.shape)} are at version {edge._version}; expected version {self._edge_version} instead "
                               f"(x_j + edge_attr under accel is formed by its first consumer: clone edge_attr before changing it in place)")
        return edge

    shape = property(lambda self: self._rows.shape)
    device = property(lambda self: self._rows.device)

    @classmethod
    def _absorb(cls, func, args, kwargs):
        x = args[0] if args else None
        if (isinstance(x, LazyEdgeRows) and x._value is None and x._act is None and func in _RELU_FUNCS and len(args) == 1
                and not kwargs.get("inplace", False) and not (set(kwargs) - {"inplace"})):
            return LazyEdgeRows(x._rows, x._edge, "relu", x._edge_version)
        return NotImplemented

    def relu(self):
        if self._value is None and self._act is None:
            return LazyEdgeRows(self._rows, self._edge, "relu", self._edge_version)
        return self._egnn_materialise().relu()

    def _egnn_materialise(self, pick=None):
        if self._value is None:
            v = self._rows._egnn_materialise() + self._current_edge()
            self._value = torch.relu(v) if self._act == "relu" else v
        return self._value if pick is None else self._value[pick]

    def _egnn_gather_scatter(self, dst, dim_size, reduce):
        rows = self._rows
        if self._value is not None or rows._value is not None or not (ops.FUSE_EDGE_ROWS and ops.FUSE_LAZY_ROWS):
            return None
        if not (isinstance(rows._idx, torch.Tensor) and _on_gpu(rows._idx)):
            return None
        base = rows._formed_base()
        if not (isinstance(base, torch.Tensor) and _on_gpu(base) and base.dtype == torch.float32 and base.dim() == 2):
            return None
        return ops.gather_add_scatter(base, rows._idx if rows._plan is None else rows._plan(), dst, dim_size, self._current_edge(), self._act, reduce)

    def __getitem__(self, idx):
        return self._egnn_materialise()[idx]
