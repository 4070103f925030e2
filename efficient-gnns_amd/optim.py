"""Row-lazy Adam for large embedding tables (the MAG ``emb_dict`` of mag_pyg/gnn.py:100-108, stepped by the dense
``torch.optim.Adam(model.parameters())`` of :424), equal to dense Adam.

Under dense Adam a row whose gradient is zero still moves: ``m`` and ``v`` decay and ``p`` goes on changing while ``m != 0``.  A plain
sparse Adam would therefore not give the reference's parameters.  ``LazyRowAdam`` touches only the rows of the batch and still does:
every table row records the last step it is current for, and before a row is read (``ops.group_input``) or stepped, the zero-gradient
steps it missed are replayed in registers (csrc/adam_rows.hip).  Nothing dense is formed per step: no ``param.grad``, no zero fill.

Semantics worth knowing:
  * between flushes ``param.data`` holds rows that are BEHIND (each by its own number of steps).  Read a lazily stepped table through
    ``ops.group_input`` (which catches the rows it reads up), or call ``flush()`` first -- ``state_dict()``, ``RGCN.inference`` and
    ``mag_train_epoch`` do.  After ``flush()`` the table, ``m`` and ``v`` are what dense Adam holds;
  * the per-step scalars ``lr_t / (1 - beta1^t)`` and ``sqrt(1 - beta2^t)`` live in two rings of ``_lib.ADAM_MAX_LAG`` = 64 steps, filled
    in double from the group's CURRENT ``lr`` at each step (a scheduler's change applies to the steps it was set for).  No row may lag
    further behind than the ring reaches, so every 64th step flushes first (one pass over the rows that ever had a gradient);
  * unique rows: a batch must name a table row at most once (GraphSAINT batches do).  A duplicate is not a fault: one of the two
    gradient rows is applied, the other is counted on the device, and the next ``flush()`` raises ``RuntimeError`` naming the table;
  * ``duplicates="sum"`` lifts both restrictions: a step takes any number of deposits per table (several ``backward()`` calls, or the
    gathered batches of several ranks), a table row may be named any number of times, and its gradient is ``grad_scale`` times the sum
    of its gradient rows in the order they were deposited -- one Adam step per row, no float atomics, no dense gradient
    (egnn_adam_rows_step_sum_f32).  The default ``"refuse"`` is the unique-rows path above, unchanged;
  * lifetime: the row state hangs on the Parameter (``param._egnn_rows``) and belongs to ONE optimiser.  ``LazyRowAdam.close()`` flushes
    and detaches it; do that before the tables are handed to another optimiser, re-initialised (``reset_parameters``) or moved
    (``model.to``).  A state whose optimiser is gone is flushed and dropped by the next reader (``row_state``), and a new ``LazyRowAdam``
    over the same table closes the old state first -- a table never stays on the lazy path without an optimiser that steps it.
"""
from __future__ import annotations

import ctypes
import math
import weakref

import torch

from . import _lib

MAX_LAG = _lib.ADAM_MAX_LAG


class AdamRing:
    """The two host rings of egnn_adam_rows_t: entry ``t % MAX_LAG`` holds ``lr_t / (1 - beta1^t)`` and ``sqrt(1 - beta2^t)``, formed in
    Python double and rounded to fp32 once (by the ctypes store), exactly the two scalars torch.optim.Adam's single-tensor path forms."""

    def __init__(self, beta1: float, beta2: float):
        self.beta1, self.beta2 = float(beta1), float(beta2)
        self.step_size = (ctypes.c_float * MAX_LAG)()
        self.bc2_sqrt = (ctypes.c_float * MAX_LAG)()

    def fill(self, t: int, lr: float) -> None:
        self.step_size[t % MAX_LAG] = float(lr) / (1.0 - self.beta1 ** t)
        self.bc2_sqrt[t % MAX_LAG] = math.sqrt(1.0 - self.beta2 ** t)


class RowState:
    """What the row-lazy Adam keeps for ONE table, attached to the Parameter as ``param._egnn_rows`` so that its readers
    (``ops.group_input``, ``RGCN.inference``) find it: ``m``, ``v``, the per-row step stamps ``last`` (int32, -1 = never had a gradient),
    the device counter of refused batch rows, the rings, the step ``t`` the table stands at and the last flushed step."""

    def __init__(self, param: torch.Tensor, group: dict, name: str, owner=None):
        _lib.require_gpu(param)
        self.owner = weakref.ref(owner) if owner is not None else None
        if param.dim() != 2 or param.dtype != torch.float32 or not param.is_contiguous() or param.shape[1] % 4 != 0:
            raise _lib.HipExtensionError(f"LazyRowAdam: table {name} must be a contiguous 2-D fp32 tensor with D % 4 == 0, got "
                                         f"{tuple(param.shape)} {param.dtype}")
        self.param, self.group, self.name = param, group, name
        self.m = torch.zeros_like(param.data)
        self.v = torch.zeros_like(param.data)
        self.last = torch.full((param.shape[0],), -1, dtype=torch.int32, device=param.device)
        self.dup = torch.zeros(1, dtype=torch.int32, device=param.device)
        self.t = 0
        self.flushed = 0
        self.ring = AdamRing(*group["betas"])
        self.deposits: list = []

    def _desc(self, step: int) -> "_lib.AdamRows":
        p = self.param.data
        b1, b2 = (float(b) for b in self.group["betas"])
        d = _lib.AdamRows()
        d.p, d.m, d.v, d.last = p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.last.data_ptr()
        d.n_rows, d.D, d.ld = p.shape[0], p.shape[1], p.stride(0)
        d.beta1, d.beta2, d.eps = b1, b2, float(self.group["eps"])
        d.one_minus_beta1, d.one_minus_beta2 = 1.0 - b1, 1.0 - b2
        d.step, d.flushed = step, self.flushed
        ctypes.memmove(d.step_size, self.ring.step_size, ctypes.sizeof(self.ring.step_size))
        ctypes.memmove(d.bc2_sqrt, self.ring.bc2_sqrt, ctypes.sizeof(self.ring.bc2_sqrt))
        d.dup_count = self.dup.data_ptr()
        return d

    def catch_up(self, type_id: int, node_type: "torch.Tensor | None", local_idx: torch.Tensor) -> None:
        """Bring the table rows ``local_idx[node_type == type_id]`` up to step ``t`` (every ``local_idx`` when ``node_type`` is None)."""
        if self.t == self.flushed or local_idx.numel() == 0:
            return                                              # every row that ever had a gradient is current
        with torch.cuda.device(self.param.device):
            _lib.check(_lib.load().egnn_adam_rows_catchup_f32(ctypes.byref(self._desc(self.t)), int(type_id), _lib.ptr(node_type),
                                                              _lib.ptr(local_idx), local_idx.numel(), _lib.stream()),
                       "egnn_adam_rows_catchup_f32")

    def _flush_to(self, step: int) -> None:
        if step > self.flushed:
            with torch.cuda.device(self.param.device):
                _lib.check(_lib.load().egnn_adam_rows_flush_f32(ctypes.byref(self._desc(step)), _lib.stream()), "egnn_adam_rows_flush_f32")
            self.flushed = step

    def flush(self) -> None:
        """Every row up to step ``t``; raises ``RuntimeError`` if a step since the last flush refused batch rows."""
        self._flush_to(self.t)
        refused = int(self.dup.item())
        if refused:
            self.dup.zero_()
            raise RuntimeError(f"LazyRowAdam: {refused} gradient row(s) of table {self.name} were not applied since the last flush: a batch "
                               "named a table row more than once (or a row outside the table, or one that had not been read through "
                               "ops.group_input in that step); batches must list unique rows")

    def deposit(self, grad_h: torch.Tensor, node_type: "torch.Tensor | None", local_idx: torch.Tensor, type_id: int) -> None:
        """Called by the backward of ``ops.group_input``: the gradient rows of this step, applied by ``LazyRowAdam.step``."""
        self.deposits.append((grad_h, node_type, local_idx, int(type_id)))

    def _merged_deposits(self, cache: dict):
        """The deposits of this step as ONE list ``(g, node_type, local_idx, type_id)``, concatenated in the order they were made.
        ``cache`` is shared by the tables of one optimiser step: they usually hold the same tensors (one ``ops.group_input`` backward
        deposits its arrays with every table), which are then concatenated once."""
        deps, self.deposits = self.deposits, []
        if len(deps) == 1:
            return deps[0]
        ids = {d[3] for d in deps}
        if len(ids) == 1 and all(d[1] is not None for d in deps):
            key = tuple(id(x) for d in deps for x in d[:3])
            if key not in cache:
                cache[key] = (deps, torch.cat([d[0] for d in deps]), torch.cat([d[1] for d in deps]), torch.cat([d[2] for d in deps]))
            _, g, node_type, local_idx = cache[key]
            return g, node_type, local_idx, deps[0][3]
        # deposits under different type ids, or without a type vector: select with a 0 / 1 vector instead
        sel = [torch.ones_like(d[2]) if d[1] is None else (d[1] == d[3]).to(torch.int64) for d in deps]
        return torch.cat([d[0] for d in deps]), torch.cat(sel), torch.cat([d[2] for d in deps]), 1

    def _advance_sum(self, grad_scale: float, cache: dict) -> None:
        """The deposit part of ``advance`` under ``duplicates="sum"``: the named rows are brought to step ``t - 1`` (rows of another
        rank's batch were not read here; the catch-up serves a row named twice once), then one summing step over the whole list."""
        g, node_type, local_idx, type_id = self._merged_deposits(cache)
        n = local_idx.numel()
        if n == 0:
            return
        g = g if g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0 else g.contiguous().clone()
        lib = _lib.load()
        with torch.cuda.device(self.param.device):
            if self.t - 1 > self.flushed:
                _lib.check(lib.egnn_adam_rows_catchup_f32(ctypes.byref(self._desc(self.t - 1)), type_id, _lib.ptr(node_type),
                                                          _lib.ptr(local_idx), n, _lib.stream()), "egnn_adam_rows_catchup_f32")
            ws_bytes = lib.egnn_adam_rows_step_sum_ws_bytes(n, self.param.shape[0])
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.param.device)
            _lib.check(lib.egnn_adam_rows_step_sum_f32(ctypes.byref(self._desc(self.t)), type_id, _lib.ptr(node_type),
                                                       _lib.ptr(local_idx), n, _lib.ptr(g), g.stride(0), float(grad_scale),
                                                       _lib.ptr(ws), ws_bytes, _lib.stream()), "egnn_adam_rows_step_sum_f32")

    def advance(self, sum_duplicates: bool = False, grad_scale: float = 1.0, cache: "dict | None" = None) -> None:
        """One optimiser step: t += 1, this step's ring entries from the group's current lr, the forced flush, then the deposit
        (``LazyRowAdam.step`` has checked that there is at most one) or, with ``sum_duplicates``, all of them in one summing step."""
        self.t += 1
        self.ring.beta1, self.ring.beta2 = (float(b) for b in self.group["betas"])
        self.ring.fill(self.t, self.group["lr"])
        if self.t - self.flushed >= MAX_LAG:
            self._flush_to(self.t - 1)
        if sum_duplicates:
            if self.deposits:
                self._advance_sum(grad_scale, {} if cache is None else cache)
            return
        if self.deposits:
            g, node_type, local_idx, type_id = self.deposits.pop()
            g = g if g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0 else g.contiguous().clone()
            with torch.cuda.device(self.param.device):
                _lib.check(_lib.load().egnn_adam_rows_step_f32(ctypes.byref(self._desc(self.t)), type_id, _lib.ptr(node_type),
                                                               _lib.ptr(local_idx), local_idx.numel(), _lib.ptr(g), g.stride(0),
                                                               _lib.stream()), "egnn_adam_rows_step_f32")


def row_state(t) -> "RowState | None":
    """The row state of a table that a live ``LazyRowAdam`` steps, else None.  A state left behind by an optimiser that no longer exists
    is flushed (the table then holds dense Adam's values) and detached here, so its readers fall back to the dense path."""
    st = getattr(t, "_egnn_rows", None)
    if st is not None and st.owner is not None and st.owner() is None:
        detach(t)
        return None
    return st


def detach(t) -> None:
    """Flush the table's row state, if any, and remove it from the Parameter."""
    st = getattr(t, "_egnn_rows", None)
    if st is not None:
        try:
            st.flush()
        finally:
            st.deposits.clear()
            del t._egnn_rows


class LazyRowAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` whose 2-D fp32 GPU Parameters listed in ``lazy`` are stepped row-lazily (module docstring); every other
    parameter is stepped by an inner ``torch.optim.Adam(..., fused=True)`` with the same options, so with ``lazy=()`` this is that
    optimiser.  ``params`` as for torch.optim.Adam (an iterable or groups).  ``weight_decay = 0`` only, no ``amsgrad`` / ``maximize`` /
    ``capturable`` (NotImplementedError).  ``state_dict()`` flushes first; it and ``load_state_dict()`` use torch Adam's layout (``step``,
    ``exp_avg``, ``exp_avg_sq`` per parameter in ``params`` order): a dense torch.optim.Adam loads it and the other way round.

    ``duplicates="refuse"`` (default): one deposit per table and step, unique rows.  ``duplicates="sum"``: any number of deposits, rows
    named any number of times; a row's gradient is ``grad_scale`` (attribute, or ``step(grad_scale=...)`` for one step; default 1.0)
    times the sum of its gradient rows.  ``grad_scale`` applies to the lazy tables only: the dense gradients of several ``backward()``
    calls accumulate in ``.grad`` as under any optimiser, and scaling them is the caller's job."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, lazy=(), weight_decay=0, amsgrad=False, maximize=False,
                 capturable=False, duplicates="refuse"):
        if duplicates not in ("refuse", "sum"):
            raise ValueError(f"LazyRowAdam: duplicates must be 'refuse' or 'sum', got {duplicates!r}")
        self.duplicates = duplicates
        self.grad_scale = 1.0
        for name, val in (("weight_decay", weight_decay), ("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable)):
            if val:
                raise NotImplementedError(f"LazyRowAdam: {name} is not supported")
        if not 0.0 <= lr or not 0.0 <= eps or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"LazyRowAdam: invalid lr / eps / betas: {lr}, {eps}, {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                                      capturable=False, foreach=None, differentiable=False, fused=None))
        lazy_ids = {id(p) for p in lazy}
        known = {id(p) for g in self.param_groups for p in g["params"]}
        if not lazy_ids <= known:
            raise ValueError("LazyRowAdam: every tensor of `lazy` must also be in `params`")
        self._rows: dict = {}
        inner_groups, idx = [], 0
        for g in self.param_groups:
            for name in ("weight_decay", "amsgrad", "maximize", "capturable"):
                if g.get(name):
                    raise NotImplementedError(f"LazyRowAdam: {name} is not supported")
            rest = []
            for p in g["params"]:
                _lib.require_gpu(p)                  # the inner fused Adam would otherwise step a CPU tensor with torch's own code
                if id(p) in lazy_ids:
                    detach(p)                        # a state of an earlier optimiser: flushed, then replaced
                    st = RowState(p, g, f"#{idx} {tuple(p.shape)}", owner=self)
                    p._egnn_rows = st
                    self._rows[p] = st
                else:
                    rest.append(p)
                idx += 1
            inner_groups.append(rest)
        self._inner_map = inner_groups               # per outer group: the parameters the inner optimiser steps
        self._inner = None
        if any(inner_groups):
            self._inner = torch.optim.Adam([{"params": ps, "lr": g["lr"], "betas": g["betas"], "eps": g["eps"]}
                                            for ps, g in zip(inner_groups, self.param_groups)], fused=True)
        self._built = True

    def add_param_group(self, param_group) -> None:
        if getattr(self, "_built", False):
            raise NotImplementedError("LazyRowAdam: parameter groups are fixed at construction (the lazy tables and the inner "
                                      "optimiser's groups are laid out there); build a new optimiser")
        super().add_param_group(param_group)

    def close(self) -> None:
        """Flush every lazy table and detach its row state from the Parameter: the tables are plain dense Parameters again (values,
        and ``state_dict()`` taken before, are dense Adam's).  This optimiser then steps only its non-lazy parameters."""
        try:
            self.flush()
        finally:
            for p in list(self._rows):
                if getattr(p, "_egnn_rows", None) is self._rows[p]:
                    detach(p)
            self._rows.clear()

    def _sync_inner(self) -> None:
        for ig, g in zip(self._inner.param_groups, self.param_groups):
            ig["lr"], ig["betas"], ig["eps"] = g["lr"], g["betas"], g["eps"]

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.duplicates == "sum":
            scale, cache = float(self.grad_scale if grad_scale is None else grad_scale), {}
            for st in self._rows.values():
                st.advance(True, scale, cache)
            if self._inner is not None:
                self._sync_inner()
                self._inner.step()
            return loss
        if grad_scale is not None:
            raise ValueError("LazyRowAdam: grad_scale needs duplicates='sum'")
        many = [st for st in self._rows.values() if len(st.deposits) > 1]
        if many:                                     # checked for ALL tables before any of them advances: a refused step changes nothing
            msg = ", ".join(f"{st.name}: {len(st.deposits)}" for st in many)
            for st in self._rows.values():
                st.deposits.clear()
            raise RuntimeError(f"LazyRowAdam: more than one gradient deposit for a table in one step ({msg}); one ops.group_input "
                               "backward per table and step")
        for st in self._rows.values():
            st.advance()
        if self._inner is not None:
            self._sync_inner()
            self._inner.step()
        return loss

    @torch.no_grad()
    def flush(self) -> None:
        """Every row of every lazy table up to the current step; raises ``RuntimeError`` (naming the table) if batch rows were refused,
        and if ``ops.group_input`` zero-filled rows whose node type or index was out of range since the last flush (its per-device
        counter is read here, where the refused-row counters are read anyway)."""
        from . import ops
        for st in self._rows.values():
            st.flush()
        for dev in {st.param.device for st in self._rows.values()}:
            bad = ops.group_input_oob(dev)
            if bad:
                raise RuntimeError(f"LazyRowAdam: ops.group_input zero-filled {bad} row(s) on {dev} since the last flush: a node type or "
                                   "an index into a source table was out of range")

    def zero_grad(self, set_to_none: bool = True) -> None:
        super().zero_grad(set_to_none)
        for st in self._rows.values():
            st.deposits.clear()

    def state_dict(self):
        for hook in self._optimizer_state_dict_pre_hooks.values():
            hook(self)
        self.flush()
        groups, state, idx = [], {}, 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(idx, idx + len(g["params"])))
            groups.append(packed)
            for p in g["params"]:
                st = self._rows.get(p)
                if st is not None:
                    if st.t > 0:
                        state[idx] = {"step": torch.tensor(float(st.t)), "exp_avg": st.m, "exp_avg_sq": st.v}
                elif self._inner is not None and len(self._inner.state.get(p, ())) > 0:
                    state[idx] = self._inner.state[p]
                idx += 1
        out = {"state": state, "param_groups": groups}
        for hook in self._optimizer_state_dict_post_hooks.values():
            res = hook(self, out)
            if res is not None:
                out = res
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        state_dict = dict(state_dict)
        for hook in self._optimizer_load_state_dict_pre_hooks.values():
            res = hook(self, state_dict)
            if res is not None:
                state_dict = res
        saved_groups, saved = state_dict["param_groups"], state_dict["state"]
        if len(saved_groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"])
                                                              for a, b in zip(saved_groups, self.param_groups)):
            raise ValueError("LazyRowAdam.load_state_dict: the parameter groups do not match")
        for sg, g in zip(saved_groups, self.param_groups):
            for k in ("lr", "betas", "eps"):
                if k in sg:
                    g[k] = tuple(sg[k]) if k == "betas" else sg[k]
        inner_state, j = {}, 0
        for sg, g in zip(saved_groups, self.param_groups):
            for i, p in zip(sg["params"], g["params"]):
                s = saved.get(i, saved.get(str(i)))
                st = self._rows.get(p)
                if st is None:
                    if s is not None:
                        inner_state[j] = s
                    j += 1
                    continue
                st.deposits.clear()                  # everything the table held is replaced: no flush, pending counts dropped
                st.dup.zero_()
                st.ring = AdamRing(*g["betas"])
                if s is None:
                    st.m.zero_(), st.v.zero_(), st.last.fill_(-1)
                    st.t = st.flushed = 0
                else:
                    st.m.copy_(s["exp_avg"]), st.v.copy_(s["exp_avg_sq"])
                    st.t = st.flushed = int(float(s["step"]))
                    st.last.fill_(st.t)
        if self._inner is not None:
            self._sync_inner()
            self._inner.load_state_dict({"state": inner_state, "param_groups": self._inner.state_dict()["param_groups"]})
        for hook in self._optimizer_load_state_dict_post_hooks.values():
            hook(self)
