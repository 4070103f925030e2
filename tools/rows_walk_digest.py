#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of the kernels that walk the sorted (row, position) keys (csrc/rows_runs.h: the plan build, the
run-sum, scatter max / min / mean / sum with its backward, the segment softmax in both directions, the summing Adam step) over a fixed
set of small cases, for comparing two builds of libegnn_hip.so bit for bit: a refactor of the run cut must leave every digest as it
was.  Inputs and indices come from ``numpy.random.RandomState``; the entry points are called over the C ABI, so a library from another
commit (``--lib``) serves as long as its ABI version matches.  With K = EGNN_ROWS_SUM_CHUNK read from include/egnn_hip.h:

  index lists (shuffled, n_rows = 37)   S in {0, 1, K-1, K, K+1, 2K, 2K+1} naming one row (a run that ends on a chunk edge, and one past it)
                                        a hub of 3K+5 among singletons; unique ids
                                        two long runs, K+2 and 2K+44, neighbours from sorted position 0 (the second head at offset 2 of
                                        the second window, where the first run's tail ends: one head and one later chunk start per window)
                                        a long run whose head is the last position of a window
                                        ids outside [-n, n) and negative ids (a NO_KEY tail, as a deferred plan produces)
  n_rows = 300                          the hub and the out-of-range list again (rows that no key names, over more than one workgroup)
  layouts                               contiguous; a pitch padded to the next multiple of 4 above C; a base 4 bytes past a 16-byte boundary
  columns                               1, 3, 4, 40, 260 (run-sum, scatter); 1, 3, 4, 8 (softmax); the Adam step: D = 8, a row named 3 times

A case is (entry point, index list, layout); its digest runs over the column counts in ascending order.  Whole buffers are hashed,
pad columns included (filled before the call), so a stray store changes a digest too.  Prints one JSON line {case: sha256}.  Each
call takes milliseconds.

  python tools/rows_walk_digest.py [--lib PATH/libegnn_hip.so]
"""
import argparse
import ctypes
import hashlib
import json
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS, SOFTMAX_COLS = (1, 3, 4, 40, 260), (1, 3, 4, 8)
LAYOUTS = ("contiguous", "padded", "offset")
REDUCE = ("sum", "mean", "max", "min")
FILL = 7.0


def chunk():
    text = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return int(re.search(r"#define\s+EGNN_ROWS_SUM_CHUNK\s+(\d+)", text).group(1))


def index_lists(K):
    """name -> (ids, n_rows); every list is shuffled with a fixed seed"""
    n = 37
    lists = {f"one_row/S={S}": ([5] * S, n) for S in (0, 1, K - 1, K, K + 1, 2 * K, 2 * K + 1)}
    singles = [r for r in range(n) if r != 7]
    lists["hub"] = ([7] * (3 * K + 5) + singles, n)
    lists["unique"] = (list(range(0, n, 2)) + list(range(1, n, 4)), n)
    lists["two_long"] = ([0] * (K + 2) + [1] * (2 * K + 44) + [9, 20, 36], n)
    lists["head_ends_window"] = ([0] * (K // 2) + [1] * (K - 1 - K // 2) + [2] * (K + 9) + [30, 31], n)
    lists["out_of_range"] = ([3, -1, -n, n, -n - 1, 2 * n, 12, 12, -5, 1 << 40, -(1 << 40), 0] * 3 + [3] * (K + 1), n)
    lists["hub/n_rows=300"] = (lists["hub"][0], 300)
    lists["out_of_range/n_rows=300"] = ([3, -1, -300, 300, -301, 600, 12, 12, -5, 1 << 40, 299, 0] * 3 + [3] * (K + 1), 300)
    out = {}
    for k, (name, (ids, rows)) in enumerate(lists.items()):
        ids = np.asarray(ids, dtype=np.int64)
        np.random.RandomState(100 + k).shuffle(ids)
        out[name] = (ids, rows)
    return out


def main(args):
    import torch

    sys.path.insert(0, ROOT)
    from efficient_gnns_amd import _lib

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load()
    assert torch.cuda.is_available(), "rows_walk_digest needs a GPU"
    dev = torch.device("cuda", 0)
    K = chunk()
    rs = np.random.RandomState(20241)
    digests = {}

    def pitch_of(C, layout):
        return C if layout != "padded" else (C // 4 + 1) * 4

    def view(n, C, layout, values=None):
        """(whole buffer, its [n, C] view) under one of the three layouts; the view holds ``values`` or, like the pad, FILL"""
        pitch, lead = pitch_of(C, layout), 1 if layout == "offset" else 0
        buf = torch.full((n * pitch + 4,), FILL, dtype=torch.float32, device=dev)
        v = buf[lead:lead + n * pitch].view(n, pitch)[:, :C]
        assert buf.data_ptr() % 16 == 0 and (n == 0 or v.data_ptr() % 16 == 4 * lead)
        if values is not None:
            v.copy_(torch.from_numpy(values).to(dev))
        return buf, v

    def randn(n, C):
        return rs.standard_normal((n, C)).astype(np.float32)

    def workspace(nbytes):
        return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)

    def add(case, *tensors):
        """the bytes of ``tensors`` join the digest of ``case`` (a case runs over its column counts in ascending order)"""
        torch.cuda.synchronize()
        h = digests.setdefault(case, hashlib.sha256())
        for t in tensors:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())

    def plan(ids, n_rows):
        S = int(ids.shape[0])
        idx = torch.from_numpy(ids).to(dev)
        keys = torch.zeros(max(S, 1), dtype=torch.int64, device=dev)
        wrapped = torch.zeros(max(S, 1), dtype=torch.int64, device=dev)
        counters = torch.zeros(4, dtype=torch.int32, device=dev)
        nws = lib.egnn_rows_plan_ws_bytes(S, n_rows)
        ws = workspace(nws)
        _lib.check(lib.egnn_rows_plan_build_i64(_lib.ptr(idx), S, n_rows, _lib.ptr(keys), _lib.ptr(counters), _lib.ptr(ws), nws, _lib.stream()),
                   "egnn_rows_plan_build_i64")
        _lib.check(lib.egnn_rows_wrap_i64(_lib.ptr(idx), S, n_rows, _lib.ptr(wrapped), _lib.stream()), "egnn_rows_wrap_i64")
        return S, max(1, (S - 1).bit_length()), keys, wrapped, counters

    for name, (ids, n_rows) in index_lists(K).items():
        S, shift, keys, wrapped, counters = plan(ids, n_rows)
        add(f"plan/{name}", keys[:S], counters, wrapped[:S])
        for layout in LAYOUTS:
            for C in COLS:
                tag = f"{name}/{layout}"
                p = pitch_of(C, layout)
                _, src = view(S, C, layout, randn(S, C))
                nws = lib.egnn_rows_add_runs_ws_bytes(S, C)
                ws = workspace(nws)
                for acc in (0, 1):
                    dbuf, dst = view(n_rows, C, layout, randn(n_rows, C) if acc else None)
                    _lib.check(lib.egnn_rows_add_runs_f32(_lib.ptr(dst), p, n_rows, _lib.ptr(keys), S, shift, _lib.ptr(src), p, C, acc,
                                                          _lib.ptr(ws), nws, _lib.stream()), "egnn_rows_add_runs_f32")
                    add(f"add_runs/acc={acc}/{tag}", dbuf)
                _, g = view(n_rows, C, layout, randn(n_rows, C))
                for red, rname in enumerate(REDUCE):
                    obuf, out = view(n_rows, C, layout)
                    count = torch.full((n_rows,), -3, dtype=torch.int32, device=dev)
                    arg = torch.full((n_rows, C), -3, dtype=torch.int64, device=dev) if red >= 2 else None
                    nws = lib.egnn_scatter_runs_ws_bytes(S, C, red)
                    ws = workspace(nws)
                    _lib.check(lib.egnn_scatter_runs_f32(_lib.ptr(out), p, n_rows, _lib.ptr(count), _lib.ptr(arg), _lib.ptr(keys), S, shift,
                                                         _lib.ptr(src), p, C, red, _lib.ptr(ws), nws, _lib.stream()), "egnn_scatter_runs_f32")
                    add(f"scatter_{rname}/{tag}", obuf, count, *([arg] if arg is not None else []))
                    dsbuf, dsrc = view(S, C, layout)
                    _lib.check(lib.egnn_scatter_bwd_f32(_lib.ptr(dsrc), p, S, _lib.ptr(wrapped), n_rows, _lib.ptr(g), p, C, red, _lib.ptr(count),
                                                        _lib.ptr(arg), _lib.stream()), "egnn_scatter_bwd_f32")
                    add(f"scatter_bwd_{rname}/{tag}", dsbuf)
            for C in SOFTMAX_COLS:
                tag = f"{name}/{layout}"
                p = pitch_of(C, layout)
                _, src = view(S, C, layout, 3.0 * randn(S, C))
                _, g = view(S, C, layout, randn(S, C))
                nws = lib.egnn_scatter_softmax_ws_bytes(S, C)
                ws = workspace(nws)
                for form, fname in enumerate(("softmax", "log_softmax")):
                    for eps in (0.0, 1e-16):
                        obuf, out = view(S, C, layout)
                        row_max, row_den = (torch.full((n_rows, C), FILL, dtype=torch.float32, device=dev) for _ in range(2))
                        _lib.check(lib.egnn_scatter_softmax_fwd_f32(_lib.ptr(out), p, _lib.ptr(row_max), _lib.ptr(row_den), n_rows, _lib.ptr(keys),
                                                                    S, shift, _lib.ptr(wrapped), _lib.ptr(src), p, C, eps, form, _lib.ptr(ws), nws,
                                                                    _lib.stream()), "egnn_scatter_softmax_fwd_f32")
                        add(f"{fname}_fwd/eps={eps:g}/{tag}", obuf, row_max, row_den)
                    dsbuf, dsrc = view(S, C, layout)                 # the backward takes the eps = 1e-16 output
                    row_dot = torch.full((n_rows, C), FILL, dtype=torch.float32, device=dev)
                    _lib.check(lib.egnn_scatter_softmax_bwd_f32(_lib.ptr(dsrc), p, _lib.ptr(row_dot), n_rows, _lib.ptr(keys), S, shift,
                                                                _lib.ptr(wrapped), _lib.ptr(out), p, _lib.ptr(g), p, C, form, _lib.ptr(ws), nws,
                                                                _lib.stream()), "egnn_scatter_softmax_bwd_f32")
                    add(f"{fname}_bwd/{tag}", dsbuf, row_dot)

    # the summing Adam step: 16 rows of D = 8, seven entries, row 3 named three times, one entry outside the table
    n_rows, D, lr, b1, b2 = 16, 8, 0.01, 0.9, 0.999
    pt, mt = (torch.from_numpy(randn(n_rows, D)).to(dev) for _ in range(2))
    vt = torch.from_numpy(randn(n_rows, D) ** 2).to(dev)
    last = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    last[::5] = -1                                                   # rows that never had a gradient: m = v = 0
    mt[::5] = 0
    vt[::5] = 0
    dup = torch.zeros(1, dtype=torch.int32, device=dev)
    local = torch.tensor([3, 9, 3, 16, 0, 3, 11], dtype=torch.int64, device=dev)
    g = torch.from_numpy(randn(7, D)).to(dev)
    d = _lib.AdamRows()
    d.p, d.m, d.v, d.last, d.dup_count = (t.data_ptr() for t in (pt, mt, vt, last, dup))
    d.n_rows, d.D, d.ld = n_rows, D, D
    d.beta1, d.beta2, d.eps, d.one_minus_beta1, d.one_minus_beta2 = b1, b2, 1e-8, 1.0 - b1, 1.0 - b2
    d.step, d.flushed = 1, 0
    d.step_size[1], d.bc2_sqrt[1] = lr / (1.0 - b1), math.sqrt(1.0 - b2)
    nws = lib.egnn_adam_rows_step_sum_ws_bytes(7, n_rows)
    ws = workspace(nws)
    _lib.check(lib.egnn_adam_rows_step_sum_f32(ctypes.byref(d), 0, None, _lib.ptr(local), 7, _lib.ptr(g), D, 0.5, _lib.ptr(ws), nws,
                                               _lib.stream()), "egnn_adam_rows_step_sum_f32")
    add("adam_rows_step_sum/D=8", pt, mt, vt, last, dup)
    print(json.dumps({k: h.hexdigest() for k, h in digests.items()}, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    sys.exit(main(ap.parse_args()))
