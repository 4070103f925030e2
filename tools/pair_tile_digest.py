#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of the all-pairs kernels (csrc/pair_tile.h: GSP forward, pair moments, distance median, RBF CKA)
over a fixed set of small cases, for comparing two builds of libegnn_hip.so bit for bit: a refactor of these kernels must leave
every digest as it was.  Inputs come from ``numpy.random.RandomState`` (the same bytes whatever torch version generates elsewhere);
the entry points are called over the C ABI, so a library from another commit (``--lib``) serves as long as its ABI version matches.

  N in {2, 3, 127, 128, 129, 257, 641}   one row, the tile edge from both sides, a ragged second tile, several tiles of the triangle
  layouts                                 vec4:   256 / 750 columns behind ``ops.pad_pitch`` (float4 operand loads)
                                          scalar: 5 / 7 columns, contiguous (pitch not a multiple of 4)
                                          offset: the vec4 buffers entered one float late (pitch a multiple of 4, base not 16-byte aligned)
  GSP                                     S in {129, 600}, P in {128, 5} and the offset view of P = 128, kernels cosine / poly / l2 / rbf

Prints one JSON line {case: sha256}.  Each case takes milliseconds.

  python tools/pair_tile_digest.py [--lib PATH/libegnn_hip.so]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (2, 3, 127, 128, 129, 257, 641)
GSP_S = (129, 600)
GSP_KERNELS = ("cosine", "poly", "l2", "rbf")


def unit_rows(rs, n, d):
    x = np.maximum(rs.standard_normal((n, d)), 0.0).astype(np.float32) + np.float32(0.05)
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32))


def main(args):
    import torch

    sys.path.insert(0, ROOT)
    from efficient_gnns_amd import _lib, ops

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load()
    assert torch.cuda.is_available(), "pair_tile_digest needs a GPU"
    dev = torch.device("cuda", 0)

    def place(x, layout):
        """The [n, C] values of the host array ``x`` on the device under one of the three layouts."""
        t = torch.from_numpy(x).to(dev)
        if layout == "scalar":
            return t.contiguous()
        t = ops.pad_pitch(t)
        if layout == "vec4":
            assert t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
            return t
        n, C, pitch = t.shape[0], t.shape[1], t.stride(0)
        buf = torch.zeros(n * pitch + 4, dtype=torch.float32, device=dev)
        v = buf[1:1 + n * pitch].view(n, pitch)[:, :C]
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    def sha(*tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()

    def f64(n):
        return torch.zeros(n, dtype=torch.float64, device=dev)

    def args2(xs, xt):
        return (_lib.ptr(xs), xs.stride(0), xs.shape[1], _lib.ptr(xt), xt.stride(0), xt.shape[1])

    def moments(xs, xt, N):
        out, nws = f64(6), lib.egnn_pair_moments_ws_bytes(N)
        ws = f64(nws // 8)
        _lib.check(lib.egnn_pair_moments_f32(*args2(xs, xt), N, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream()), "egnn_pair_moments_f32")
        return out

    def median(x, N):
        out, nws = f64(2), lib.egnn_sqdist_median_ws_bytes(N)
        ws = f64(nws // 8)
        _lib.check(lib.egnn_sqdist_median_f32(_lib.ptr(x), x.stride(0), x.shape[1], N, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream()),
                   "egnn_sqdist_median_f32")
        return out

    def rbf_cka(xs, xt, N, sigma2):
        out, nws = f64(3), lib.egnn_rbf_cka_ws_bytes(N)
        ws = f64(nws // 8)
        _lib.check(lib.egnn_rbf_cka_f32(*args2(xs, xt), N, _lib.ptr(sigma2), _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream()),
                   "egnn_rbf_cka_f32")
        return out

    def gsp(xs, xt, S, kernel):
        Ws, Wt = (torch.zeros(S, S, dtype=torch.float32, device=dev) for _ in range(2))
        loss, nws = torch.zeros(1, dtype=torch.float32, device=dev), lib.egnn_gsp_ws_floats(S)
        ws = torch.zeros(nws, dtype=torch.float32, device=dev)
        _lib.check(lib.egnn_gsp_fwd_f32(*args2(xs, xt), S, GSP_KERNELS.index(kernel), _lib.ptr(Ws), _lib.ptr(Wt), _lib.ptr(loss),
                                        _lib.ptr(ws), nws, _lib.stream()), "egnn_gsp_fwd_f32")
        return loss, Ws, Wt

    digests = {}
    rs = np.random.RandomState(20240)
    for N in NS:
        for layout in ("vec4", "scalar", "offset"):
            Ds, Dt = (5, 7) if layout == "scalar" else (256, 750)
            xs, xt = place(unit_rows(rs, N, Ds), layout), place(unit_rows(rs, N, Dt), layout)
            key = f"N={N}/{layout}"
            digests[f"pair_moments/{key}"] = sha(moments(xs, xt, N))
            med = torch.stack([median(xs, N), median(xt, N)])
            digests[f"sqdist_median/{key}"] = sha(med)
            digests[f"rbf_cka_own_sigma/{key}"] = sha(rbf_cka(xs, xt, N, med[:, 0].contiguous()))
            given = torch.tensor([0.75 ** 2, 1.25 ** 2], dtype=torch.float64, device=dev)
            digests[f"rbf_cka_given_sigma/{key}"] = sha(rbf_cka(xs, xt, N, given))
    for S in GSP_S:
        for P, layout in ((128, "vec4"), (5, "scalar"), (128, "offset")):
            xs, xt = place(unit_rows(rs, S, P), layout), place(unit_rows(rs, S, P), layout)
            for kernel in GSP_KERNELS:
                digests[f"gsp_{kernel}/S={S}/P={P}/{layout}"] = sha(*gsp(xs, xt, S, kernel))
    print(json.dumps(digests, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    sys.exit(main(ap.parse_args()))
