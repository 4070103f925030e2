#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of the kernels that reduce through csrc/block_reduce.h (the loss and metric kernels, the segment
kernels, the column sum, the GAT and SIGN backward finalizes) over a fixed set of small cases, for comparing two builds of
libegnn_hip.so bit for bit: a refactor of the reduction helpers must leave every digest as it was.  Inputs come from
``numpy.random.RandomState``; the entry points are called over the C ABI (the GAT layer and the SIGN PReLU backward through their
autograd functions, which build the descriptor structs), so a library from another commit (``--lib``) serves as long as its ABI
version matches.

  fitnet, AT energy / forward, CE/KD   n in {1, 4, 5, 4*1024, 4*1024+1}: one partial, one row more than a workgroup, the grid cap and
                                       the first row count past it.  CE/KD: C in {3, 40, 64, 65} (16-lane path to its limit, 64-lane
                                       path), with / without teacher and row list, one label outside [0, C)
  AT finish / partial                  n in {1, 1023, 1024, 1025, 5000}
  NCE forward, block forward           S in {1, 255, 256, 257, 1000}; block form: 130 more columns (two or more column splits), both
                                       forms of the saved scores
  BCE pair                             total in {1, 255, 256, 257, 256*1024+3}
  LSP forward / backward, segment      pointers with an empty segment, segments of 1, 16, 17, 256 and 257 entries; n_seg in
  softmax, segment sum                 {1, 15, 16, 17} and one past 16*1024 (the cap binds); both terms, with / without teacher gradient
  column sum                           C in {1, 3, 4, 250, 256, 260} x n in {1, 5, 1025}, C = 1 also n = 256*1024+1, padded pitch
  GAT layer backward                   9 nodes, a self-loop-only row and a hub, H x C in {1x5, 2x8}, concatenated and averaged heads
  SIGN prelu_drop backward             H in {1, 3}, Cs in {4, 9}, B in {1, 2500}
  split accuracy / counts              n in {1, 15, 16, 17, 16*1024+1}; a NaN row, a tie, an empty split

Whole buffers are hashed, workspaces (prefilled) and pad columns included, so a stray store changes a digest too.  Prints one JSON
line {case: sha256}.  Each call takes milliseconds.

  python tools/reduce_digest.py [--lib PATH/libegnn_hip.so]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.0
ROW_NS = (1, 4, 5, 4 * 1024, 4 * 1024 + 1)


def seg_ptr(rs, n_seg):
    """segment lengths cycling through (0, 1, 16, 17, 256, 257, 3) from a seed-dependent start"""
    lens = np.array((0, 1, 16, 17, 256, 257, 3))[(np.arange(n_seg) + rs.randint(7)) % 7]
    if n_seg > 64:
        lens = np.where(np.arange(n_seg) % 97 == 0, lens, lens % 5)     # a few long segments among short ones
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def main(args):
    import torch

    sys.path.insert(0, ROOT)
    from efficient_gnns_amd import _lib, ops, ops_edge
    from efficient_gnns_amd.sparse import SparseTensor

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load()
    assert torch.cuda.is_available(), "reduce_digest needs a GPU"
    dev = torch.device("cuda", 0)
    P, st = _lib.ptr, _lib.stream
    digests = {}

    def dv(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def normal(rs, *shape):
        return rs.standard_normal(shape).astype(np.float32)

    def filled(*shape, dtype=torch.float32):
        return torch.full(shape, FILL, dtype=dtype, device=dev)

    def padded(x):
        """[n, C] values in a buffer whose pitch is the next multiple of 4 above C + 1, pad columns prefilled"""
        n, C = x.shape
        buf = filled(n, (C + 4) // 4 * 4 + 4)
        buf[:, :C] = dv(x)
        return buf, buf[:, :C]

    def sha(*tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()

    def call(name, *a):
        _lib.check(getattr(lib, name)(*a), name)

    # ---- fitnet, attention transfer
    rs = np.random.RandomState(31415)
    for n in ROW_NS:
        D, Dt = 70, 33
        _, f = padded(normal(rs, n, D))
        _, t = padded(normal(rs, n, D))
        _, t2 = padded(normal(rs, n, Dt))
        nws = lib.egnn_feature_loss_ws_floats(n)
        loss, ws = filled(1), filled(nws)
        call("egnn_fitnet_fwd_f32", P(f), f.stride(0), P(t), t.stride(0), n, D, 1e-12, P(loss), P(ws), nws, st())
        digests[f"fitnet_fwd/n={n}"] = sha(loss, ws)
        loss, ws = filled(1), filled(nws)
        call("egnn_at_fwd_f32", P(f), f.stride(0), D, P(t2), t2.stride(0), Dt, n, 1e-12, P(loss), P(ws), nws, st())
        digests[f"at_fwd/n={n}"] = sha(loss, ws)
        es, et, sumsq, ws = filled(n), filled(n), filled(2), filled(nws)
        call("egnn_at_energy_f32", P(f), f.stride(0), D, P(t2), t2.stride(0), Dt, n, P(es), P(et), P(sumsq), P(ws), nws, st())
        digests[f"at_energy/n={n}"] = sha(es, et, sumsq, ws)
    for n in (1, 1023, 1024, 1025, 5000):
        f, t = dv(normal(rs, n, 3)), dv(normal(rs, n, 2))
        nws = lib.egnn_feature_loss_ws_floats(n)
        loss, ws = filled(1), filled(nws)
        call("egnn_at_fwd_f32", P(f), 3, 3, P(t), 2, 2, n, 1e-12, P(loss), P(ws), nws, st())
        digests[f"at_finish/n={n}"] = sha(loss, ws)
        es, et = dv(np.abs(normal(rs, n))), dv(np.abs(normal(rs, n)))
        sumsq = torch.stack([(es * es).sum(), (et * et).sum()]).contiguous()
        scal, sums, ws = filled(4), filled(3), filled(nws)
        call("egnn_at_partial_f32", P(es), P(et), n, P(sumsq), 1e-12, P(scal), P(sums), P(ws), nws, st())
        digests[f"at_partial/n={n}"] = sha(scal, sums, ws)

    # ---- cross entropy + logit KD
    rs = np.random.RandomState(27182)
    for n in ROW_NS:
        for C in (3, 40, 64, 65):
            n_all = n + 3
            buf_l, logits = padded(normal(rs, n_all, C) * 3)
            buf_t, teacher = padded(normal(rs, n_all, C) * 3)
            labels_h = rs.randint(0, C, n_all).astype(np.int64)
            labels_h[rs.randint(n_all)] = C + 2                       # one label outside [0, C): ignored
            labels_h[0] = -100 if n > 1 else labels_h[0]
            labels = dv(labels_h)
            rows = dv(rs.permutation(n_all)[:n].astype(np.int64))
            for with_t in (False, True):
                for with_rows in (False, True):
                    out3, ws = filled(3), filled(lib.egnn_ce_kd_ws_floats(n))
                    call("egnn_ce_kd_fwd_f32", P(logits), logits.stride(0), P(teacher) if with_t else None, teacher.stride(0) if with_t else 0,
                         P(labels), P(rows) if with_rows else None, n, C, 2.0, P(out3), P(ws), st())
                    digests[f"ce_kd_fwd/n={n}/C={C}/teacher={int(with_t)}/rows={int(with_rows)}"] = sha(out3, ws)

    # ---- NCE forward
    rs = np.random.RandomState(16180)

    def unit(n, d):
        x = normal(rs, n, d)
        return dv(x / np.sqrt((x * x).sum(1, keepdims=True)))

    for S in (1, 255, 256, 257, 1000):
        Pd = 32
        fh, th = unit(S, Pd), unit(S, Pd)
        nws = lib.egnn_nce_ws_floats(S)
        for unit_rows in (1, 0):
            Z, lse, loss, ws = filled(S, S), filled(S), filled(1), filled(nws)
            call("egnn_nce_fwd_f32", P(fh), P(th), S, Pd, Pd, 0.075, unit_rows, P(Z), P(lse), P(loss), P(ws), nws, st())
            digests[f"nce_fwd/S={S}/unit_rows={unit_rows}"] = sha(Z, lse, loss, ws)
            Sc = S + 130
            ta = unit(Sc, Pd)
            Z, lse, loss, ws = filled(S, Sc), filled(S), filled(1), filled(nws)
            call("egnn_nce_block_fwd_f32", P(fh), Pd, P(ta), Pd, S, Sc, 65, Pd, 0.075, 1.0 / Sc, unit_rows, P(Z), P(lse), P(loss), P(ws),
                 nws, st())
            digests[f"nce_block_fwd/Sr={S}/Sc={Sc}/unit_rows={unit_rows}"] = sha(Z, lse, loss, ws)

    # ---- BCE pair
    rs = np.random.RandomState(14142)
    for total in (1, 255, 256, 257, 256 * 1024 + 3):
        x, t = dv(normal(rs, total) * 2), dv(normal(rs, total) * 2)
        y = dv((rs.rand(total) < 0.3).astype(np.float32))
        out2, ws = filled(2), filled(lib.egnn_bce_pair_ws_floats())
        call("egnn_bce_pair_fwd_f32", P(x), P(y), P(t), total, P(out2), P(ws), st())
        digests[f"bce_pair_fwd/total={total}"] = sha(out2, ws)

    # ---- LSP, segment softmax, segment sum
    rs = np.random.RandomState(17320)
    for n_seg in (1, 6, 7, 15, 16, 17, 16 * 1024 + 5):
        ptr_h = seg_ptr(rs, n_seg)
        E = max(int(ptr_h[-1]), 1)
        ptr = dv(ptr_h)
        xs, xt, gp = dv(normal(rs, E)), dv(normal(rs, E)), dv(normal(rs, E))
        p, gx, out = filled(E), filled(E), filled(n_seg)
        call("egnn_segment_softmax_fwd_f32", P(ptr), P(xs), n_seg, P(p), st())
        call("egnn_segment_softmax_bwd_f32", P(ptr), P(p), P(gp), n_seg, P(gx), st())
        call("egnn_segment_sum_f32", P(ptr), P(xs), n_seg, P(out), st())
        digests[f"segment_softmax/n_seg={n_seg}"] = sha(p, gx)
        digests[f"segment_sum/n_seg={n_seg}"] = sha(out)
        g = dv(np.array([0.7], dtype=np.float32))
        for crit in (0, 1):
            ps, pt, loss, ws = filled(E), filled(E), filled(1), filled(lib.egnn_lsp_loss_ws_floats())
            call("egnn_lsp_loss_fwd_f32", P(ptr), P(xs), P(xt), n_seg, E, crit, P(ps), P(pt), P(loss), P(ws), st())
            digests[f"lsp_fwd/n_seg={n_seg}/criterion={crit}"] = sha(ps, pt, loss, ws)
            for with_t in (False, True):
                gs, gt = filled(E), filled(E)
                call("egnn_lsp_loss_bwd_f32", P(ptr), P(ps), P(pt), n_seg, E, crit, P(g), P(gs), P(gt) if with_t else None, st())
                digests[f"lsp_bwd/n_seg={n_seg}/criterion={crit}/teacher_grad={int(with_t)}"] = sha(gs, gt)

    # ---- column sums
    rs = np.random.RandomState(22360)
    for C in (1, 3, 4, 250, 256, 260):
        for n in (1, 5, 1025) + ((256 * 1024 + 1,) if C == 1 else ()):
            buf, x = padded(normal(rs, n, C))
            out, ws = filled(C), filled(lib.egnn_colsum_ws_floats(C))
            call("egnn_colsum_f32", P(x), x.stride(0), n, C, P(out), P(ws), st())
            digests[f"colsum/C={C}/n={n}"] = sha(out, ws, buf)

    # ---- GAT layer backward (the d_att partial finalize): node 0 has only its self loop, node 4 is a hub
    rs = np.random.RandomState(26457)
    n = 9
    dst = [0] + [4] * 8 + [1, 2, 3, 5, 6, 7, 8, 8]
    src = [0] + [0, 1, 2, 3, 5, 6, 7, 8] + [4, 1, 4, 5, 5, 6, 8, 2]
    adj = SparseTensor(row=dv(np.array(dst, dtype=np.int64)), col=dv(np.array(src, dtype=np.int64)), sparse_sizes=(n, n))
    for H, C in ((1, 5), (2, 8)):
        for concat in (True, False):
            xl = dv(normal(rs, n, H * C)).requires_grad_()
            al, ar = dv(normal(rs, 1, H, C)).requires_grad_(), dv(normal(rs, 1, H, C)).requires_grad_()
            out = ops_edge.gat_attention(xl, al, ar, adj, H, concat, 0.2)
            out.backward(dv(normal(rs, *out.shape)))
            digests[f"gat_layer_bwd/H={H}/C={C}/mean_heads={int(not concat)}"] = sha(out, xl.grad, al.grad, ar.grad)

    # ---- SIGN prelu_drop backward (the PReLU slope gradients)
    rs = np.random.RandomState(28284)
    for H in (1, 3):
        for Cs in (4, 9):
            for B in (1, 2500):
                z = dv(normal(rs, B, H * Cs)).requires_grad_()
                slopes = [dv(np.array([0.25 + 0.1 * h], dtype=np.float32)).requires_grad_() for h in range(H)]
                y = ops.prelu_drop(z, slopes, Cs, 0.0, False)
                y.backward(dv(normal(rs, B, H * Cs)))
                digests[f"prelu_drop_bwd/H={H}/Cs={Cs}/B={B}"] = sha(y, z.grad, *[a.grad for a in slopes])

    # ---- split accuracy and counts
    rs = np.random.RandomState(30000)
    for n in (1, 15, 16, 17, 16 * 1024 + 1):
        C = 7
        lg = normal(rs, n, C)
        lg[0, 2] = np.nan                                              # a NaN counts as the maximum
        if n > 1:
            lg[1, 3] = lg[1, 5] = 9.0                                  # a tie: the first maximal column wins
        _, logits = padded(lg)
        y = dv(rs.randint(0, C, n).astype(np.int64))
        sid = dv(np.where(np.arange(n) % 3 == 0, 0, 2).astype(np.int8))  # split 1 (valid) is empty
        nws = lib.egnn_split_accuracy_ws_ints()
        acc3, out6 = filled(3, dtype=torch.float64), filled(6, dtype=torch.float64)
        ws = torch.full((nws,), 7, dtype=torch.int32, device=dev)
        call("egnn_split_accuracy_f32", P(logits), logits.stride(0), n, C, P(y), P(sid), P(acc3), P(ws), nws, st())
        ws2 = torch.full((nws,), 7, dtype=torch.int32, device=dev)
        call("egnn_split_counts_f32", P(logits), logits.stride(0), n, C, P(y), P(sid), P(out6), P(ws2), nws, st())
        digests[f"split_accuracy/n={n}"] = sha(acc3, ws)
        digests[f"split_counts/n={n}"] = sha(out6, ws2)

    print(json.dumps(digests, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libegnn_hip.so (same ABI version) instead of the in-tree one")
    sys.exit(main(ap.parse_args()))
