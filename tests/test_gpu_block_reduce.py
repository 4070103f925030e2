"""The fixed-order reduction of csrc/block_reduce.h on the device (run with ``-m gpu``), exactly: every input is a multiple of 0.25
with |x| <= 4, so every partial sum is an integer multiple of 0.25 below 2^24 quarters and exact in fp32 WHATEVER the order -- the result
must equal the float64 sum bit for bit, and a partial that is dropped or counted twice (at a grid cap, at a ragged last workgroup)
cannot hide inside a tolerance.  Shapes sit on the edges of the launch geometry: one partial, one item more than a workgroup's
worth, the grid cap and the first size past it."""
import numpy as np
import pytest
import torch

import efficient_gnns_amd.ops as ops
from efficient_gnns_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def quarters(rs, *shape):
    return (rs.randint(-16, 17, size=shape) * 0.25).astype(np.float32)


# C: one column (256 rows per workgroup: the cap of 1024 workgroups binds only past 256 * 1024 rows), below / at / above a column
# group of 4, the widest single chunk and its neighbours; n: one row, fewer rows than row lanes, more than one workgroup
@pytest.mark.parametrize("n,C", [(1, 1), (5, 3), (1025, 4), (1025, 250), (5, 256), (1025, 260), (256 * 1024 + 1, 1)])
def test_colsum_is_the_exact_sum(n, C):
    rs = np.random.RandomState(1000 * C + n % 1000)
    x_h = quarters(rs, n, C)
    buf = torch.full((n, C + 5), 7.0, device=DEV)                      # a padded pitch; the pad columns must not enter any sum
    x = buf[:, :C]
    x.copy_(torch.from_numpy(x_h))
    lib = _lib.load()
    out = torch.full((C,), 7.0, device=DEV)
    ws = torch.full((lib.egnn_colsum_ws_floats(C),), 7.0, device=DEV)
    _lib.check(lib.egnn_colsum_f32(_lib.ptr(x), x.stride(0), n, C, _lib.ptr(out), _lib.ptr(ws), _lib.stream()), "egnn_colsum_f32")
    assert np.array_equal(out.cpu().numpy().astype(np.float64), x_h.astype(np.float64).sum(0))
    assert torch.equal(ops.colsum(x), out)


# segment lengths around the 16-lane group (0, 1, 16, 17) and the 256-entry limit past which the whole wave walks (256, 257);
# n_seg: one segment, one workgroup pass of 16 from both sides, and more than the 16 * 16384 the capped grid covers in one pass
@pytest.mark.parametrize("n_seg", [1, 15, 16, 17, 16 * 16384 + 5])
def test_segment_sum_is_the_exact_sum(n_seg):
    rs = np.random.RandomState(n_seg)
    lens = np.array((257, 0, 1, 16, 17, 256, 3))[np.arange(n_seg) % 7]
    if n_seg > 64:
        lens = np.where(np.arange(n_seg) % 4099 == 0, lens, lens % 5)  # a few long segments among short ones
    ptr_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x_h = quarters(rs, int(ptr_h[-1]))
    ptr, x = torch.from_numpy(ptr_h).to(DEV), torch.from_numpy(x_h).to(DEV)
    out = torch.full((n_seg,), 7.0, device=DEV)
    _lib.check(_lib.load().egnn_segment_sum_f32(_lib.ptr(ptr), _lib.ptr(x), n_seg, _lib.ptr(out), _lib.stream()), "egnn_segment_sum_f32")
    want = np.add.reduceat(np.concatenate([x_h.astype(np.float64), [0.0]]), ptr_h[:-1]) * (lens > 0)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want)


# 16 rows per workgroup pass and at most 1024 workgroups: one row, the pass from both sides, the first row count past the cap
@pytest.mark.parametrize("n", [1, 15, 16, 17, 16 * 1024 + 1])
def test_split_counts_are_the_exact_counts(n):
    rs = np.random.RandomState(n)
    C = 7
    lg = quarters(rs, n, C)
    lg[0, 2] = np.nan                                                  # NaN counts as the maximum, like torch.argmax
    if n > 1:
        lg[1, :] = 0.0
        lg[1, 3] = lg[1, 5] = 4.0                                      # a tie: the first maximal column wins
    y = rs.randint(0, C, n).astype(np.int64)
    y[0] = 2
    sid = np.where(np.arange(n) % 3 == 0, 0, 2)                        # no valid node: an empty split
    pred = np.where(np.isnan(lg).any(1), np.isnan(lg).argmax(1), np.nan_to_num(lg, nan=-np.inf).argmax(1))
    hit = pred == y
    want = [float((hit & (sid == s)).sum()) for s in range(3)] + [float((sid == s).sum()) for s in range(3)]
    split = {k: torch.from_numpy(np.nonzero(sid == s)[0]).to(DEV) for s, k in enumerate(("train", "valid", "test"))}
    logits, yd = torch.from_numpy(lg).to(DEV), torch.from_numpy(y).to(DEV)
    assert ops.split_accuracy(logits, yd, split, counts=True).cpu().tolist() == want
    acc = ops.split_accuracy(logits, yd, split).cpu().numpy()
    assert acc[0] == want[0] / want[3] and np.isnan(acc[1]) and (want[5] == 0 or acc[2] == want[2] / want[5])
