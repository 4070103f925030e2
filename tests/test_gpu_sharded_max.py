"""Max aggregation on a node-range shard, on the GPU (single process): egnn_spmm_csr_max_piece_f32 (own piece from scratch, halo piece
merged) against the one-call kernel over the unsplit [own | halo] matrix, and the gather-form backward egnn_spmm_csr_max_bwd_rows_f32
against a float64 statement built from argmax.

ONE hand-built shard (rank 1 of 3, so halo columns lie on BOTH sides of the own ones in the row's CSR order): 67 rows, 67 own and 9 halo
columns; row 0 is a hub with 150 own + 9 halo entries (two 64-entry chunk boundaries), the others are own-only, halo-only, mixed or
empty; row 2 is halo-only with negative candidates only.  x in {-2, -1, 0, 1}: ties within and across the pieces, the first maximal entry
now in one piece, now in the other.  Max involves no rounding: forward bars are equality."""
import ctypes
import types

import pytest
import torch

import efficient_gnns_amd.dist as DD
import efficient_gnns_amd.models as PM
import efficient_gnns_amd.ops as ops
from efficient_gnns_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_LOCAL, WORLD, RANK = 67, 3, 1
N = N_LOCAL * WORLD
LO = N_LOCAL * RANK
HALO_IDS = [3, 20, 41, 66, 134, 150, 151, 177, 200]            # 4 below the own range, 5 above it
NEG_ROW, NEG_HALO = 2, (20, 151)                                 # row 2 references only these two halo nodes, whose x rows are negative
KS = [1, 5, 40, 64, 132]
EINVAL = -1


def _shard():
    """(rowptr_local, col_global) of the hand-built shard, columns ascending within every row."""
    g = torch.Generator().manual_seed(5)
    own = torch.arange(LO, LO + N_LOCAL)
    halo = torch.tensor(HALO_IDS)
    rows = [torch.cat([own[torch.arange(150) % N_LOCAL], halo])]             # the hub: 150 own (every column 2-3 times) + 9 halo entries
    for r in range(1, N_LOCAL):
        kind = r % 5
        n_own = int(torch.randint(1, 12, (1,), generator=g))
        n_halo = int(torch.randint(1, 6, (1,), generator=g))
        pick_own = own[torch.randperm(N_LOCAL, generator=g)[:n_own]]
        pick_halo = halo[torch.randperm(9, generator=g)[:n_halo]]
        if r == NEG_ROW:
            rows.append(torch.tensor(NEG_HALO))
        elif kind == 0:
            rows.append(torch.cat([pick_own, pick_halo]))
        elif kind == 1:
            rows.append(pick_own)
        elif kind == 2:
            rows.append(pick_halo)
        elif kind == 3:
            rows.append(torch.zeros(0, dtype=torch.int64))
        else:
            rows.append(torch.cat([pick_own, pick_own[:2], pick_halo]))     # duplicate entries: equal candidates inside one piece
    rows = [torch.sort(r)[0] for r in rows]
    rowptr = torch.zeros(N_LOCAL + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
    return rowptr, torch.cat(rows)


def _values(rowptr, nnz):
    """Per-entry values with both signs (exact in fp32 against the small-integer x); the all-negative row keeps positive ones."""
    g = torch.Generator().manual_seed(6)
    val = torch.tensor([-1.5, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 5, (nnz,), generator=g)]
    val[int(rowptr[NEG_ROW]):int(rowptr[NEG_ROW + 1])] = torch.tensor([0.5, 2.0])
    return val


class _Case:
    def __init__(self, with_val):
        rowptr, col = _shard()
        val = _values(rowptr, col.numel()) if with_val else None
        plan = DD.ShardPlan(N, WORLD, RANK, rowptr, col, val, torch.zeros(0, dtype=torch.int64), [0] * WORLD)
        assert plan.n_local == N_LOCAL and plan.n_halo == 9 and plan.halo_ids.tolist() == HALO_IDS
        self.sadj = DD.ShardedAdj(None, None, N, WORLD, RANK, DEV, None, with_gcn=False, _plan=plan)
        self.plan = plan
        self.mp = self.sadj._max_plan(valueless=not with_val)
        self.local = self.sadj.raw                                          # plan.local_adj(): the unsplit [own | halo] matrix
        self.refs = {}

    def x_ext(self, K, aligned=True):
        g = torch.Generator().manual_seed(100 + K)
        x = torch.randint(-2, 2, (N_LOCAL + 9, K), generator=g).float()
        for h in NEG_HALO:
            x[N_LOCAL + HALO_IDS.index(h)] = torch.randint(-2, 0, (K,), generator=g).float()
        if aligned:
            return x.to(DEV)
        buf = torch.zeros(N_LOCAL + 9, K + 1, device=DEV)                   # rows behind an odd pitch, one float off 16-byte alignment
        buf[:, 1:] = x.to(DEV)
        return buf[:, 1:]

    def reference(self, K):
        """The one-call kernel over the unsplit matrix (computed once per K, never written afterwards)."""
        if K not in self.refs:
            y, arg = ops.spmm_raw(self.local, self.x_ext(K), "max")
            self.refs[K] = (y.clone(), arg.clone())
        return self.refs[K]


@pytest.fixture(scope="module", params=[False, True], ids=["noval", "val"])
def case(request):
    return _Case(request.param)


def _pieces(case, x_ext, own_first=True):
    mp = case.mp
    x_own, x_halo = x_ext[:N_LOCAL], x_ext[N_LOCAL:]
    order = [(mp.own, x_own, mp.eid_own), (mp.halo, x_halo, mp.eid_halo)]
    if not own_first:
        order.reverse()
    y, arg = ops.spmm_max_piece(*order[0], False)
    return ops.spmm_max_piece(*order[1], True, y, arg)


def test_the_shard_has_every_kind_of_row(case):
    cnt_own = (case.mp.own.csr()[0][1:] - case.mp.own.csr()[0][:-1]).cpu()
    cnt_halo = (case.mp.halo.csr()[0][1:] - case.mp.halo.csr()[0][:-1]).cpu()
    assert cnt_own[0] == 150 and cnt_halo[0] == 9
    assert int(((cnt_own > 0) & (cnt_halo == 0)).sum()) > 3 and int(((cnt_own == 0) & (cnt_halo > 0)).sum()) > 3
    assert int(((cnt_own == 0) & (cnt_halo == 0)).sum()) > 3 and int(((cnt_own > 0) & (cnt_halo > 0)).sum()) > 3
    assert cnt_own[NEG_ROW] == 0 and cnt_halo[NEG_ROW] == 2
    # ties across the pieces occur with the winner on either side: some argmax ids belong to the halo piece although the row has own entries
    _, arg = case.reference(5)
    arg = arg.cpu()
    is_halo = torch.zeros(case.local.nnz() + 1, dtype=torch.bool)
    is_halo[case.mp.eid_halo.cpu()] = True
    mixed = ((cnt_own > 0) & (cnt_halo > 0)).unsqueeze(1) & (arg >= 0)
    won_by_halo = is_halo[arg.clamp(min=0)] & mixed
    assert bool(won_by_halo.any()) and bool((mixed & ~won_by_halo).any())


@pytest.mark.parametrize("K", KS)
def test_own_then_halo_piece_equals_the_unsplit_kernel(case, K):
    y_ref, arg_ref = case.reference(K)
    y, arg = _pieces(case, case.x_ext(K))
    assert torch.equal(arg, arg_ref), "merged argmax must be the first maximal entry of the whole row in local_adj numbering"
    assert torch.equal(y, y_ref)


@pytest.mark.parametrize("K", KS)
def test_halo_then_own_piece_gives_the_same_state(case, K):
    y_ref, arg_ref = case.reference(K)
    y, arg = _pieces(case, case.x_ext(K), own_first=False)
    assert torch.equal(arg, arg_ref) and torch.equal(y, y_ref)


@pytest.mark.parametrize("K", [40, 132])
def test_pieces_on_rows_that_are_not_16_byte_aligned_take_the_scalar_path(case, K):
    """K % 4 == 0 behind an odd pitch: the scalar lanes (132 columns: three column slices of 64 lanes)."""
    y_ref, arg_ref = case.reference(K)
    x = case.x_ext(K, aligned=False)
    assert x.data_ptr() % 16 != 0 and x.stride(0) % 4 != 0
    for own_first in (True, False):
        y, arg = _pieces(case, x, own_first)
        assert torch.equal(arg, arg_ref) and torch.equal(y, y_ref)


@pytest.mark.parametrize("K", KS)
def test_one_piece_from_scratch_without_ids_equals_the_existing_kernel(case, K):
    x = case.x_ext(K)
    y_ref, arg_ref = case.reference(K)
    y_rows, arg_rows = ops.spmm_raw(case.local, x, "max", use_plan=False)     # egnn_spmm_csr_f32 with its three row lists NULL
    y, arg = ops.spmm_max_piece(case.local, x)
    assert torch.equal(arg, arg_rows) and torch.equal(y, y_rows)
    assert torch.equal(arg, arg_ref) and torch.equal(y, y_ref)


@pytest.mark.parametrize("K", KS)
def test_negative_halo_only_row_keeps_its_negative_maximum_and_empty_rows_are_zero(case, K):
    y, arg = _pieces(case, case.x_ext(K))
    assert bool((y[NEG_ROW] < 0).all()), "a row without own entries must not compare against the 0.0 of its empty state"
    assert bool((arg[NEG_ROW] >= 0).all())
    rowptr = case.local.csr()[0]
    empty = rowptr[1:] == rowptr[:-1]
    assert int(empty.sum()) > 3
    assert bool((y[empty] == 0).all()) and bool((arg[empty] == -1).all())


def _bwd_raw(t_adj, t_eid, val, arg, gy, addend=None):
    """The C entry point itself, on a destination pre-filled with NaN."""
    n_src, n_rows = t_adj.sparse_sizes()
    K = gy.shape[1]
    gx = torch.full((n_src, K), float("nan"), device=DEV)
    rowptr, col, bits = t_adj._index_arrays()
    rc = _lib.load().egnn_spmm_csr_max_bwd_rows_f32(n_src, n_rows, K, _lib.ptr(rowptr), _lib.ptr(col), bits, _lib.ptr(t_eid), _lib.ptr(val),
                                                    _lib.ptr(arg), _lib.ptr(gy), gy.stride(0), _lib.ptr(addend),
                                                    0 if addend is None else addend.stride(0), _lib.ptr(gx), gx.stride(0), _lib.stream())
    assert rc == 0
    return gx


def _bwd_float64(case, arg, gy):
    """dX over the extended columns from argmax alone, in float64: (sum of terms, sum of |terms|, number of terms) per element."""
    _, col, val = case.local.csr()
    K = gy.shape[1]
    n_ext = N_LOCAL + 9
    valid = arg >= 0
    e = arg.clamp(min=0)
    term = gy.double() if val is None else gy.double() * val.double()[e]
    term = torch.where(valid, term, torch.zeros_like(term))
    src = col[e]
    kk = torch.arange(K, device=DEV).expand_as(src)
    flat = (src * K + kk).reshape(-1)
    out = [torch.zeros(n_ext * K, dtype=torch.float64, device=DEV).index_add_(0, flat, t.reshape(-1)).view(n_ext, K)
           for t in (term, term.abs(), valid.double())]
    return out


U = 2.0 ** -24


@pytest.mark.parametrize("K", KS)
def test_gather_backward_against_float64(case, K):
    mp = case.mp
    y, arg = _pieces(case, case.x_ext(K))
    g = torch.Generator().manual_seed(200 + K)
    gy = torch.randn(N_LOCAL, K, generator=g).to(DEV)
    ref, abs_sum, m = _bwd_float64(case, arg, gy)
    got = torch.cat([_bwd_raw(mp.own_t, mp.t_eid_own, mp.val, arg, gy), _bwd_raw(mp.halo_t, mp.t_eid_halo, mp.val, arg, gy)])
    assert got.shape == ref.shape and not bool(torch.isnan(got).any()), "every element of dX must be written"
    assert bool((got[m == 0] == 0).all()), "rows nobody picked are exactly 0"
    assert int((m == 0).sum()) > 0 and int((m > 1).sum()) > 0
    err = (got.double() - ref).abs()
    bound = m * U * abs_sum                                                   # the fp32 summation bound of m terms
    assert bool((err <= bound).all()), float((err - bound).max())
    again = torch.cat([_bwd_raw(mp.own_t, mp.t_eid_own, mp.val, arg, gy), _bwd_raw(mp.halo_t, mp.t_eid_halo, mp.val, arg, gy)])
    assert torch.equal(got, again), "two runs must be bit-equal"
    # the ops wrapper (its own allocation) is the same call
    assert torch.equal(ops.spmm_max_bwd_rows(mp.own_t, mp.t_eid_own, mp.val, arg, gy), got[:N_LOCAL])


@pytest.mark.parametrize("K", KS)
def test_gather_backward_with_addend(case, K):
    """dX = addend + picked gradients.  On dyadic data (every partial sum exact in fp32) the addend form IS the plain form plus the addend;
    on normal data it stays inside the fp32 bound of its own chain: the sum starts at the addend and makes m rounded additions, each of a
    partial sum no larger than |addend| + sum |terms|, so |error| <= m 2^-24 (|addend| + sum |terms|) (and exactly the addend where m = 0)."""
    mp = case.mp
    y, arg = _pieces(case, case.x_ext(K))
    g = torch.Generator().manual_seed(300 + K)
    gy = (torch.randint(-32, 33, (N_LOCAL, K), generator=g).float() / 8).to(DEV)
    add = (torch.randint(-32, 33, (N_LOCAL + 9, K), generator=g).float() / 8).to(DEV)
    for t_adj, t_eid, sl in ((mp.own_t, mp.t_eid_own, slice(0, N_LOCAL)), (mp.halo_t, mp.t_eid_halo, slice(N_LOCAL, N_LOCAL + 9))):
        a = add[sl].contiguous()
        plain = _bwd_raw(t_adj, t_eid, mp.val, arg, gy)
        with_add = _bwd_raw(t_adj, t_eid, mp.val, arg, gy, a)
        assert not bool(torch.isnan(with_add).any())
        assert torch.equal(with_add, plain + a)
    gy = torch.randn(N_LOCAL, K, generator=g).to(DEV)
    add = torch.randn(N_LOCAL + 9, K, generator=g).to(DEV)
    ref, abs_sum, m = _bwd_float64(case, arg, gy)
    got = torch.cat([_bwd_raw(mp.own_t, mp.t_eid_own, mp.val, arg, gy, add[:N_LOCAL].contiguous()),
                     _bwd_raw(mp.halo_t, mp.t_eid_halo, mp.val, arg, gy, add[N_LOCAL:].contiguous())])
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got[m == 0], add[m == 0]), "rows nobody picked receive the addend"
    err = (got.double() - (ref + add.double())).abs()
    bound = m * U * (abs_sum + add.double().abs())
    assert bool((err <= bound).all()), float((err - bound).max())


def test_gather_backward_on_unaligned_rows_takes_the_scalar_path(case):
    K = 40
    mp = case.mp
    y, arg = _pieces(case, case.x_ext(K))
    g = torch.Generator().manual_seed(77)
    gy = torch.randn(N_LOCAL, K, generator=g).to(DEV)
    buf = torch.zeros(N_LOCAL, K + 1, device=DEV)
    buf[:, 1:] = gy
    ref = _bwd_raw(mp.own_t, mp.t_eid_own, mp.val, arg, gy)
    assert torch.equal(_bwd_raw(mp.own_t, mp.t_eid_own, mp.val, arg, buf[:, 1:]), ref)     # same order of addition on both paths


def test_int64_index_arrays_give_the_same_results(case):
    """The host narrows its index arrays to int32 whenever they fit; the 64-bit instantiations through the C entry points themselves."""
    K = 40
    mp, lib = case.mp, _lib.load()
    x = case.x_ext(K)
    y_ref, arg_ref = case.reference(K)
    y = torch.full((N_LOCAL, K), float("nan"), device=DEV)
    arg = torch.full((N_LOCAL, K), -7, dtype=torch.int64, device=DEV)
    for piece, xs, eid, merge in ((mp.own, x[:N_LOCAL], mp.eid_own, 0), (mp.halo, x[N_LOCAL:], mp.eid_halo, 1)):
        rowptr, col, _ = piece.csr()
        assert rowptr.dtype == col.dtype == torch.int64
        op = ops._spmm_desc(piece, rowptr, col, 64, xs, y, 2, None, None)
        assert lib.egnn_spmm_csr_max_piece_f32(ctypes.byref(op), _lib.ptr(eid), merge, _lib.ptr(arg), _lib.stream()) == 0
    assert torch.equal(arg, arg_ref) and torch.equal(y, y_ref)
    g = torch.Generator().manual_seed(78)
    gy = torch.randn(N_LOCAL, K, generator=g).to(DEV)
    for t_adj, t_eid in ((mp.own_t, mp.t_eid_own), (mp.halo_t, mp.t_eid_halo)):
        t_rowptr, t_row, _ = t_adj.csr()
        assert t_rowptr.dtype == t_row.dtype == torch.int64
        n_src = t_adj.sparse_size(0)
        gx = torch.full((n_src, K), float("nan"), device=DEV)
        rc = lib.egnn_spmm_csr_max_bwd_rows_f32(n_src, N_LOCAL, K, _lib.ptr(t_rowptr), _lib.ptr(t_row), 64, _lib.ptr(t_eid), _lib.ptr(mp.val),
                                                _lib.ptr(arg_ref), _lib.ptr(gy), K, None, 0, _lib.ptr(gx), K, _lib.stream())
        assert rc == 0 and torch.equal(gx, _bwd_raw(t_adj, t_eid, mp.val, arg_ref, gy))


def test_bias_or_relu_in_the_descriptor_is_einval(case):
    K = 8
    x = case.x_ext(K)[:N_LOCAL].contiguous()
    y = torch.zeros(N_LOCAL, K, device=DEV)
    arg = torch.full((N_LOCAL, K), -1, dtype=torch.int64, device=DEV)
    bias = torch.zeros(K, device=DEV)
    own = case.mp.own
    rowptr, col, bits = own._index_arrays()
    lib = _lib.load()

    def call(**kw):
        op = ops._spmm_desc(own, rowptr, col, bits, x, y, 2, None, None)
        for k, v in kw.items():
            setattr(op, k, v)
        return lib.egnn_spmm_csr_max_piece_f32(ctypes.byref(op), _lib.ptr(case.mp.eid_own), 0, _lib.ptr(arg), _lib.stream())
    assert call() == 0
    assert call(bias=_lib.ptr(bias)) == EINVAL
    assert call(flags=8) == EINVAL
    assert call(addend=_lib.ptr(y), ld_addend=K) == EINVAL
    assert call(stat_part=_lib.ptr(y)) == EINVAL
    assert call(reduce=0) == EINVAL


def test_sharded_aggregate_max_refuses_bias_and_relu(case):
    x = case.x_ext(8)[:N_LOCAL].contiguous()
    with pytest.raises(ValueError, match="bias"):
        case.sadj.aggregate(x, "max", valueless=True, bias=torch.zeros(8, device=DEV))
    with pytest.raises(ValueError, match="ReLU"):
        case.sadj.aggregate(x, "max", valueless=True, relu=True)


def test_sharded_graphed_epoch_refuses_a_max_model():
    model = PM.SAGE(16, 8, 4, 2, 0.0, aggr="max").to(DEV)
    prob = types.SimpleNamespace(x=torch.zeros(4, 16, device=DEV), world=1)
    with pytest.raises(ValueError, match="max"):
        DD.ShardedGraphedEpoch(model, prob, torch.optim.Adam(model.parameters()), "supervised", {})
