"""GPU tests of the structure-preservation metrics (csrc/similarity.hip, efficient-gnns_amd/similarity.py, models.student_similarity).

References are float64 and written here from the definitions: ``scipy.stats.pearsonr`` over the ``np.triu_indices`` pairs of
``1 - A @ A.T`` (global), over the per-edge cosine distances (local), and linear CKA through the explicit n x n centring H K H -- a
different route from the product's feature-space form.

Tolerance rule, per case: the fp32 restatement of the reference's own arithmetic (an fp32 ``torch.mm`` on the CPU, the statistic then
taken in float64) must itself be within 1e-6 of float64 -- that shows the inputs are fair -- and the GPU must be within
``max(20 x that case's CPU fp32 deviation, 1e-6)`` of float64: absolute for r and CKA, relative for the five sums (the inputs of the
sum tests are positive, so no sum is a cancellation and |sum| is its natural scale).  The factor 20 covers the MFMA's accumulation
order and the kernel's fp32 per-lane partial sums."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.stats import pearsonr

import efficient_gnns_amd as E
import efficient_gnns_amd.models as M
import efficient_gnns_amd.similarity as S
from efficient_gnns_amd import _lib
from efficient_gnns_amd.utils import subgraph

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1e-6
NS = (2, 3, 127, 128, 129, 257, 641)
DIMS = ((8, 8), (5, 7), (130, 66), (256, 750))


def bound(cpu_dev):
    assert cpu_dev <= FLOOR, f"the fp32 restatement is {cpu_dev:.3g} away from float64: unfair inputs"
    return max(20.0 * cpu_dev, FLOOR)


def positive_features(N, D, seed):
    """Correlated positive rows (a shared 4-d latent plus noise, magnitudes): every cosine is well above 0."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 4, generator=g)
    return (z @ torch.randn(4, D, generator=g) + 0.5 * torch.randn(N, D, generator=g)).abs() + 0.05


def relu_features(N, D, seed, latent=None, noise=0.5):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 6, generator=g) if latent is None else latent
    return torch.relu(z @ torch.randn(6, D, generator=g) + noise * torch.randn(N, D, generator=g))


def unit64(x):
    x = x.double().numpy()
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def sums_over_pairs(As, At):
    iu = np.triu_indices(As.shape[0], 1)
    a, b = As[iu].astype(np.float64), At[iu].astype(np.float64)
    return np.array([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()])


@functools.lru_cache(maxsize=None)
def moments_case(N, Ds, Dt):
    """Unit fp32 rows, the float64 sums over i < j of their Grams, and the relative deviation of the fp32-mm restatement per sum."""
    xs = F.normalize(positive_features(N, Ds, 7 * N + Ds))
    xt = F.normalize(positive_features(N, Dt, 11 * N + Dt))
    xs64, xt64 = xs.double().numpy(), xt.double().numpy()
    ref = sums_over_pairs(xs64 @ xs64.T, xt64 @ xt64.T)
    cpu = sums_over_pairs(torch.mm(xs, xs.t()).numpy(), torch.mm(xt, xt.t()).numpy())
    return xs, xt, ref, np.abs(cpu - ref) / np.abs(ref)


def lay_out(x, layout):
    """The same values as a contiguous tensor, a column block at a 1-float offset of a wider buffer (unaligned rows: the scalar-load
    path), or behind a 16-byte aligned padded pitch (the float4 path with a ragged K)."""
    x = x.to(DEV)
    if layout == "contiguous":
        return x
    if layout == "offset1":
        B, C = x.shape
        buf = torch.full((B, C + 3), 9.0, dtype=torch.float32, device=DEV)   # loud neighbours: a read past a row shows in the sums
        buf[:, 1:1 + C] = x
        return buf[:, 1:1 + C]
    B, C = x.shape
    buf = torch.full((B, (C + 3) // 4 * 4 + 4), 9.0, dtype=torch.float32, device=DEV)
    buf[:, :C] = x
    return buf[:, :C]


# ------------------------------------------------------------------------------------------------ all-pairs moments
@pytest.mark.parametrize("layout", ["contiguous", "offset1", "padded"])
@pytest.mark.parametrize("Ds,Dt", DIMS)
@pytest.mark.parametrize("N", NS)
def test_pair_moments_match_float64(N, Ds, Dt, layout):
    xs, xt, ref, cpu_rel = moments_case(N, Ds, Dt)
    got = S.pair_moments(lay_out(xs, layout), lay_out(xt, layout)).cpu().numpy()
    rel = np.abs(got[1:] - ref) / np.abs(ref)
    print(f"N={N} D=({Ds},{Dt}) {layout}: n={got[0]:.0f} gpu rel {rel.max():.3g} cpu fp32 rel {cpu_rel.max():.3g}")
    assert got[0] == N * (N - 1) // 2            # a dropped or doubled tile shows here, whatever r says
    for q in range(5):
        assert rel[q] <= bound(cpu_rel[q]), (q, rel[q], cpu_rel[q])


@pytest.mark.parametrize("N", [29_799, 169_343])
def test_pair_moments_tile_map_at_full_size(N):
    """233 and 1 323 tiles per side (27 261 / 875 826 workgroups): the block index -> (ti, tj) map must hit every upper tile once.
    Narrow rows keep it to milliseconds; the float64 reference is the closed form, O(N D^2):
      sum_{i<j} a = (|sum_i x_i|^2 - sum_i |x_i|^2) / 2,  sum a^2 = (|X^T X|_F^2 - sum_i |x_i|^4) / 2,
      sum ab = (|Xs^T Xt|_F^2 - sum_i |xs_i|^2 |xt_i|^2) / 2.
    No fp32 restatement exists at this size (it would be the N x N matrix), so the floor of the tolerance rule alone applies."""
    xs = F.normalize(positive_features(N, 8, 3))
    xt = F.normalize(positive_features(N, 8, 4))
    s, t = xs.double().numpy(), xt.double().numpy()
    ns, nt = (s * s).sum(1), (t * t).sum(1)
    fro2 = lambda m: (m * m).sum()   # noqa: E731
    ref = np.array([(fro2(s.sum(0)) - ns.sum()) / 2, (fro2(t.sum(0)) - nt.sum()) / 2, (fro2(s.T @ s) - (ns * ns).sum()) / 2,
                    (fro2(t.T @ t) - (nt * nt).sum()) / 2, (fro2(s.T @ t) - (ns * nt).sum()) / 2])
    got = S.pair_moments(xs.to(DEV), xt.to(DEV)).cpu().numpy()
    rel = np.abs(got[1:] - ref) / np.abs(ref)
    print(f"N={N}: n={got[0]:.0f} gpu rel {rel.max():.3g}")
    assert got[0] == N * (N - 1) // 2
    assert rel.max() <= FLOOR, rel


@pytest.mark.parametrize("N,Ds,Dt", [(2, 5, 7), (129, 130, 66), (641, 256, 750)])
def test_pair_moments_two_calls_are_bit_equal(N, Ds, Dt):
    xs, xt, _, _ = moments_case(N, Ds, Dt)
    xs, xt = xs.to(DEV), xt.to(DEV)
    a, b = S.pair_moments(xs, xt), S.pair_moments(xs, xt)
    assert torch.equal(a, b)


def test_pair_moments_error_codes():
    lib = _lib.load()
    xs, xt, _, _ = moments_case(129, 8, 8)
    xs, xt = xs.to(DEV), xt.to(DEV)
    out = torch.zeros(6, dtype=torch.float64, device=DEV)
    need = lib.egnn_pair_moments_ws_bytes(129)
    assert need == 3 * 6 * 8
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    call = lambda n, nbytes: lib.egnn_pair_moments_f32(_lib.ptr(xs), 8, 8, _lib.ptr(xt), 8, 8, n, _lib.ptr(out), _lib.ptr(ws), nbytes,  # noqa: E731
                                                       _lib.stream())
    assert call(129, need - 1) == -3       # EGNN_EWORKSPACE
    assert call(1, need) == -1             # EGNN_EINVAL
    assert call(129, need) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == 129 * 128 // 2
    with pytest.raises(ValueError):
        S.pair_moments(xs[:1], xt[:1])
    with pytest.raises(ValueError):
        S.pair_moments(xs, xt[:100])


# ------------------------------------------------------------------------------------------------ global r
def r_global_refs(x, t, idx):
    """(float64 r, |fp32-mm restatement - float64 r|) of the cosine-distance matrices of rows idx."""
    if idx is not None:
        x, t = x[idx], t[idx]
    iu = np.triu_indices(x.shape[0], 1)
    xs64, xt64 = unit64(x), unit64(t)
    r64 = pearsonr((1 - xs64 @ xs64.T)[iu], (1 - xt64 @ xt64.T)[iu])[0]
    fs, ft = F.normalize(x), F.normalize(t)
    r32 = pearsonr((1 - torch.mm(fs, fs.t())).double().numpy()[iu], (1 - torch.mm(ft, ft.t())).double().numpy()[iu])[0]
    return r64, abs(r32 - r64)


def anti_correlated(xs, seed):
    """Teacher rows whose cosines FALL where the student's rise: Gram = alpha 11^T - k G_s + beta I (positive definite for
    beta > k lambda_max), realised through its symmetric square root, plus a little noise."""
    G = unit64(xs) @ unit64(xs).T
    N = G.shape[0]
    k = 1.4 / N                                # lambda_max(G) <= N, so k lambda_max <= 1.4 < beta
    Gt = 0.5 * np.ones((N, N)) - k * G + 1.5 * np.eye(N)
    w, V = np.linalg.eigh(Gt)
    T = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    g = torch.Generator().manual_seed(seed)
    return torch.from_numpy(T).float() + 0.0005 * torch.randn(N, N, generator=g)


@functools.lru_cache(maxsize=None)
def global_case(name):
    N, Ds, Dt = 300, 64, 96
    g = torch.Generator().manual_seed(5)
    z = torch.randn(N, 6, generator=g)
    x = relu_features(N, Ds, 21, latent=z)
    idx = None
    if name == "correlated":
        t = relu_features(N, Dt, 22, latent=z)
    elif name == "identical":
        t = x.clone()
    elif name == "anti":
        x = x[:96]
        t = anti_correlated(x, 23)
    elif name == "independent":
        t = relu_features(N, Dt, 24)
    else:   # a repeated index and an all-zero row (cosine 0 to everything, as F.normalize gives)
        t = relu_features(N, Dt, 22, latent=z)
        x, t = x.clone(), t.clone()
        x[17] = 0.0
        t[17] = 0.0
        idx = torch.cat([torch.randperm(N, generator=g)[:150], torch.tensor([17, 40, 40])])
    return x, t, idx, r_global_refs(x, t, idx)


@pytest.mark.parametrize("name", ["correlated", "identical", "anti", "independent", "repeat_zero"])
def test_structural_correlation_matches_float64(name):
    x, t, idx, (r64, cpu_dev) = global_case(name)
    got = E.structural_correlation(x.to(DEV), t.to(DEV), None if idx is None else idx.to(DEV))
    print(f"global {name}: r64={r64:.9f} gpu dev {abs(got - r64):.3g} cpu fp32 dev {cpu_dev:.3g}")
    assert isinstance(got, float)
    assert abs(got - r64) <= bound(cpu_dev)
    if name == "correlated":
        assert r64 > 0.5
    elif name == "identical":
        assert abs(r64 - 1.0) <= 1e-12 and got == 1.0
        # r == 1 is reached through the clamp of pearson_from_moments: the moments themselves must say a == b, bit for bit
        xh = F.normalize(x).to(DEV)
        m = S.pair_moments(xh, xh).tolist()
        assert m[1] == m[2] and m[3] == m[4] == m[5]
    elif name == "anti":
        assert r64 < -0.5
    elif name == "independent":
        assert abs(r64) < 0.1


# ------------------------------------------------------------------------------------------------ local r
@functools.lru_cache(maxsize=None)
def local_case(n_edges, with_idx):
    N, Ds, Dt = 200, 64, 96
    g = torch.Generator().manual_seed(100 + n_edges)
    z = torch.randn(N, 6, generator=g)
    x, t = relu_features(N, Ds, 31, latent=z), relu_features(N, Dt, 32, latent=z)
    idx = torch.randperm(N, generator=g)[:120] if with_idx else None
    n = 120 if with_idx else N
    ei = torch.randint(0, n, (2, n_edges), generator=g)
    ei[1] = torch.where(ei[1] == ei[0], (ei[1] + 1) % n, ei[1])
    if n_edges > 0:
        ei[:, 0] = 3                        # a self-loop edge: cosine 1 on both sides
    xr, tr = (x, t) if idx is None else (x[idx], t[idx])
    src, dst = ei[0].numpy(), ei[1].numpy()
    if n_edges < 2:
        return x, t, idx, ei, (math.nan, 0.0)
    xs64, xt64 = unit64(xr), unit64(tr)
    d64 = lambda u: 1 - (u[src] * u[dst]).sum(1)   # noqa: E731
    r64 = pearsonr(d64(xt64), d64(xs64))[0]
    fs, ft = F.normalize(xr), F.normalize(tr)
    d32 = lambda f: (1 - F.cosine_similarity(f[ei[0]], f[ei[1]])).double().numpy()   # noqa: E731
    r32 = pearsonr(d32(ft), d32(fs))[0]
    return x, t, idx, ei, (r64, abs(r32 - r64))


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("n_edges", [2, 63, 64, 65, 1000])
def test_local_structural_correlation_matches_float64(n_edges, with_idx):
    x, t, idx, ei, (r64, cpu_dev) = local_case(n_edges, with_idx)
    got = E.local_structural_correlation(x.to(DEV), t.to(DEV), ei.to(DEV), None if idx is None else idx.to(DEV))
    print(f"local E={n_edges} idx={with_idx}: r64={r64:.9f} gpu dev {abs(got - r64):.3g} cpu fp32 dev {cpu_dev:.3g}")
    assert isinstance(got, float)
    assert abs(got - r64) <= bound(cpu_dev)


def test_local_structural_correlation_argument_errors():
    x, t, _, ei, _ = local_case(1, False)
    x, t = x.to(DEV), t.to(DEV)
    with pytest.raises(ValueError, match="at least 2 edges"):
        E.local_structural_correlation(x, t, ei.to(DEV))
    with pytest.raises(ValueError):
        E.local_structural_correlation(x, t, torch.tensor([[0, 1, 2], [1, 2, 200]], device=DEV))   # row 200 of 200
    with pytest.raises(ValueError):
        E.local_structural_correlation(x, t, torch.tensor([[0, 1, -1], [1, 2, 0]], device=DEV))


def test_vector_moments_two_calls_are_bit_equal_and_match_float64():
    g = torch.Generator().manual_seed(9)
    for n in (1, 255, 256, 257, 300001):     # one block, a ragged block, more elements than the grid has threads
        a, b = torch.rand(n, generator=g) + 0.1, torch.rand(n, generator=g) + 0.1
        m1, m2 = S.vector_moments(a.to(DEV), b.to(DEV)), S.vector_moments(a.to(DEV), b.to(DEV))
        assert torch.equal(m1, m2)
        a64, b64 = a.double().numpy(), b.double().numpy()
        ref = np.array([n, a64.sum(), b64.sum(), (a64 * a64).sum(), (b64 * b64).sum(), (a64 * b64).sum()])
        got = m1.cpu().numpy()
        assert got[0] == n
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), (n, got, ref)   # float64 from the first addition on


# ------------------------------------------------------------------------------------------------ CKA
def cka_nxn(X, Y):
    """Linear CKA through the explicit n x n centring: sum(HKH o HLH) / sqrt(sum(HKH^2) sum(HLH^2)), K = X X^T, L = Y Y^T."""
    return cka_from_grams(X @ X.T, Y @ Y.T)


def cka_from_grams(K, L):
    n = K.shape[0]
    H = np.eye(n) - np.ones((n, n)) / n
    Kc, Lc = H @ K @ H, H @ L @ H
    return (Kc * Lc).sum() / math.sqrt((Kc * Kc).sum() * (Lc * Lc).sum())


def cka_refs(x, t, normalize=True):
    if normalize:
        X64, Y64, X32, Y32 = unit64(x), unit64(t), F.normalize(x), F.normalize(t)
    else:
        X64, Y64, X32, Y32 = x.double().numpy(), t.double().numpy(), x, t
    c64 = cka_nxn(X64, Y64)
    c32 = cka_from_grams(torch.mm(X32, X32.t()).double().numpy(), torch.mm(Y32, Y32.t()).double().numpy())
    return c64, abs(c32 - c64)


@functools.lru_cache(maxsize=None)
def cka_case(N, Ds, Dt):
    g = torch.Generator().manual_seed(N + Ds)
    z = torch.randn(N, 6, generator=g)
    x, t = relu_features(N, Ds, 41, latent=z) + 0.01, relu_features(N, Dt, 42, latent=z) + 0.01
    return x, t, cka_refs(x, t)


@pytest.mark.parametrize("Ds,Dt", [(8, 8), (64, 96)])
@pytest.mark.parametrize("N", [2, 3, 129, 1000])
def test_linear_cka_matches_the_nxn_centring_form(N, Ds, Dt):
    x, t, (c64, cpu_dev) = cka_case(N, Ds, Dt)
    got = E.linear_cka(x.to(DEV), t.to(DEV))
    print(f"cka N={N} D=({Ds},{Dt}): c64={c64:.9f} gpu dev {abs(got - c64):.3g} cpu fp32 dev {cpu_dev:.3g}")
    assert isinstance(got, float)
    assert abs(got - c64) <= bound(cpu_dev)
    idx = torch.arange(N - 1, -1, -1)      # CKA does not depend on the order of the rows
    assert abs(E.linear_cka(x.to(DEV), t.to(DEV), idx.to(DEV)) - c64) <= bound(cpu_dev)


def test_linear_cka_of_a_matrix_with_itself_is_one():
    x, _, _ = cka_case(129, 64, 96)
    assert E.linear_cka(x.to(DEV), x.to(DEV)) == 1.0
    assert E.linear_cka(x.to(DEV), x.to(DEV), normalize=False) == 1.0


def test_linear_cka_is_invariant_under_an_orthogonal_map():
    x, _, _ = cka_case(129, 64, 96)
    g = torch.Generator().manual_seed(3)
    Q, _ = torch.linalg.qr(torch.randn(64, 64, generator=g, dtype=torch.float64))
    xq = (x.double() @ Q).float()
    c64, cpu_dev = cka_refs(x, xq, normalize=False)
    assert abs(c64 - 1.0) <= 1e-6           # XQ rounded to fp32 is the only departure from exact invariance
    got = E.linear_cka(x.to(DEV), xq.to(DEV), normalize=False)
    print(f"cka orthogonal: c64={c64:.9f} gpu dev {abs(got - c64):.3g} cpu fp32 dev {cpu_dev:.3g}")
    assert abs(got - c64) <= bound(cpu_dev)
    assert abs(got - E.linear_cka(x.to(DEV), x.to(DEV), normalize=False)) <= 2 * bound(cpu_dev)


def test_linear_cka_of_constant_features_is_nan():
    x = torch.ones(10, 8, device=DEV)
    t = torch.rand(10, 8, generator=torch.Generator().manual_seed(0)).to(DEV)
    assert math.isnan(E.linear_cka(x, t))


# ------------------------------------------------------------------------------------------------ memory
def test_structural_correlation_allocates_no_n_by_n_object():
    N, Ds, Dt = 4096, 64, 96
    x, t = relu_features(N, Ds, 51).to(DEV), relu_features(N, Dt, 52).to(DEV)
    E.structural_correlation(x[:256], t[:256])     # the library and the allocator are warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = E.structural_correlation(x, t)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"memory: N={N} peak growth {grown} bytes, one Gram would be {N * N * 4}")
    assert math.isfinite(r)
    assert grown < N * N * 4


# ------------------------------------------------------------------------------------------------ the combined entry points
@functools.lru_cache(maxsize=None)
def graph_case():
    N = 200
    g = torch.Generator().manual_seed(77)
    a, b = torch.randint(0, N, (2, 900), generator=g)
    keep = a != b
    a, b = a[keep], b[keep]
    key = torch.unique(torch.cat([a * N + b, b * N + a]))         # symmetric, no duplicates
    ei = torch.stack([key // N, key % N])
    x = torch.randn(N, 16, generator=g)
    teacher = relu_features(N, 24, 61)
    idx = torch.randperm(N, generator=g)[:120]
    return N, ei, x, teacher, idx


def test_representation_similarity_equals_the_three_calls():
    N, ei, _, teacher, idx = graph_case()
    feat = relu_features(N, 32, 62).to(DEV)
    teacher, idx, ei = teacher.to(DEV), idx.to(DEV), ei.to(DEV)
    got = E.representation_similarity(feat, teacher, idx, ei)
    assert sorted(got) == ["cka", "global_", "local"]
    sub = subgraph(idx, ei, relabel_nodes=True, num_nodes=N)[0]
    assert sub.shape[1] >= 2
    assert got["global_"] == E.structural_correlation(feat, teacher, idx)
    assert got["local"] == E.local_structural_correlation(feat, teacher, sub, idx)
    assert got["cka"] == E.linear_cka(feat, teacher, idx)
    assert all(isinstance(v, float) for v in got.values())
    assert E.representation_similarity(feat, teacher, idx)["local"] is None


def test_student_similarity_runs_one_eval_forward_and_restores_the_model():
    N, ei, x, teacher, idx = graph_case()
    adj = E.SparseTensor(row=ei[1], col=ei[0], sparse_sizes=(N, N)).to(DEV)
    x, teacher, idx, ei = x.to(DEV), teacher.to(DEV), idx.to(DEV), ei.to(DEV)
    torch.manual_seed(0)
    model = M.SAGE(16, 32, 5, 2, 0.5).to(DEV)
    model.train()
    model(x, adj)                                   # running statistics away from their initial values
    state = {k: v.clone() for k, v in model.state_dict().items()}
    for training in (True, False):
        model.train(training)
        got = M.student_similarity(model, x, adj, teacher, idx, ei)
        assert model.training is training and all(m.training is training for m in model.modules())
        now = model.state_dict()
        assert sorted(now) == sorted(state) and all(torch.equal(now[k], state[k]) for k in state)
        model.eval()
        with torch.no_grad():
            model(x, adj)
        want = E.representation_similarity(model.out_feat, teacher, idx, ei)
        assert sorted(got) == ["cka", "global_", "local"]
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    assert not any(p.grad is not None for p in model.parameters())
