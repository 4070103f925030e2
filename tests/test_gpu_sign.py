"""GPU tests of the SIGN student (csrc/sign.hip, ops.sign_gather_drop / prelu_drop / linear_blocks / gemm_raw(out=), models.SIGN and its
loops): the kernels against float64 restatements written here with masks from ``oracle.dropout.counter_mask``; the model, its training
epochs and its test loop against tests/golden/sign.npz (the reference's own arxiv_dgl/sign.py, tests/golden/make_golden_sign.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import efficient_gnns_amd.models as M
from efficient_gnns_amd import _lib, ops
from oracle.dropout import counter_mask
from conftest import GOLDEN, as_t
from test_gpu_parity import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPES = (0.25, -0.5, 0.0)
HP = dict(alpha=0.9, kd_T=4.0, beta=0.5, nce_T=0.075, max_samples=64, kernel="rbf")
LR = 0.01


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "sign.npz"), allow_pickle=False)


def seeds_for(H, salt):
    rs = np.random.RandomState(1000 + salt)
    return [int(s) for s in rs.randint(0, 2 ** 62, size=H, dtype=np.int64)]


def seg_mask(seeds, B, Cs, p):
    """[B, H*Cs] float32: the masks of the H segments side by side (all ones for p == 0)."""
    if p == 0:
        return torch.ones(B, len(seeds) * Cs)
    return torch.cat([counter_mask(s, B, Cs, p) for s in seeds], dim=1)


def block_view(B, C, vec, fill, gen=None):
    """A [B, C] column-block view of a wider buffer (leading dimension > C), 16-byte aligned rows when ``vec``; the whole buffer too."""
    off, ld = (4, C + 8) if vec else (1, C + 3)
    buf = torch.full((B, ld), fill, dtype=torch.float32) if gen is None else torch.randn(B, ld, generator=gen)
    buf = buf.to(DEV)
    return buf[:, off:off + C], buf, off


def untouched(buf, off, C, before):
    a, b = buf.cpu(), before.cpu()
    return torch.equal(a[:, :off], b[:, :off]) and torch.equal(a[:, off + C:], b[:, off + C:])


# ------------------------------------------------------------------------------------------------ gather + input dropout
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N,F,H,B", [(50, 12, 3, 1), (50, 12, 3, 67), (300, 130, 2, 300), (70, 4, 1, 70)])
def test_gather_drop_is_bit_equal(N, F, H, B, p):
    g = torch.Generator().manual_seed(N + F + B)
    pad = 4 if F % 4 == 0 else 1
    bufs = [torch.randn(N, F + pad, generator=g).to(DEV) for _ in range(H)]
    feats = [b[:, :F] for b in bufs]                                  # padded pitch
    batch = torch.randint(0, N, (B,), generator=g)
    batch[0] = N - 1
    if B > 1:
        batch[1] = 0                                                  # N-1 before 0: not sorted
    seeds = seeds_for(H, B)
    out = ops.sign_gather_drop(feats, batch.to(DEV), p, True, seeds=seeds)
    assert out.shape == (B, H * F)
    want = torch.cat([f.cpu()[batch] for f in feats], dim=1) * seg_mask(seeds, B, F, p)
    assert torch.equal(out.cpu(), want)
    if p > 0:
        assert torch.equal(ops.sign_gather_drop(feats, batch.to(DEV), p, False), torch.cat([f[batch.to(DEV)] for f in feats], dim=1))


# ------------------------------------------------------------------------------------------------ PReLU + dropout, forward and backward
def prelu_case(B, Cs, H, p):
    g = torch.Generator().manual_seed(B * 7 + Cs + H)
    vec = Cs % 4 == 0
    C = H * Cs
    z, zbuf, off = block_view(B, C, vec, 0.0, gen=g)
    dy, _, _ = block_view(B, C, vec, 0.0, gen=g)
    z[0, 0] = 0.0
    z[-1, -1] = -0.0
    if C > 2:
        z[0, 1], z[-1, -2] = -0.0, 0.0
    slopes = [torch.tensor([SLOPES[h % 3]], device=DEV) for h in range(H)]
    seeds = seeds_for(H, B + Cs) if p > 0 else None
    return z, dy, slopes, seeds, vec


def run_fwd(z, slopes, seeds, Cs, p, vec):
    B, C = z.shape
    y, ybuf, off = block_view(B, C, vec, 7.0)
    before = ybuf.clone()
    d, keep = ops._sign_desc(B, Cs, len(slopes), p, seeds, slopes=slopes)
    _lib.check(_lib.load().egnn_prelu_drop_fwd_f32(ctypes.byref(d), _lib.ptr(z), z.stride(0), _lib.ptr(y), y.stride(0), _lib.stream()), "fwd")
    torch.cuda.synchronize()
    assert untouched(ybuf, off, C, before), "columns outside the block were written"
    return y


def run_bwd(z, dy, slopes, seeds, Cs, p, vec):
    B, C = z.shape
    H = len(slopes)
    lib = _lib.load()
    dz, dzbuf, off = block_view(B, C, vec, 7.0)
    before = dzbuf.clone()
    da, db = torch.full((H,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
    nws = lib.egnn_prelu_drop_ws_floats(B, Cs, H)
    ws = torch.empty(nws, device=DEV)
    d, keep = ops._sign_desc(B, Cs, H, p, seeds, slopes=slopes)
    _lib.check(lib.egnn_prelu_drop_bwd_f32(ctypes.byref(d), _lib.ptr(z), z.stride(0), _lib.ptr(dy), dy.stride(0), _lib.ptr(dz), dz.stride(0),
                                           _lib.ptr(da), _lib.ptr(db), _lib.ptr(ws), nws, _lib.stream()), "bwd")
    torch.cuda.synchronize()
    assert untouched(dzbuf, off, C, before), "columns outside the block were written"
    return dz.cpu().clone(), da.cpu(), db.cpu()


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B,Cs,H", [(1, 4, 1), (67, 36, 3), (257, 130, 2), (300, 512, 1), (5, 16, 16)])
def test_prelu_drop_forward_and_backward_vs_float64(B, Cs, H, p):
    z, dy, slopes, seeds, vec = prelu_case(B, Cs, H, p)
    z_before = z.clone()
    mask = seg_mask(seeds or [0] * H, B, Cs, p)
    z64, dy64, m64 = z.cpu().double(), dy.cpu().double(), mask.double()
    a64 = torch.cat([torch.full((Cs,), float(s)) for s in slopes]).double()          # the slope of every column
    pos = z64 > 0

    y = run_fwd(z, slopes, seeds, Cs, p, vec).cpu()
    assert torch.equal(z, z_before)
    y_ref = torch.where(pos, z64, a64 * z64) * m64
    np.testing.assert_allclose(y.double().numpy(), y_ref.numpy(), rtol=1e-6, atol=0)
    assert bool((y[mask == 0] == 0).all())
    assert torch.equal(run_fwd(z, slopes, seeds, Cs, p, vec).cpu(), y), "two forward runs differ"

    dz, da, db = run_bwd(z, dy, slopes, seeds, Cs, p, vec)
    dz_ref = dy64 * m64 * torch.where(pos, torch.ones_like(a64), a64)
    np.testing.assert_allclose(dz.double().numpy(), dz_ref.numpy(), rtol=1e-6, atol=0)
    assert bool((dz[mask == 0] == 0).all())
    terms = dy64 * m64 * torch.where(pos, torch.zeros_like(z64), z64)
    for h in range(H):
        t = terms[:, h * Cs:(h + 1) * Cs]
        err, bound = abs(float(da[h]) - float(t.sum())), 1e-5 * float(t.abs().sum())
        print(f"da[{h}] err {err:.3e} bound {bound:.3e}")
        assert err <= bound
    err, bound = (db.double() - dz_ref.sum(0)).abs(), 1e-5 * dz_ref.abs().sum(0)
    print(f"dbias max err {float(err.max()):.3e} min bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all())
    dz2, da2, db2 = run_bwd(z, dy, slopes, seeds, Cs, p, vec)
    assert torch.equal(dz2, dz) and torch.equal(da2, da) and torch.equal(db2, db), "two backward runs differ"


def test_seventeen_segments_is_an_argument_error_without_a_launch():
    B, Cs, H = 4, 4, 17
    z = torch.randn(B, H * Cs, device=DEV)
    y = torch.full_like(z, 7.0)
    slopes = [torch.tensor([0.25], device=DEV) for _ in range(H)]
    d, keep = ops._sign_desc(B, Cs, H, 0.0, None, slopes=slopes)
    lib = _lib.load()
    assert lib.egnn_prelu_drop_fwd_f32(ctypes.byref(d), _lib.ptr(z), z.stride(0), _lib.ptr(y), y.stride(0), _lib.stream()) == -1
    ws = torch.empty(4096, device=DEV)
    assert lib.egnn_prelu_drop_bwd_f32(ctypes.byref(d), _lib.ptr(z), z.stride(0), _lib.ptr(z), z.stride(0), _lib.ptr(y), y.stride(0),
                                       _lib.ptr(ws), _lib.ptr(ws), _lib.ptr(ws), 4096, _lib.stream()) == -1
    d, keep = ops._sign_desc(B, Cs, H, 0.0, None, srcs=[z[:, :Cs]] * H, batch=torch.arange(B, device=DEV))
    assert lib.egnn_sign_gather_drop_f32(ctypes.byref(d), _lib.ptr(y), y.stride(0), _lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "an output was written"
    with pytest.raises(_lib.HipExtensionError):
        ops.prelu_drop(z, slopes, Cs, 0.0, False)


def test_prelu_drop_autograd_matches_torch_and_tags_the_column_sums():
    B, Cs, H, p = 67, 36, 3, 0.5
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, H * Cs, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(B, H * Cs, generator=g).to(DEV)
    slopes = [torch.nn.Parameter(torch.tensor([s], device=DEV)) for s in SLOPES]
    seeds = seeds_for(H, 9)
    y = ops.prelu_drop(z, slopes, Cs, p, True, seeds=seeds)
    seen = {}
    z.register_hook(lambda gr: seen.update(tag=getattr(gr, "_egnn_colsum", None)))
    (y * w).sum().backward()
    z64 = z.detach().cpu().double().requires_grad_(True)
    s64 = [s.detach().cpu().double().requires_grad_(True) for s in slopes]
    mask = seg_mask(seeds, B, Cs, p).double()
    y64 = torch.cat([torch.nn.functional.prelu(z64[:, h * Cs:(h + 1) * Cs], s64[h]) for h in range(H)], dim=1) * mask
    (y64 * w.cpu().double()).sum().backward()
    close(y, y64, rtol=1e-6, atol_scale=1e-6)
    close(z.grad, z64.grad, rtol=1e-6, atol_scale=1e-6)
    terms = w.cpu().double() * mask * torch.where(z64 > 0, torch.zeros_like(z64), z64).detach()
    for h, (a, b) in enumerate(zip(slopes, s64)):
        assert abs(float(a.grad) - float(b.grad)) <= 1e-5 * float(terms[:, h * Cs:(h + 1) * Cs].abs().sum())
    assert seen["tag"] is not None, "dz does not carry its column sums"
    close(seen["tag"][0], z64.grad.sum(0), rtol=1e-5, atol_scale=1e-5)


# ------------------------------------------------------------------------------------------------ gemm_raw(out=view)
@pytest.mark.parametrize("Mr,N,K,width", [(67, 36, 12, 108), (300, 512, 130, 1536)])
def test_gemm_raw_writes_into_a_column_block(Mr, N, K, width):
    g = torch.Generator().manual_seed(Mr + N)
    a, w, bias = torch.randn(Mr, K, generator=g).to(DEV), torch.randn(N, K, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    ref = ops.gemm_raw(a, w, False, True, bias)
    buf = torch.full((Mr, width), 7.0, device=DEV)
    view = buf[:, N:2 * N]
    got = ops.gemm_raw(a, w, False, True, bias, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(view, ref)
    assert bool((buf[:, :N] == 7.0).all()) and bool((buf[:, 2 * N:] == 7.0).all())
    # the blocks of a wide gradient as strided operands: dW = dZ_h^T X and dX = dZ_h W
    gz = torch.randn(Mr, width, generator=g).to(DEV)
    assert torch.equal(ops.gemm_raw(gz[:, N:2 * N], a, True, False), ops.gemm_raw(gz[:, N:2 * N].contiguous(), a, True, False))
    dx = torch.full((Mr, K + 8), 7.0, device=DEV)
    ops.gemm_raw(gz[:, N:2 * N], w, False, False, out=dx[:, 4:4 + K])
    assert torch.equal(dx[:, 4:4 + K], ops.gemm_raw(gz[:, N:2 * N].contiguous(), w, False, False))
    assert bool((dx[:, :4] == 7.0).all()) and bool((dx[:, 4 + K:] == 7.0).all())
    with pytest.raises(ValueError):
        ops.gemm_raw(a, w, False, True, bias, out=buf[:, :N + 1])
    assert torch.equal(ops.linear(a, w, bias, out=view), ref)


# ------------------------------------------------------------------------------------------------ model vs goldens
class SeedFeed:
    """Stands in for ops._draw_dropout_seed: hands out the recorded sequence; a shortfall raises, ``done`` checks for a surplus."""

    def __init__(self, seeds):
        self.seeds, self.used = [int(s) for s in seeds], 0

    def __call__(self):
        assert self.used < len(self.seeds), "more seeds drawn than the reference has dropout calls"
        self.used += 1
        return self.seeds[self.used - 1]

    def done(self):
        assert self.used == len(self.seeds), f"{len(self.seeds) - self.used} recorded seeds were never drawn"


def problem(G):
    feats = [as_t(G[f"in_feat{h}"], DEV) for h in range(3)]
    return feats, as_t(G["in_labels"], DEV), [as_t(G["in_batch0"], DEV), as_t(G["in_batch1"], DEV)]


def load_into(module, G, prefix):
    module.load_state_dict({k[len(prefix):]: as_t(G[k]) for k in G.files if k.startswith(prefix)}, strict=True)
    return module.to(DEV)


def sign_model(G, prefix, L):
    return load_into(M.SIGN(12, 16, 5, 3, L, 0.5, 0.1), G, prefix)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_forward_backward_and_eval_vs_reference(G, L, monkeypatch):
    feats, labels, (b0, b1) = problem(G)
    model = sign_model(G, f"L{L}__init__", L).train()
    feed = SeedFeed(G[f"L{L}__seeds"])
    monkeypatch.setattr(ops, "_draw_dropout_seed", feed)
    logits = model.forward_rows(feats, b0)
    feed.done()
    (logits * as_t(G["in_w"], DEV)).sum().backward()
    close(logits, G[f"L{L}__logits"], rtol=1e-4, atol_scale=1e-4, msg="logits")
    close(model.out_feat, G[f"L{L}__out_feat"], rtol=1e-4, atol_scale=1e-4, msg="out_feat")
    for k, v in model.named_parameters():
        close(v.grad, G[f"L{L}__grad__{k}"], rtol=1e-4, atol_scale=1e-4, msg=f"d {k}")
    model.eval()
    with torch.no_grad():
        close(model.forward_rows(feats, b0), G[f"L{L}__eval_logits"], rtol=1e-4, atol_scale=1e-4, msg="eval logits")
        close(model([f[b0] for f in feats]), G[f"L{L}__eval_logits"], rtol=1e-4, atol_scale=1e-4, msg="eval logits, gathered")
    assert feed.used == len(feed.seeds), "eval mode drew a seed"


@pytest.mark.parametrize("tag,mode,kd_and_aux", [(f"kda_{m}", m, True) for m in M.SIGN_MODES] + [("tr_supervised", "supervised", False),
                                                                                                ("tr_nce", "nce", False)])
def test_two_adam_steps_vs_reference(G, tag, mode, kd_and_aux, monkeypatch):
    feats, labels, batches = problem(G)
    model = sign_model(G, f"{tag}__init__model.", 2)
    sp = tp = None
    if mode in ("nce", "fitnet", "gpw"):
        sp, tp = M.make_sign_projections(16, 3, 8, teacher_dim=17)
        sp, tp = load_into(sp, G, f"{tag}__init__sproj."), load_into(tp, G, f"{tag}__init__tproj.")
        opt = torch.optim.Adam([{"params": model.parameters(), "lr": LR}, {"params": sp.parameters(), "lr": LR},
                                {"params": tp.parameters(), "lr": LR}])
    else:
        opt = torch.optim.Adam(model.parameters(), lr=LR)
    feed = SeedFeed(G[f"{tag}__seeds"])
    monkeypatch.setattr(ops, "_draw_dropout_seed", feed)
    means = M.sign_train_epoch(model, feats, labels, opt, batches, mode, HP, as_t(G["in_teacher_out_feat"], DEV),
                               as_t(G["in_teacher_logits"], DEV), sp, tp, kd_and_aux=kd_and_aux)
    feed.done()
    print(tag, "means", means, "reference", G[f"{tag}__means"])
    close(np.array(means), G[f"{tag}__means"], rtol=2e-4, atol_scale=2e-4, msg="epoch means")
    for name, mod in (("model", model), ("sproj", sp), ("tproj", tp)):
        if mod is None:
            continue
        for k, v in mod.state_dict().items():
            ref = G[f"{tag}__final__{name}.{k}"]
            if not v.dtype.is_floating_point:
                assert int(v) == int(ref), (name, k)
            elif name != "model" and k == "0.bias":
                # the bias of a Linear in front of a training-mode BatchNorm: its gradient is an exactly cancelling sum (the batch mean
                # removes any constant), rounding noise on both sides, and Adam moves a parameter by up to lr per step whatever the
                # gradient's size -- after two steps the two sides may differ by 2 * 2 * lr and nothing downstream depends on the value
                assert float((v.cpu() - as_t(ref)).abs().max()) <= 4 * LR + 1e-6, (name, k)
            elif name != "model" and k == "1.running_mean":
                # the batch mean of x W^T + b contains that bias: entering step 2 the two sides' biases differ by up to 2 * lr (above),
                # and step 2 adds momentum (0.1) times its batch mean to the running mean
                err = float((v.cpu() - as_t(ref)).abs().max())
                print(f"{tag} {name}.{k}: max abs difference {err:.3e}")
                assert err <= 0.1 * 2 * LR + 2e-4 * float(np.abs(ref).max()), (name, k)
            else:
                close(v, ref, rtol=2e-4, atol_scale=2e-4, msg=f"after the steps: {name}.{k}")


def test_sign_test_vs_reference(G):
    feats, labels, _ = problem(G)
    model = sign_model(G, "kda_nce__final__model.", 2)
    loader = [torch.arange(96)[i:i + 40] for i in range(0, 96, 40)]
    logits, accs = M.sign_test(model, feats, labels, loader, as_t(G["in_train"], DEV), as_t(G["in_val"], DEV), as_t(G["in_test"], DEV))
    assert not model.training and logits.shape == (96, 5) and len(accs) == 3
    close(logits, G["test__logits"], rtol=1e-4, atol_scale=1e-4, msg="test() logits")
    np.testing.assert_allclose(np.array(accs), G["test__accs"], rtol=0, atol=1e-12)
    # device index tensors (no contiguity check on the host) take the gather-fused GEMM: same answer
    logits2, accs2 = M.sign_test(model, feats, labels, [b.to(DEV) for b in loader], as_t(G["in_train"], DEV), as_t(G["in_val"], DEV),
                                 as_t(G["in_test"], DEV))
    close(logits2, G["test__logits"], rtol=1e-4, atol_scale=1e-4, msg="test() logits, device batches")
    assert accs2 == accs


def test_forward_rows_equals_forward_of_gathered_rows_bit_for_bit(G, monkeypatch):
    feats, labels, (b0, b1) = problem(G)
    model = sign_model(G, "L2__init__", 2).train()
    seeds = G["L2__seeds"]
    outs = []
    for call in (lambda: model.forward_rows(feats, b0), lambda: model([f[b0] for f in feats])):
        feed = SeedFeed(seeds)
        monkeypatch.setattr(ops, "_draw_dropout_seed", feed)
        with torch.no_grad():
            outs.append((call().clone(), model.out_feat.clone()))
        feed.done()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    model.eval()
    with torch.no_grad():
        a = model.forward_rows(feats, range(10, 50))
        b = model([f[10:50] for f in feats])
        c = model.forward_rows(feats, torch.arange(10, 50, device=DEV))
    assert torch.equal(a, b)
    close(c, a, rtol=1e-5, atol_scale=1e-5, msg="gather-fused first GEMM vs the slice")


def test_seed_draw_order(G, monkeypatch):
    """Seeds numbered 1, 2, 3, .. in draw order reach the launches as the reference's dropout call order prescribes: input drop of
    hops 0..2; hop by hop, that hop's two hidden levels; the concatenation; project's two hidden levels."""
    feats, labels, (b0, b1) = problem(G)
    model = sign_model(G, "L3__init__", 3).train()
    feed = SeedFeed(range(1, 13))
    monkeypatch.setattr(ops, "_draw_dropout_seed", feed)
    launches = []
    orig = ops._sign_desc

    def spy(B, Cs, H, p, seeds, **kw):
        launches.append((Cs, tuple(seeds)))
        return orig(B, Cs, H, p, seeds, **kw)
    monkeypatch.setattr(ops, "_sign_desc", spy)
    with torch.no_grad():
        model.forward_rows(feats, b0)
    feed.done()
    assert launches == [(12, (1, 2, 3)), (16, (4, 6, 8)), (16, (5, 7, 9)), (48, (10,)), (16, (11,)), (16, (12,))]
    short = SeedFeed(range(1, 12))
    monkeypatch.setattr(ops, "_draw_dropout_seed", short)
    with pytest.raises(AssertionError, match="more seeds drawn"), torch.no_grad():
        model.forward_rows(feats, b0)


def test_thirty_steps_reduce_the_loss(G):
    feats, labels, batches = problem(G)
    torch.manual_seed(0)
    model = sign_model(G, "L2__init__", 2)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses = [M.sign_train_epoch(model, feats, labels, opt, batches, "supervised", HP)[0] for _ in range(15)]
    print("epoch losses", [round(v, 3) for v in losses])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())
