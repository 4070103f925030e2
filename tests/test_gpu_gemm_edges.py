"""Every route of the dense GEMM dispatcher (csrc/gemm.hip::gemm_impl) at its thresholds, against a float64 product.

Each case names the kernel it means to run -- egnn_gemm_last_route, include/egnn_hip.h -- so a threshold that drifts fails here instead
of quietly testing another kernel.  Operands are views inside NaN-filled buffers (rows before and after, pitch padding), the output is a
view inside a buffer filled with a sentinel bit pattern: a kernel that lets padding reach a result or stores outside its view is seen.

Error unit: |alpha| * sum_k |a_k b_k| + |bias| + |addend|; bar: max < 2e-6 in that unit (the bar of
test_split_pipeline_error_is_not_above_the_f32_mfma_pipeline).  torch's float32 CPU product of the same inputs must be inside the same
bar, which shows that the inputs do not put fp32 rounding itself above it.

Run as a script the module runs groups of cases in the process it is started in:
    python tests/test_gpu_gemm_edges.py --groups a,b,c,d           one RESULT line (failures, routes): the EGNN_GEMM_PIPE=f32 child
    python tests/test_gpu_gemm_edges.py --report FILE              worst error per route -> FILE (profiles/gemm_edge_errors.txt)
    python tests/test_gpu_gemm_edges.py --cpu-check                the float32 CPU figure of every case, no GPU
"""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import efficient_gnns_amd.ops as ops   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-6
SENTINEL = 0x7FA5C3D2            # a NaN bit pattern no kernel produces
SPLIT_PIPE = not os.environ.get("EGNN_GEMM_PIPE", "").startswith("f")
LAYOUTS = {"NN": (False, False), "NT": (False, True), "TN": (True, False), "TT": (True, True)}
FORMS = {1: "skinny_fwd_tile", 2: "skinny_fwd", 3: "skinny_dx", 4: "skinny_dw narrow=A", 5: "skinny_dw narrow=B", 6: "DMA",
         7: "general 128x64", 8: "general 128x128"}
# operand / output views: "al" 16-byte aligned rows behind a padded pitch, "off" the same pitch with the base one float further,
# "odd" an odd pitch (rows change their alignment); all with two rows of padding before and after
KINDS = ("al", "off", "odd")


def route(form, vec4=0, wide=0, ga=0, gb=0, split=1):
    """The route word the library must report (include/egnn_hip.h).  Skinny forms (1-5) report the form alone; only the 128x128 tile and
    the DMA form run on the split pipe."""
    if form <= 5:
        return form
    pipe = 1 if (form == 6 or (form == 8 and SPLIT_PIPE)) else 0
    return form | vec4 << 8 | wide << 9 | pipe << 10 | ga << 11 | gb << 12 | split << 16


def describe(r):
    bits = [n for b, n in ((8, "vec4"), (9, "wide"), (10, "split-pipe"), (11, "gatherA"), (12, "gatherB")) if r >> b & 1]
    return f"{FORMS.get(r & 255, r & 255)} [{' '.join(bits)}] split_k={r >> 16}"


def _pitch(cols, kind):
    p = (cols + 3) // 4 * 4 + 4
    return p + 1 if kind == "odd" else p


def _view(buf, rows, cols, kind):
    pitch = _pitch(cols, kind)
    return buf.as_strided((rows, cols), (pitch, 1), 2 * pitch + (1 if kind == "off" else 0) + (2 if kind == "odd" else 0))


def operand(values, kind, fill=float("nan")):
    """``values`` [rows, cols] as a device view of kind ``kind`` inside a buffer filled with ``fill``."""
    rows, cols = values.shape
    buf = torch.full(((rows + 4) * _pitch(cols, kind) + 8,), fill, dtype=torch.float32, device=DEV)
    v = _view(buf, rows, cols, kind)
    v.copy_(values)
    assert (v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0) == (kind == "al")
    return v


def out_view(rows, cols, kind):
    n = (rows + 4) * _pitch(cols, kind) + 8
    buf = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    inside = torch.zeros(n, dtype=torch.bool, device=DEV)
    _view(inside, rows, cols, kind).fill_(True)
    return buf, _view(buf.view(torch.float32), rows, cols, kind), inside


def rand(g, *shape):
    return torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-3, 4, shape, generator=g).float())


def case(name, lay, M, N, K, expect, ak="al", bk="al", ok="al", bias=True, alpha=1.0, relu=False, addend=None, split_k=None,
         a_ids=None, b_ids=None, storage_rows=0):
    """One call: shape, layout, view kinds of A / B / out (``addend``: the view kind of an [M, N] addend or None), and the route it must
    report.  a_ids / b_ids: row ids of a fused gather out of ``storage_rows`` rows."""
    return dict(name=name, lay=lay, M=M, N=N, K=K, expect=expect, ak=ak, bk=bk, ok=ok, bias=bias, alpha=alpha, relu=relu, addend=addend,
                split_k=split_k, a_ids=a_ids, b_ids=b_ids, storage_rows=storage_rows)


def prepare(c, seed):
    """CPU side of a case: inputs, the float64 reference, the error unit, and the float32 CPU product's error in that unit."""
    g = torch.Generator().manual_seed(seed)
    ta, tb = LAYOUTS[c["lay"]]
    M, N, K = c["M"], c["N"], c["K"]
    a_sto = rand(g, *((c["storage_rows"], K) if c["a_ids"] is not None else ((K, M) if ta else (M, K))))
    b_sto = rand(g, *((c["storage_rows"], N) if c["b_ids"] is not None else ((N, K) if tb else (K, N))))
    a = a_sto[c["a_ids"]] if c["a_ids"] is not None else (a_sto.t() if ta else a_sto)
    b = b_sto[c["b_ids"]] if c["b_ids"] is not None else (b_sto.t() if tb else b_sto)
    bias = rand(g, N) if c["bias"] else None
    addend = rand(g, M, N) if c["addend"] else None
    alpha = c["alpha"]
    ref = alpha * (a.double() @ b.double())
    unit = abs(alpha) * (a.double().abs() @ b.double().abs())
    r32 = alpha * (a.contiguous() @ b.contiguous())
    for t in (bias, addend):
        if t is not None:
            ref, unit, r32 = ref + t.double(), unit + t.double().abs(), r32 + t
    if c["relu"]:
        ref, r32 = ref.clamp(min=0), r32.clamp(min=0)
    err32 = float(((r32.double() - ref).abs() / unit).max())
    assert err32 < BAR, f"{c['name']}: the float32 CPU product is {err32:.3g} units off: the inputs themselves are above the bar"
    return dict(a_sto=a_sto, b_sto=b_sto, bias=bias, addend=addend, ref=ref, unit=unit, err32=err32)


def run_case(c, seed=0):
    """Runs one case on the device and asserts route, finiteness, untouched surroundings, bit-stability and the error bar.
    Returns (route, error, float32-CPU error)."""
    p = prepare(c, seed)
    ta, tb = LAYOUTS[c["lay"]]
    M, N = c["M"], c["N"]
    a_sto, b_sto = p["a_sto"], p["b_sto"]
    for sto, ids in ((a_sto, c["a_ids"]), (b_sto, c["b_ids"])):
        if ids is not None:                       # rows no id names are NaN: a gather that reads another row is seen
            named = torch.zeros(sto.shape[0], dtype=torch.bool)
            named[ids] = True
            sto[~named] = float("nan")
    a, b = operand(a_sto, c["ak"]), operand(b_sto, c["bk"])
    bias = None if p["bias"] is None else operand(p["bias"][None, :], "off")[0]
    addend = None if p["addend"] is None else operand(p["addend"], c["addend"])
    buf, out, inside = out_view(M, N, c["ok"])
    kw = dict(bias=bias, alpha=c["alpha"], split_k=c["split_k"], relu=c["relu"], addend=addend, out=out,
              a_rows=None if c["a_ids"] is None else c["a_ids"].to(DEV), b_rows=None if c["b_ids"] is None else c["b_ids"].to(DEV))
    y = ops.gemm_raw(a, b, ta, tb, **kw)
    got = ops.gemm_last_route()
    assert y is out
    assert got == c["expect"], f"route {got:#x} = {describe(got)}; expected {c['expect']:#x} = {describe(c['expect'])}"
    first = out.clone()
    assert bool(torch.isfinite(first).all()), "non-finite result: padding reached it, or an element was never stored"
    assert bool((buf[~inside] == SENTINEL).all()), "the kernel stored outside its output view"
    ops.gemm_raw(a, b, ta, tb, **kw)
    assert ops.gemm_last_route() == got
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), "two calls differ in their bits"
    assert bool((buf[~inside] == SENTINEL).all())
    err = float(((first.cpu().double() - p["ref"]).abs() / p["unit"]).max())
    print(f"{c['name']}: {describe(got)}  err {err:.3g}  f32-cpu {p['err32']:.3g}")
    assert err < BAR, f"error {err:.3g} units (float32 CPU product: {p['err32']:.3g}); bar {BAR:g}"
    return got, err, p["err32"]


def run_all(cases, worst=None, routes=None):
    """Every case (none is skipped after a failure); returns the failures as 'name: message' lines."""
    failures = []
    for i, c in enumerate(cases):
        try:
            r, err, err32 = run_case(c, seed=1000 + i)
        except AssertionError as e:
            failures.append(f"{c['name']}: {str(e).splitlines()[0] if str(e) else 'assert'}")
            continue
        if routes is not None:
            routes.append(r)
        if worst is not None:
            w = worst.setdefault(r & 0x1FFF, [0.0, 0.0, 0])
            w[0], w[1], w[2] = max(w[0], err), max(w[1], err32), w[2] + 1
    return failures


def _vec4(ak, bk):
    return int(ak == "al" and bk == "al")


# ---- a. general kernels: k-ladder x tile edges ----------------------------------------------------------------------------------------
def cases_a(lay):
    """nk = ceil(K / 16) k-steps of the ring (depth 4, unrolled by 4): 1 ragged, 1 full, 2, 3, 4 (one unrolled group), 4 + ragged, 5,
    9; on one element, inside one tile, one short of / exactly / one past the 128 edge.  The view kinds rotate with the case so that
    the 16-byte and the 4-byte operand loads and both stores meet every K."""
    out, i = [], 0
    for (M, N) in ((1, 1), (33, 65), (127, 129), (128, 128), (129, 64)):
        for K in (1, 15, 16, 17, 48, 64, 79, 80, 144):
            ak, bk, ok = KINDS[i % 3], KINDS[(i // 3) % 3] if i % 2 else "al", KINDS[(i // 2) % 3]
            i += 1
            out.append(case(f"a {lay} {M}x{N}x{K} A={ak} B={bk} C={ok}", lay, M, N, K,
                            route(7 if N <= 64 else 8, _vec4(ak, bk), int(ok == "al")), ak, bk, ok, alpha=0.5))
    return out


@pytest.mark.parametrize("lay", list(LAYOUTS))
def test_general_k_ladder_at_tile_edges(lay):
    failures = run_all(cases_a(lay))
    assert not failures, "\n".join(failures)


# ---- b. vec4 x wide_store ---------------------------------------------------------------------------------------------------------------
def cases_b():
    out = []
    for lay in ("NN", "NT", "TN"):
        for (M, N, K) in ((129, 68, 40), (130, 256, 32), (129, 40, 48)):
            form = 7 if N <= 64 else 8
            for ak in KINDS:
                for ok in KINDS:
                    bk = "al" if ak != "odd" else "off"
                    out.append(case(f"b {lay} {M}x{N}x{K} A={ak} B={bk} C={ok}", lay, M, N, K,
                                    route(form, _vec4(ak, bk), int(ok == "al")), ak, bk, ok))
                out.append(case(f"b {lay} {M}x{N}x{K} A=al B={ak} C=al", lay, M, N, K, route(form, _vec4("al", ak), 1), "al", ak, "al"))
            for ok, adk in (("al", "al"), ("al", "off"), ("al", "odd"), ("off", "al"), ("odd", "al")):   # the wide store needs both
                wide = int(ok == "al" and adk == "al")
                out.append(case(f"b {lay} {M}x{N}x{K} addend={adk} C={ok}", lay, M, N, K, route(form, 1, wide), ok=ok, addend=adk))
                out.append(case(f"b {lay} {M}x{N}x{K} relu C={ok}", lay, M, N, K, route(form, 1, int(ok == "al")), ok=ok, relu=True))
    return out


def test_vec4_and_wide_store_combinations():
    failures = run_all(cases_b())
    assert not failures, "\n".join(failures)


# ---- c. split-K -------------------------------------------------------------------------------------------------------------------------
def cases_c():
    """k_per_split = ceil(ksteps / split_k) * 16.  K = 160 (10 steps): split_k 7 -> 32 per range, ranges 5 and 6 start at or past K and
    are empty; 10 -> one step each; 64 -> clamped to 10.  K = 167 (11 steps): 7 -> range 5 is the ragged 7, range 6 is empty; 64 ->
    clamped to 11, the last range ragged.  The partial store is wide when N % 4 == 0; bias, ReLU and addend belong to the reduce."""
    out = []
    for lay in ("TN", "NN"):
        for (M, N) in ((70, 36), (70, 38), (129, 130)):
            for K, sk, eff in ((160, 7, 7), (160, 10, 10), (160, 64, 10), (167, 7, 7), (167, 64, 11)):
                exp = route(7 if N <= 64 else 8, 1, int(N % 4 == 0), split=eff)
                nm = f"c {lay} {M}x{N}x{K} split_k={sk}"
                out.append(case(nm + " bias", lay, M, N, K, exp, split_k=sk, alpha=0.5))
                out.append(case(nm + " bias relu", lay, M, N, K, exp, split_k=sk, relu=True))
                out.append(case(nm + " addend(odd pitch)", lay, M, N, K, exp, split_k=sk, bias=False, addend="odd"))
                out.append(case(nm + " bias C=odd", lay, M, N, K, exp, split_k=sk, ok="odd"))
                out.append(case(nm + " A=off", lay, M, N, K, exp & ~(1 << 8), ak="off", split_k=sk, bias=False, ok="off"))
    return out


def test_split_k_empty_ranges_clamp_and_reduce_epilogue():
    failures = run_all(cases_c())
    assert not failures, "\n".join(failures)


# ---- d. fused gathers -------------------------------------------------------------------------------------------------------------------
def id_sets(m):
    return {"reversed": 299 - torch.arange(m), "all-0": torch.zeros(m, dtype=torch.int64), "all-299": torch.full((m,), 299),
            "pairs": (7 + torch.arange((m + 1) // 2)).repeat_interleave(2)[:m]}


def cases_d():
    out = []
    for m in (1, 127, 129):
        for idn, ids in id_sets(m).items():
            for kind in ("al", "odd"):
                for lay in ("NN", "NT"):          # a_rows: op(A) = A[ids], m output rows on either side of the 128-row tile edge
                    for (K, N) in ((40, 70), (16, 40)):
                        out.append(case(f"d a_rows {lay} m={m} {idn} K={K} N={N} A={kind}", lay, m, N, K,
                                        route(7 if N <= 64 else 8, int(kind == "al"), 1, ga=1), ak=kind, a_ids=ids, storage_rows=300))
                for lay in ("NN", "TN"):          # b_rows: B = B[ids], m gathered k-rows (m = 127 / 129: a ragged last k-step)
                    for (M, N) in ((70, 130), (33, 40)):
                        out.append(case(f"d b_rows {lay} k={m} {idn} M={M} N={N} B={kind}", lay, M, N, m,
                                        route(7 if N <= 64 else 8, int(kind == "al"), 1, gb=1), bk=kind, b_ids=ids, storage_rows=300))
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 300, (200,), generator=g)     # repeats; 13 k-steps in ranges of 5, 5 and 3 (the last one ragged)
    for lay in ("NN", "TN"):
        for (M, N) in ((70, 130), (129, 36)):
            for kind in ("al", "odd"):
                out.append(case(f"d b_rows {lay} k=200 split_k=3 M={M} N={N} B={kind}", lay, M, N, 200,
                                route(7 if N <= 64 else 8, int(kind == "al"), int(N % 4 == 0), gb=1, split=3), bk=kind, b_ids=ids,
                                storage_rows=300, split_k=3))
    return out


def test_fused_gathers_repeated_ids_and_storage_edges():
    failures = run_all(cases_d())
    assert not failures, "\n".join(failures)


# ---- e. DMA form thresholds ---------------------------------------------------------------------------------------------------------------
def cases_e():
    """Taken: M >= 4096, N a multiple of 128 up to 1024, K a multiple of 32 in 64 .. 4096, A rows 16-byte aligned, no split-K.  All with a
    bias: without one, K <= 64 would be the skinny dx form.  (EGNN_GEMM_PIPE=f32 has no DMA form: the general kernel then.)"""
    out = []
    dma = lambda wide=1, vec4=1: route(6, 0, wide) if SPLIT_PIPE else route(8, vec4, wide)
    for lay in ("NN", "NT"):
        out.append(case(f"e {lay} 4096x128x64", lay, 4096, 128, 64, dma()))
        out.append(case(f"e {lay} 4097x128x96", lay, 4097, 128, 96, dma(), alpha=0.5))
    out.append(case("e NT 4096x1024x64", "NT", 4096, 1024, 64, dma()))
    out.append(case("e NT 4096x128x4096 split_k=1", "NT", 4096, 128, 4096, dma(), split_k=1))
    out.append(case("e NN 4097x256x64 B=off (B is cut into planes: any alignment)", "NN", 4097, 256, 64, dma(1, 0), bk="off"))
    out.append(case("e NT 4097x128x96 relu", "NT", 4097, 128, 96, dma(), relu=True))
    out.append(case("e NT 4097x128x96 addend", "NT", 4097, 128, 96, dma(), addend="al"))
    out.append(case("e NT 4097x128x96 addend=odd (narrow store)", "NT", 4097, 128, 96, dma(0), addend="odd"))
    out.append(case("e NT 4097x128x96 C=off (narrow store)", "NT", 4097, 128, 96, dma(0), ok="off"))
    out.append(case("e NT 4097x128x96 C=odd (narrow store)", "NT", 4097, 128, 96, dma(0), ok="odd"))
    gen = lambda vec4=1: route(8, vec4, 1)
    out.append(case("e not taken: M=4095", "NT", 4095, 128, 64, gen()))
    out.append(case("e not taken: K=32", "NT", 4096, 128, 32, gen()))
    out.append(case("e not taken: K=80", "NT", 4096, 128, 80, gen()))
    out.append(case("e not taken: N=192", "NT", 4096, 192, 64, gen()))
    out.append(case("e not taken: N=1152", "NT", 4096, 1152, 64, gen()))
    out.append(case("e not taken: K=4128", "NT", 4096, 128, 4128, gen(), split_k=1))
    out.append(case("e not taken: A=off", "NT", 4096, 128, 64, gen(0), ak="off"))
    out.append(case("e not taken: split_k=2", "NT", 4096, 128, 64, route(8, 1, 1, split=2), split_k=2))
    return out


def test_dma_form_thresholds():
    failures = run_all(cases_e())
    assert not failures, "\n".join(failures)


# ---- f. skinny forward ------------------------------------------------------------------------------------------------------------------
def cases_f():
    """N <= 64 classes, M >= 4096 rows, K a multiple of 16 up to 1024.  K = 256 is the LDS-tile form (1), the others skinny_fwd (2) while
    W's LDS image K * (16 ceil(N / 16) + 4) * 4 B fits 160 KB - 2 KB: N = 64 up to K = 592; above 64 KB (N = 64, K = 272; N = 12,
    K = 1024) the kernel needs its dynamic-LDS attribute.  4097 rows leave the last workgroup a single row."""
    out = []
    gen = lambda N, vec4=1, wide=1: route(7 if N <= 64 else 8, vec4, wide)
    for lay in ("NN", "NT"):
        f = lambda nm, M, N, K, exp, **kw: out.append(case(f"f {lay} {M}x{N}x{K} {nm}", lay, M, N, K, exp, **kw))
        f("M below", 4095, 40, 32, gen(40), alpha=0.5)
        f("M at", 4096, 40, 32, 2, alpha=0.5)
        f("M past", 4097, 40, 32, 2, alpha=0.5, bias=False)
        for N in (1, 16, 17, 32, 33, 64):
            f("classes", 4097, N, 32, 2, bias=N % 2 == 0, ok=KINDS[N % 3], bk=KINDS[(N // 16) % 3])
        f("tile form", 4097, 40, 256, 1, alpha=0.5)
        f("tile form no bias C=odd W=off", 4096, 17, 256, 1, bias=False, ok="odd", bk="off")
        f("tile form 64 classes", 4097, 64, 256, 1)
        f("K=240", 4097, 40, 240, 2, alpha=0.5)
        f("64 classes, LDS image > 64 KB", 4097, 64, 272, 2)
        f("12 classes, LDS image > 64 KB", 4096, 12, 1024, 2, alpha=0.5)
        f("largest image that fits", 4097, 64, 592, 2)
        f("image too large", 4097, 64, 608, gen(64))
        f("K above 1024", 4097, 12, 1040, gen(12), alpha=0.5)
        f("K=16", 4097, 40, 16, 2)
        f("W=off", 4097, 40, 48, 2, bk="off")
        f("W=odd", 4097, 40, 48, 2, bk="odd", bias=False)
        f("X=off", 4097, 40, 48, gen(40, 0), ak="off")
        f("X=odd", 4097, 40, 48, gen(40, 0, 0), ak="odd", ok="off")
        f("X=off tile shape", 4097, 40, 256, gen(40, 0), ak="off")
    return out


def test_skinny_forward_forms_and_lds_budget():
    failures = run_all(cases_f())
    assert not failures, "\n".join(failures)


# ---- g. skinny dx -----------------------------------------------------------------------------------------------------------------------
def cases_g():
    """dX = G [M, Ks] x B: Ks <= 64, Nbig a multiple of 64 up to 1024, M >= 4096, no bias, 16-byte output rows.  The k-step template
    instances: Ks <= 16 -> 4, <= 32 -> 8, <= 40 -> 10, <= 48 -> 12, else 16.  With Nbig = 64 and Ks in {16, 32, 64} the shape is a skinny
    FORWARD first (N <= 64, K % 16 == 0): form 2; those Ks reach the dx kernel at Nbig = 128."""
    out = []
    for lay in ("NN", "NT"):
        f = lambda nm, M, N, K, exp, **kw: out.append(case(f"g {lay} {M}x{N}x{K} {nm}", lay, M, N, K, exp, **{"bias": False, **kw}))
        for M in (4096, 4097, 4351):
            f("rows", M, 64, 40, 3, alpha=0.5)
        for Ks in (1, 4, 16, 17, 32, 33, 40, 41, 49, 64):
            f("k-steps", 4097, 64, Ks, 2 if Ks % 16 == 0 else 3)
            f("k-steps", 4097, 128, Ks, 3, alpha=0.5)
        f("Ks above 64", 4097, 64, 65, route(7, 1, 1))
        f("widest", 4096, 1024, 17, 3)
        f("Nbig=96", 4097, 96, 40, route(8, 1, 1))
        f("Nbig=1088", 4096, 1088, 40, route(8, 1, 1))
        f("bias", 4097, 128, 40, route(8, 1, 1), bias=True)
        f("C=off", 4097, 128, 40, route(8, 1, 0), ok="off")
        f("C=odd", 4097, 128, 40, route(8, 1, 0), ok="odd")
        f("G=off", 4097, 128, 40, 3, ak="off")
        f("G=odd", 4351, 128, 33, 3, ak="odd")
        if lay == "NN":
            f("B=off (16-byte loads of B)", 4097, 128, 40, route(8, 0, 1), bk="off")
            f("B=odd (16-byte loads of B)", 4097, 128, 40, route(8, 0, 1), bk="odd")
        else:
            f("B=off (k-major: 4-byte loads)", 4097, 128, 40, 3, bk="off")
            f("B=odd (k-major: 4-byte loads)", 4097, 128, 40, 3, bk="odd")
    return out


def test_skinny_dx_k_step_instances_and_fallbacks():
    failures = run_all(cases_g())
    assert not failures, "\n".join(failures)


# ---- h. skinny dw -----------------------------------------------------------------------------------------------------------------------
def cases_h():
    """dW = S^T Bg over R >= 4096 rows (layout TN, no bias): form 4 when the narrow matrix (Ns <= 64 columns) is A, form 5 when it is B --
    stored through strides (1, ldc).  Ns = Nb = 64 satisfies both and is form 4.  R = 4097 / 5121: a last wave / workgroup with one row.
    R >= 4096 makes gemm_raw ask for split-K; the skinny forms do not split."""
    out = []

    def both(nm, R, Ns, Nb, **kw):
        out.append(case(f"h narrow=A R={R} Ns={Ns} Nb={Nb} {nm}", "TN", Ns, Nb, R, 4, bias=False, **kw))
        out.append(case(f"h narrow=B R={R} Ns={Ns} Nb={Nb} {nm}", "TN", Nb, Ns, R, 4 if Ns == 64 and Nb == 64 else 5, bias=False, **kw))
    for i, Ns in enumerate((1, 16, 17, 32, 33, 64)):
        for Nb in (64, 320):
            both("", 4097, Ns, Nb, alpha=0.5, ok=KINDS[(i + Nb // 320) % 3])
    for R in (4096, 5121):
        both("rows", R, 17, 64, alpha=0.5)
        both("rows", R, 64, 320, ok="odd")
    out.append(case("h narrow=A S=odd", "TN", 40, 64, 4097, 4, bias=False, ak="odd"))
    out.append(case("h narrow=B S=off", "TN", 64, 40, 4097, 5, bias=False, bk="off"))
    # below the row threshold, and a wide matrix without 16-byte rows: the general kernel (K < 4096: no split-K from gemm_raw)
    out.append(case("h R=4095 narrow=A", "TN", 40, 320, 4095, route(8, 1, 1), bias=False))
    out.append(case("h R=4095 narrow=B", "TN", 320, 40, 4095, route(7, 1, 1), bias=False))
    out.append(case("h wide matrix off", "TN", 40, 64, 4097, route(7, 0, 1), bias=False, bk="off", split_k=1))
    out.append(case("h bias", "TN", 40, 64, 4097, route(7, 1, 1), bias=True, split_k=1))
    return out


def test_skinny_dw_both_orientations():
    failures = run_all(cases_h())
    assert not failures, "\n".join(failures)


# ---- i. the f32-input MFMA pipe ------------------------------------------------------------------------------------------------------------
GROUPS = {"a": lambda: [c for lay in LAYOUTS for c in cases_a(lay)], "b": cases_b, "c": cases_c, "d": cases_d, "e": cases_e, "f": cases_f,
          "g": cases_g, "h": cases_h}


def test_cases_a_to_d_on_the_f32_pipe():
    """EGNN_GEMM_PIPE is read once per process: the general kernels' f32-input pipeline (csrc/gemm_core.h) runs cases a to d in one
    fresh child; no route may carry the split-pipe bit."""
    env = dict(os.environ, EGNN_GEMM_PIPE="f32")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--groups", "a,b,c,d"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["failures"] == [], "\n".join(res["failures"])
    assert res["cases"] == len(res["routes"]) == sum(len(GROUPS[k]()) for k in "abcd")
    assert all(r & 255 in (7, 8) and not r >> 10 & 1 for r in res["routes"])


def main(argv):
    if "--cpu-check" in argv:
        worst = 0.0
        for name, fn in GROUPS.items():
            cs = fn()
            errs = [prepare(c, 1000 + i)["err32"] for i, c in enumerate(cs)]
            worst = max(worst, max(errs))
            print(f"group {name}: {len(cs)} cases, float32 CPU product at most {max(errs):.3g} units (bar {BAR:g})")
        return 0 if worst < BAR else 1
    names = argv[argv.index("--groups") + 1].split(",") if "--groups" in argv else list(GROUPS)
    worst, routes, failures, n = {}, [], [], 0
    for name in names:
        cs = GROUPS[name]()
        n += len(cs)
        failures += run_all(cs, worst, routes)
    if "--report" in argv:
        with open(argv[argv.index("--report") + 1], "w") as fh:
            fh.write("# worst error per GEMM route over the cases of tests/test_gpu_gemm_edges.py (groups %s; pipe: %s)\n"
                     "# unit: |alpha| sum_k |a_k b_k| + |bias| + |addend|; bar %g; f32-cpu = torch's float32 CPU product of the same inputs\n"
                     "# route   cases   worst-err   worst-f32-cpu   what\n" % (",".join(names), "split" if SPLIT_PIPE else "f32", BAR))
            for r in sorted(worst):
                e, e32, k = worst[r]
                fh.write(f"{r:#06x}  {k:5d}   {e:.3e}   {e32:.3e}   {describe(r).rsplit(' split_k', 1)[0]}\n")
            for line in failures:
                fh.write("# FAILED " + line + "\n")
    print("RESULT " + json.dumps({"cases": n, "failures": failures, "routes": routes}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
