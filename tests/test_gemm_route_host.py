"""The GEMM route report (egnn_gemm_last_route) as far as it can be checked without a GPU: declared in the header, bound by the ctypes
table, additive (the ABI stays 9), written by gemm_impl alone, and 0 while the calling thread has launched nothing.  What each route
computes is tests/test_gpu_gemm_edges.py."""
import os
import re
import threading

from efficient_gnns_amd import _lib, build, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_route_report_and_its_encoding():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    assert re.search(r"\bint\s+egnn_gemm_last_route\s*\(\s*void\s*\)\s*;", src)
    doc = src[:src.index("int egnn_gemm_last_route")]
    doc = doc[doc.rindex("/*"):]
    for word in ("skinny_fwd_tile", "skinny_fwd", "skinny_dx", "skinny_dw", "DMA", "128x64", "128x128", "vec4", "wide_store", "split pipe",
                 "a_rows", "b_rows", "split_k"):
        assert word in doc, word
    assert "#define EGNN_ABI_VERSION 9" in src


def test_lib_binds_it_and_the_abi_is_unchanged():
    assert _lib.SIGNATURES["egnn_gemm_last_route"] == (_lib._i32, [])
    lib = _lib.load()
    assert lib.egnn_abi_version() == 9
    assert isinstance(ops.gemm_last_route(), int)


def test_one_writer_in_gemm_impl():
    """The dispatch predicates exist once: the route is stored where gemm_impl commits to a kernel, not derived by a second function."""
    text = open(os.path.join(build.CSRC, "gemm.hip")).read()
    impl = text[text.index("static int gemm_impl("):text.index('extern "C" int egnn_gemm_last_route')]
    assert len(re.findall(r"\bg_last_route\s*=", impl)) == 4                  # reset, skinny, DMA, general
    assert len(re.findall(r"\bg_last_route\s*=", text)) == 5                  # ... and the definition
    assert "thread_local int g_last_route = 0;" in text
    for other in ("gemm_skinny.hip", "fused_bn.hip", "gemm_core.h", "gemm_split.h", "gemm3.h"):
        assert "g_last_route" not in open(os.path.join(build.CSRC, other)).read()


def test_route_is_zero_before_any_call_and_after_an_empty_call():
    lib = _lib.load()
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.egnn_gemm_last_route()))    # a thread that never called a GEMM
    t.start()
    t.join()
    assert seen == [0]
    # M == 0 returns before any pointer is looked at or any GPU work is issued
    assert lib.egnn_gemm_f32(0, 0, 0, 8, 8, 1.0, None, 8, None, 8, None, None, 8, 1, None, 0, None) == 0
    assert lib.egnn_gemm_last_route() == 0
    # an argument error (null operands with a non-empty output) is refused before the dispatch as well
    assert lib.egnn_gemm_f32(0, 0, 4, 8, 8, 1.0, None, 8, None, 8, None, None, 8, 1, None, 0, None) == -1
    assert ops.gemm_last_route() == 0
