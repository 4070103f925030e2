"""Weighted adjacency, host side (no GPU): the new C entry points are declared, bound and exported; a CPU tensor is refused with the
package's own error, not with the "not offered" one the weighted calls raised before."""
import ctypes
import os
import re

import pytest
import torch

import efficient_gnns_amd as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("egnn_sddmm_csr_f32", "egnn_gcn_norm_fill_val_i64", "egnn_gcn_norm_scale_i64")


def test_new_symbols_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(egnn_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(E._lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/egnn_hip.h"
        assert s in E._lib.SIGNATURES, f"{s} is not in _lib.SIGNATURES"
        assert hasattr(lib, s), f"{s} is not exported by the built library"
    assert "sddmm.hip" in open(os.path.join(ROOT, "efficient-gnns_amd", "build.py")).read()


def test_abi_version_is_still_9():
    assert E._lib.load().egnn_abi_version() == 9


def test_sddmm_argument_checks_need_no_gpu():
    """The entry point's argument checks run on the host before any launch: nnz == 0 is a no-op, bad widths / pitches are EGNN_EINVAL."""
    f = E._lib.load().egnn_sddmm_csr_f32
    assert f(3, 3, 8, None, None, 32, 0, None, 8, None, 8, None, None, None, None) == 0      # nnz == 0: launches nothing
    assert f(3, 3, 8, None, None, 16, 0, None, 8, None, 8, None, None, None, None) != 0      # index_bits
    assert f(3, 3, 8, None, None, 32, 0, None, 4, None, 8, None, None, None, None) != 0      # ldg < K
    assert f(3, 3, 8, None, None, 32, 5, None, 8, None, 8, None, None, None, None) != 0      # entries without arrays


def test_weighted_calls_on_cpu_tensors_raise_the_no_fallback_error():
    x = torch.randn(3, 4)
    edge_index = torch.tensor([[0, 1, 2, 1], [1, 0, 1, 1]])
    w = torch.tensor([0.5, 0.25, 2.0, 0.3])
    with pytest.raises(E._lib.HipExtensionError):
        E.GCNConv(4, 4)(x, edge_index, w)
    adj = E.SparseTensor(row=edge_index[1], col=edge_index[0], value=w, sparse_sizes=(3, 3))
    with pytest.raises(E._lib.HipExtensionError):
        E.sparse.gcn_norm(adj)
    with pytest.raises(E._lib.HipExtensionError):
        E.GCNConv(4, 4)(x, adj)
    with pytest.raises(E._lib.HipExtensionError):
        adj.set_value(w.clone().requires_grad_(True)).matmul(x, "sum")


def test_what_stays_out_says_so():
    adj = E.SparseTensor(row=torch.tensor([0, 1]), col=torch.tensor([1, 0]), value=torch.tensor([0.5, 2.0]), sparse_sizes=(2, 2))
    with pytest.raises(NotImplementedError):
        adj.to_symmetric()

    class Shard:   # stands for dist.ShardedAdj: GCNConv recognises a shard by this method
        def gcn_normalized(self):
            raise AssertionError("must not be reached with edge_weight")

    with pytest.raises(NotImplementedError, match="shard"):
        E.GCNConv(4, 4)(torch.randn(2, 4), Shard(), torch.tensor([1.0, 1.0]))
