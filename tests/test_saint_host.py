"""CPU-side checks of the MAG mini-batch layer: ``utils.group_hetero_graph`` / ``to_undirected`` known answers, the golden toy's
grouping, the C ABI of csrc/saint.hip (declared, exported, bound, argument errors before any launch), ``data.mag_hetero_like`` and
the drop-in names of /root/reference/mag_pyg/gnn.py:14-16."""
import ctypes
import os
import re
import sys

import pytest
import torch

import efficient_gnns_amd.data as D
import efficient_gnns_amd.utils as U
from efficient_gnns_amd import _lib
from conftest import ROOT, mag_rgcn_case

SAINT_SYMBOLS = ("egnn_saint_induced_geometry", "egnn_saint_random_walk_i64", "egnn_saint_scan_ws_bytes", "egnn_saint_select_i64",
                 "egnn_saint_induced_count_i64", "egnn_saint_induced_fill_i64", "egnn_saint_gather_i64")


def test_group_hetero_graph_known_answer():
    """3 node types / 3 relations by hand: one relation is empty and node type 'c' appears in no edge."""
    eid = {("a", "r0", "b"): torch.tensor([[0, 2, 1], [1, 0, 1]]),
           ("b", "r1", "a"): torch.zeros((2, 0), dtype=torch.int64),
           ("d", "r2", "a"): torch.tensor([[1, 0], [2, 2]])}
    sizes = {"a": 3, "b": 2, "c": 4, "d": 2}
    ei, et, nt, li, l2g, k2i = U.group_hetero_graph(eid, sizes)
    # offsets: a 0, b 3, c 5, d 9
    assert torch.equal(ei, torch.tensor([[0, 2, 1, 10, 9], [4, 3, 4, 2, 2]]))
    assert torch.equal(et, torch.tensor([0, 0, 0, 2, 2]))
    assert torch.equal(nt, torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3]))
    assert torch.equal(li, torch.tensor([0, 1, 2, 0, 1, 0, 1, 2, 3, 0, 1]))
    assert k2i == {"a": 0, "b": 1, "c": 2, "d": 3, ("a", "r0", "b"): 0, ("b", "r1", "a"): 1, ("d", "r2", "a"): 2}
    assert set(l2g) == {"a", "b", "c", "d", 0, 1, 2, 3}
    assert torch.equal(l2g["c"], torch.tensor([5, 6, 7, 8])) and torch.equal(l2g[2], l2g["c"]) and torch.equal(l2g["d"], torch.tensor([9, 10]))
    for v in (ei, et, nt, li):
        assert v.dtype == torch.int64


def test_to_undirected_known_answer():
    ei = torch.tensor([[3, 0, 1, 1, 2, 0], [0, 3, 2, 2, 2, 1]])     # a reversed pair, a duplicate, a self loop
    assert torch.equal(U.to_undirected(ei), torch.tensor([[0, 0, 1, 1, 2, 2, 3], [1, 3, 0, 2, 1, 2, 0]]))
    assert torch.equal(U.to_undirected(ei, num_nodes=6), U.to_undirected(ei))
    assert U.to_undirected(torch.zeros((2, 0), dtype=torch.int64)).shape == (2, 0)


def test_group_hetero_graph_reproduces_the_golden_toy(golden_mag_rgcn):
    """tests/golden/mag_rgcn.npz was grouped the canonical way (node types laid out in order, relations in dict order)."""
    sizes, edge_index_dict, key2int, _, args = mag_rgcn_case(golden_mag_rgcn)
    ei, et, nt, li, l2g, k2i = U.group_hetero_graph(edge_index_dict, {"a": sizes[0], "b": sizes[1], "c": sizes[2]})
    assert torch.equal(ei, args[1]) and torch.equal(et, args[2]) and torch.equal(nt, args[3]) and torch.equal(li, args[4])
    assert k2i == key2int


def test_saint_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SAINT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, decl), f"{s} is not declared in include/egnn_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES
    assert "mag_pyg/gnn.py:361-366" in src
    assert _lib.load().egnn_abi_version() == 9 and "#define EGNN_ABI_VERSION 9" in src
    g = _lib.load().egnn_saint_induced_geometry
    assert g(0) == 64 and g(1) % 64 == 0 and g(2) >= g(1) and g(3) < 0


def test_saint_entry_points_reject_bad_arguments_before_any_launch():
    """Null pointers, negative sizes, L < 1 and N >= 2^31 come back as negative codes; callable without a GPU."""
    lib = _lib.load()
    ibuf, bbuf, fbuf = (ctypes.c_int64 * 64)(), (ctypes.c_uint8 * 64)(), (ctypes.c_float * 64)()
    ip, bp, fp = ctypes.addressof(ibuf), ctypes.addressof(bbuf), ctypes.addressof(fbuf)
    BIG = 1 << 31
    walk = lib.egnn_saint_random_walk_i64
    assert walk(None, ip, 4, 4, 2, 2, None, None, 0, None, ip, bp, None) < 0            # rowptr
    assert walk(ip, None, 4, 4, 2, 2, None, None, 0, None, ip, bp, None) < 0            # col with nnz > 0
    assert walk(ip, ip, 4, 4, 2, 2, None, None, 0, None, ip, None, None) < 0            # flag
    assert walk(ip, ip, 4, 4, 2, 0, None, None, 0, None, ip, bp, None) < 0              # L < 1
    assert walk(ip, ip, 4, 4, -1, 2, None, None, 0, None, ip, bp, None) < 0             # B < 0
    assert walk(ip, ip, 4, -1, 2, 2, None, None, 0, None, ip, bp, None) < 0             # nnz < 0
    assert walk(ip, ip, 0, 4, 2, 2, None, None, 0, None, ip, bp, None) < 0              # N < 1
    assert walk(ip, ip, BIG, 4, 2, 2, None, None, 0, None, ip, bp, None) < 0            # N >= 2^31
    assert walk(ip, ip, 4, 4, 2, 2, ip, None, 0, None, ip, bp, None) < 0                # start without rand
    assert walk(ip, ip, 4, 4, 2, 2, None, fp, 0, None, ip, bp, None) < 0                # rand without start
    assert walk(ip, ip, 4, 4, 0, 2, None, None, 0, None, None, bp, None) == 0           # no walks: nothing to do
    sel = lib.egnn_saint_select_i64
    assert sel(None, 4, ip, ip, 4, ip, 1 << 20, None) < 0
    assert sel(bp, 4, None, ip, 4, ip, 1 << 20, None) < 0
    assert sel(bp, 4, ip, None, 4, ip, 1 << 20, None) < 0
    assert sel(bp, -1, ip, ip, 4, ip, 1 << 20, None) < 0
    assert sel(bp, BIG, ip, ip, 4, ip, 1 << 20, None) < 0
    assert sel(bp, 4, ip, ip, 0, ip, 1 << 20, None) < 0
    cnt = lib.egnn_saint_induced_count_i64
    assert cnt(None, ip, ip, 4, None, 1, 0, 4, bp, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, None, ip, 4, None, 1, 0, 4, bp, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, None, 4, None, 1, 0, 4, bp, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, 4, None, 1, 0, 4, None, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, 4, None, 1, 0, 4, bp, None, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, 4, None, 1, 0, 4, bp, ip, None, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, -4, None, 1, 0, 4, bp, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, 4, None, 0, 0, 4, bp, ip, ip, ip, 1 << 20, None) < 0         # groups < 1
    assert cnt(ip, ip, ip, 4, None, 1, -1, 4, bp, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, 4, None, 1, 0, BIG, bp, ip, ip, ip, 1 << 20, None) < 0
    assert cnt(ip, ip, ip, 1 << 30, None, 4, 0, 4, bp, ip, ip, ip, 1 << 20, None) < 0   # groups * n_map >= 2^31
    fill = lib.egnn_saint_induced_fill_i64
    assert fill(None, ip, None, ip, 4, None, 1, 0, 4, bp, ip, ip, 4, ip, ip, ip, None) < 0
    assert fill(ip, ip, None, ip, 4, None, 1, 0, 4, bp, None, ip, 4, ip, ip, ip, None) < 0      # relabel
    assert fill(ip, ip, None, ip, 4, None, 1, 0, 4, bp, ip, None, 4, ip, ip, ip, None) < 0      # out_ptr
    assert fill(ip, ip, None, ip, 4, None, 1, 0, 4, bp, ip, ip, 4, ip, None, ip, None) < 0      # out_col with out_cap > 0
    assert fill(ip, ip, None, ip, 4, None, 1, 0, 4, bp, ip, ip, -1, ip, ip, ip, None) < 0       # out_cap < 0
    assert fill(ip, ip, None, ip, 4, None, 1, 0, BIG, bp, ip, ip, 4, ip, ip, ip, None) < 0
    assert fill(ip, ip, None, ip, 4, None, 1, 0, 4, bp, ip, ip, 0, None, None, None, None) == 0  # nothing kept: nothing to do
    gat = lib.egnn_saint_gather_i64
    assert gat(None, 4, ip, None, None, None, ip, None, None, None, None, 0, None, None, None) < 0   # node_idx
    assert gat(ip, -1, ip, None, None, None, ip, None, None, None, None, 0, None, None, None) < 0
    assert gat(ip, 4, ip, None, None, None, None, None, None, None, None, 0, None, None, None) < 0   # node_type without its output
    assert gat(ip, 4, None, None, None, bp, None, None, None, None, None, 0, None, None, None) < 0   # train_mask without its output
    assert gat(ip, 4, None, None, None, None, None, None, None, None, None, 4, ip, None, None) < 0   # edge_attr without edge_idx / output
    assert gat(ip, 4, None, None, None, None, None, None, None, None, None, -4, None, None, None) < 0
    assert gat(ip, 0, None, None, None, None, None, None, None, None, None, 0, None, None, None) == 0


def test_mag_hetero_like_counts_ranges_and_split():
    d = D.mag_hetero_like(0.001, seed=1)
    full = D.MAG
    assert list(d.num_nodes_dict) == ["author", "field_of_study", "institution", "paper"]
    for k, n in full["num_nodes"].items():
        assert d.num_nodes_dict[k] == max(4, round(n * 0.001))
    assert [k[1] for k in d.edge_index_dict] == ["affiliated_with", "writes", "cites", "has_topic"]
    for key, e in full["num_edges"].items():
        ei = d.edge_index_dict[key]
        assert ei.dtype == torch.int64 and ei.shape == (2, round(e * 0.001))
        assert int(ei.min()) >= 0 and int(ei[0].max()) < d.num_nodes_dict[key[0]] and int(ei[1].max()) < d.num_nodes_dict[key[-1]]
        assert torch.unique(ei[0] * d.num_nodes_dict[key[-1]] + ei[1]).numel() == ei.shape[1]      # no duplicate edge
    n_paper = d.num_nodes_dict["paper"]
    assert list(d.x_dict) == ["paper"] and d.x_dict["paper"].shape == (n_paper, 128)
    assert d.y_dict["paper"].shape == (n_paper, 1) and int(d.y_dict["paper"].max()) < d.num_classes == 349
    parts = torch.cat([d.split_idx[k]["paper"] for k in ("train", "valid", "test")])
    assert torch.equal(parts.sort().values, torch.arange(n_paper))
    assert d.split_idx["train"]["paper"].numel() == round(n_paper * 629_571 / 736_389)
    # power-law in-degrees: the busiest paper of `writes` is far above the mean
    deg = torch.bincount(d.edge_index_dict[("author", "writes", "paper")][1], minlength=n_paper)
    assert int(deg.max()) > 4 * float(deg.float().mean())
    same = D.mag_hetero_like(0.001, seed=1)
    assert all(torch.equal(same.edge_index_dict[k], v) for k, v in d.edge_index_dict.items())
    assert D.mag_like(0.0005).num_nodes == max(256, round(1_939_743 * 0.0005))                     # the homogeneous form is untouched


def test_sampler_constructor_contract():
    import types
    from efficient_gnns_amd.saint import GraphSAINTRandomWalkSampler
    data = types.SimpleNamespace(edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), num_nodes=4)
    with pytest.raises(NotImplementedError):
        GraphSAINTRandomWalkSampler(data, batch_size=2, walk_length=2, sample_coverage=10)
    s = GraphSAINTRandomWalkSampler(data, batch_size=2, walk_length=2, num_steps=5, sample_coverage=0, save_dir="/nowhere", log=False,
                                    num_workers=4)
    assert len(s) == 5
    with pytest.raises(_lib.HipExtensionError):          # no CPU fallback: sampling needs the GPU
        s.sample()
    with pytest.raises(ValueError):
        GraphSAINTRandomWalkSampler(types.SimpleNamespace(edge_index=torch.tensor([[0, 5], [1, 2]]), num_nodes=4), 2, 2)


def test_mag_dropin_names_import():
    dropin = os.path.join(ROOT, "efficient-gnns_amd", "dropin")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "torch_geometric" or k.startswith("torch_geometric.")}
    sys.path.insert(0, dropin)
    try:
        from torch_geometric.utils import to_undirected, subgraph
        from torch_geometric.data import Data, GraphSAINTRandomWalkSampler
        from torch_geometric.utils.hetero import group_hetero_graph
        import efficient_gnns_amd.saint as S
        assert to_undirected is U.to_undirected and subgraph is U.subgraph and group_hetero_graph is U.group_hetero_graph
        assert GraphSAINTRandomWalkSampler is S.GraphSAINTRandomWalkSampler and Data is S.Data
        d = Data(edge_index=torch.zeros((2, 0), dtype=torch.int64), num_nodes=3)
        assert d.num_nodes == 3
    finally:
        sys.path.remove(dropin)
        for k in [k for k in sys.modules if k == "torch_geometric" or k.startswith("torch_geometric.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_models_expose_the_mag_epoch_and_the_relations_keyword():
    import inspect
    import efficient_gnns_amd.models as PM
    import efficient_gnns_amd.nn as PN
    assert PM.MAG_MODES == PM.PPI_MODES
    assert "relations" in inspect.signature(PN.RGCNConv.forward).parameters and "relations" in inspect.signature(PM.RGCN.forward).parameters
    assert inspect.signature(PN.RGCNConv.forward).parameters["relations"].default is None
    assert list(inspect.signature(PM.mag_train_epoch).parameters) == ["model", "loader", "x_dict", "optimizer", "mode", "hp", "teacher_model",
                                                                    "student_proj", "teacher_proj"]
    assert list(inspect.signature(PM.mag_test).parameters) == ["model", "x_dict", "edge_index_dict", "key2int", "y_paper", "split_idx"]
    assert "out of scope" not in PM.RGCN.__doc__
