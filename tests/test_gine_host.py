"""Host checks of the fused gather-add-activate-aggregate path (csrc/gather_edge_scatter.hip, ``ops.gather_add_scatter``,
``lazy.LazyEdgeRows``) and of what is built on it for graph classification (``nn.GINConv`` / ``nn.GINEConv`` / ``nn.CategoricalEncoder``,
``saint.Batch``, ``data.molhiv_like``, ``models.MolGNN``): the C ABI additions against ``_lib.SIGNATURES``, the argument errors that must
come back before any launch, which adds of a ``lazy.LazyRows`` stay deferred, and the batch arithmetic on CPU tensors.  No GPU (the
kernels themselves: tests/test_gpu_gine.py)."""
import ctypes
import importlib
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from efficient_gnns_amd import _lib, data, lazy, models, ops, saint
from efficient_gnns_amd import nn as PN
from conftest import ROOT

EINVAL, EWORKSPACE, EALIGN = -1, -3, _lib.EGNN_EALIGN
NEW = ("egnn_gather_edge_scatter_ws_bytes", "egnn_gather_edge_scatter_runs_f32", "egnn_edge_gate_f32")
LAST = ("egnn_gather_scatter_ws_bytes", "egnn_gather_scatter_runs_f32", "egnn_edge_dot_f32")
CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}


def _header():
    src = open(os.path.join(ROOT, "include", "egnn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def _chunk():
    return int(re.search(r"#define\s+EGNN_ROWS_SUM_CHUNK\s+(\d+)", _header()).group(1))


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_header_prototype_matches_the_binding_argument_by_argument(name):
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;{]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/egnn_hip.h"
    res, argtypes = _lib.SIGNATURES[name]
    assert res is CTYPE[m.group(1)]
    decls = [a.strip() for a in m.group(2).split(",")]
    assert len(decls) == len(argtypes), (decls, argtypes)
    for decl, ct in zip(decls, argtypes):
        want = ctypes.c_void_p if "*" in decl else CTYPE[re.sub(r"\bconst\b", "", decl).split()[0]]
        assert ct is want, (name, decl, ct)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"


def test_the_abi_is_still_9_and_the_source_shares_the_cut():
    assert re.search(r"#define\s+EGNN_ABI_VERSION\s+9\b", _header())
    assert _lib.load().egnn_abi_version() == 9
    build = importlib.import_module("efficient_gnns_amd.build")
    assert "gather_edge_scatter.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gather_edge_scatter.hip"))
    text = open(os.path.join(build.CSRC, "gather_edge_scatter.hip")).read()
    code = text.split("namespace {", 1)[1]
    assert '#include "rows_runs.h"' in text and "atomic" not in code                # no atomics of any kind in the code
    for shared in ("chunk_start(", "chunk_is_long(", "chunk_limit(", "part_slot(", "part_slots(", "part_pitch(", "long_run_head(", "run_chunks(",
                   "key_usable(", "load_w<", "store_w<", "dispatch_w(", "lanes_lg(", "egnn_rows_add_runs_ws_bytes("):
        assert shared in code, shared                                              # the cut, the slots and the workspace are the shared ones
    for own in ("int64_t lower_bound", "int64_t part_slot", "int64_t part_slots", "int64_t part_pitch", "bool key_usable", "void load_w",
                "void store_w", "void dispatch_w", "int lanes_lg", "void chunk_start", "bool chunk_is_long", "int64_t chunk_limit",
                "int64_t long_run_head", "int64_t run_chunks"):
        assert own not in text, own                                                # none of them is defined again
    names = re.findall(r"\b(?:int|size_t|int64_t)\s+(egnn_\w+)\s*\(", _header())
    assert tuple(names[-3:]) == LAST                                                # the new section sits before the gather_scatter block
    assert tuple(names[-6:-3]) == NEW


def _buf():
    keep = (ctypes.c_float * 64)()                       # a 16-byte aligned stand-in: nothing is launched on these paths
    return (ctypes.addressof(keep) + 15) & ~15, keep


def test_workspace_size_is_the_run_sums():
    lib, chunk = _lib.load(), _chunk()
    assert lib.egnn_gather_edge_scatter_ws_bytes(0, 256) == 0 and lib.egnn_gather_edge_scatter_ws_bytes(chunk, 256) == 0
    for S in (chunk + 1, 10 * chunk, 1_000_000):
        for C in (1, 40, 260, 300):
            assert lib.egnn_gather_edge_scatter_ws_bytes(S, C) == lib.egnn_rows_add_runs_ws_bytes(S, C) > 0


def test_gather_edge_scatter_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()
    chunk = _chunk()

    def call(**kw):
        S = kw.get("S", 3)
        shift = kw.get("shift", max(1, (S - 1).bit_length()))
        return lib.egnn_gather_edge_scatter_runs_f32(kw.get("out", base), kw.get("ld_out", 8), kw.get("n_rows", 4), kw.get("count", base),
                                                     kw.get("keys", base), S, shift, kw.get("frm", base), kw.get("x", base), kw.get("ld_x", 8),
                                                     kw.get("n_x", 5), kw.get("from_count", None), kw.get("e", base), kw.get("ld_e", 8),
                                                     kw.get("own", base), kw.get("ld_own", 8), kw.get("mode", 1), kw.get("C", 8),
                                                     kw.get("reduce", 0), kw.get("ws", None), kw.get("ws_bytes", 0), None)
    for red in (0, 1):
        for mode in (0, 1, 2):      # S == 0 without an output: nothing to do
            assert lib.egnn_gather_edge_scatter_runs_f32(None, 8, 4, None, None, 0, 0, None, None, 8, 5, None, None, 0, None, 0, mode, 8, red,
                                                         None, 0, None) == 0
    assert call(reduce=2) == EINVAL and call(reduce=3) == EINVAL and call(reduce=-1) == EINVAL       # max / min stay with egnn_scatter_runs_f32
    assert call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(mode=1, e=None) == EINVAL and call(mode=2, e=None) == EINVAL                         # relu and its gate read the edge rows
    assert call(mode=2, own=None) == EINVAL and call(mode=2, ld_own=7) == EINVAL                     # the gate reads the own row
    assert call(ld_out=7) == EINVAL and call(ld_x=4) == EINVAL and call(ld_e=7) == EINVAL and call(C=0) == EINVAL and call(n_x=-1) == EINVAL
    assert call(out=None) == EINVAL and call(keys=None) == EINVAL and call(frm=None) == EINVAL and call(x=None) == EINVAL
    assert call(S=-1) == EINVAL and call(S=2 ** 31 - 1) == EINVAL and call(n_rows=2 ** 31 - 1) == EINVAL and call(shift=5) == EINVAL
    assert call(n_x=2 ** 31 - 1) == EINVAL
    assert call(reduce=1, count=None) == EINVAL                                     # mean needs the counts
    S = 3 * chunk + 5
    need = lib.egnn_gather_edge_scatter_ws_bytes(S, 8)
    assert need > 0
    assert call(S=S, ws=None, ws_bytes=need) == EWORKSPACE and call(S=S, ws=base, ws_bytes=need - 1) == EWORKSPACE
    assert call(S=S, ws=base + 4, ws_bytes=need) == EALIGN
    assert call(keys=base + 4) == EALIGN and call(frm=base + 4) == EALIGN and call(count=base + 2) == EALIGN
    assert call(from_count=base + 2) == EALIGN and call(x=base + 2) == EALIGN and call(e=base + 2) == EALIGN
    assert call(mode=2, own=base + 2) == EALIGN


def test_edge_gate_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    base, keep = _buf()

    def call(**kw):
        return lib.egnn_edge_gate_f32(kw.get("de", base), kw.get("ld_de", 8), kw.get("S", 3), kw.get("C", 8), kw.get("a_rows", base),
                                      kw.get("x", base), kw.get("ld_x", 8), kw.get("n_x", 4), kw.get("e", base), kw.get("ld_e", 8),
                                      kw.get("b_rows", base), kw.get("g", base), kw.get("ld_g", 8), kw.get("n_g", 5), kw.get("b_count", None),
                                      kw.get("mode", 1), None)
    assert lib.egnn_edge_gate_f32(None, 8, 0, 8, None, None, 8, 4, None, 8, None, None, 8, 5, None, 1, None) == 0          # S == 0
    assert call(S=-1) == EINVAL and call(C=0) == EINVAL and call(ld_de=7) == EINVAL and call(ld_g=7) == EINVAL and call(n_g=-1) == EINVAL
    assert call(mode=2) == EINVAL and call(mode=-1) == EINVAL                       # the gate of the edge rows: ADD or ADD_RELU
    assert call(ld_x=7) == EINVAL and call(ld_e=7) == EINVAL
    assert call(de=None) == EINVAL and call(b_rows=None) == EINVAL and call(g=None) == EINVAL
    assert call(a_rows=None) == EINVAL and call(e=None) == EINVAL and call(x=None) == EINVAL
    assert call(a_rows=base + 4) == EALIGN and call(b_rows=base + 4) == EALIGN and call(b_count=base + 2) == EALIGN
    assert call(e=base + 2) == EALIGN and call(g=base + 2) == EALIGN


# ------------------------------------------------------------------------------------------------
# ops.gather_add_scatter: what is refused before any plan is built or kernel called
# ------------------------------------------------------------------------------------------------
def test_python_argument_errors_come_first(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a kernel path was reached")
    monkeypatch.setattr(ops._GatherAddScatter, "apply", boom)
    monkeypatch.setattr(ops, "_rows_plan_launch", boom)
    x, e = torch.zeros(5, 8), torch.zeros(6, 8)
    src, dst = torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)
    for red in ("max", "min"):
        with pytest.raises(ValueError, match="ops.scatter"):
            ops.gather_add_scatter(x, src, dst, 4, e, reduce=red)
    with pytest.raises(ValueError, match="reduce"):
        ops.gather_add_scatter(x, src, dst, 4, e, reduce="prod")
    with pytest.raises(ValueError, match="act"):
        ops.gather_add_scatter(x, src, dst, 4, e, act="elu")
    with pytest.raises(TypeError):
        ops.gather_add_scatter(x.double(), src, dst, 4, e)
    with pytest.raises(TypeError):
        ops.gather_add_scatter(x, src, dst, 4, e.double())
    with pytest.raises(TypeError):
        ops.gather_add_scatter(torch.zeros(5, 2, 4), src, dst, 4, e)
    with pytest.raises(ValueError, match="columns"):
        ops.gather_add_scatter(x, src, dst, 4, torch.zeros(6, 1))
    with pytest.raises(ValueError, match="edge rows"):
        ops.gather_add_scatter(x, src, dst[:5], 4, e)
    with pytest.raises(TypeError, match="src"):
        ops.gather_add_scatter(x, src.int(), dst, 4, e)
    plan_src, plan_dst = ops.RowsPlan(src, 5, 6), ops.RowsPlan(dst, 4, 6)
    with pytest.raises(ValueError, match="built for 4 rows"):
        ops.gather_add_scatter(x, plan_src, plan_dst, 9, e)
    with pytest.raises(ValueError, match="built for 5 rows"):
        ops.gather_add_scatter(torch.zeros(7, 8), plan_src, plan_dst, 4, e)
    with pytest.raises(_lib.HipExtensionError):
        ops.gather_add_scatter(x, plan_src, plan_dst, 4, e)                         # everything fits: refused as a CPU tensor, no fallback


# ------------------------------------------------------------------------------------------------
# lazy.LazyRows + edge rows
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    """CPU tensors stand in for the device's: the shape rules are what is under test."""
    monkeypatch.setattr(lazy, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ops, "FUSE_LAZY_ROWS", True)
    monkeypatch.setattr(ops, "FUSE_EDGE_ROWS", True)
    calls = []

    def gather_add_scatter(x, src, dst, dim_size, edge, act="relu", reduce="sum"):
        calls.append((x, src, dst, dim_size, edge, act, reduce))
        return "fused"
    monkeypatch.setattr(ops, "gather_add_scatter", gather_add_scatter)
    return calls


ADDS = (lambda r, e: r + e, lambda r, e: e + r, lambda r, e: torch.add(r, e), lambda r, e: torch.add(e, r))
RELUS = (lambda m: m.relu(), lambda m: F.relu(m), lambda m: torch.relu(m))


def test_lazy_rows_plus_edge_rows_stays_deferred(stubbed):
    E = 6
    idx = torch.tensor([0, 2, 2, 1, 4, 0])
    x2 = torch.randn(5, 8)
    for e in (torch.randn(E, 8), torch.nn.Parameter(torch.randn(E, 8))):
        for add in ADDS:
            rows = lazy.LazyRows(x2, idx)
            got = add(rows, e)
            assert isinstance(got, lazy.LazyEdgeRows) and got._act is None and rows._value is None
            assert tuple(got.shape) == (E, 8)
            for relu in RELUS:
                act = relu(got)
                assert isinstance(act, lazy.LazyEdgeRows) and act._act == "relu" and act._value is None and rows._value is None
                assert torch.equal(lazy.materialise(relu(add(lazy.LazyRows(x2, idx), e))), torch.relu(x2[idx] + e))
            assert torch.equal(lazy.materialise(got), x2[idx] + e)                  # every other consumer: exactly take_rows(...) + e


def test_other_operands_and_consumers_materialise(stubbed):
    E = 6
    idx = torch.tensor([0, 2, 2, 1, 4, 0])
    x2, x3 = torch.randn(5, 8), torch.randn(5, 2, 4)
    rejected = ((x2, torch.randn(E, 1)), (x2, torch.tensor(0.5)), (x2, torch.randn(E, 8).double()), (x2, torch.randn(1, 8)), (x3, torch.randn(E, 2, 4)),
                (x2, 2.0))
    for base, e in rejected:
        for add in ADDS[:2]:
            rows = lazy.LazyRows(base, idx)
            got = add(rows, e)
            assert not isinstance(got, lazy._TensorLike) and rows._value is not None, (base.shape, getattr(e, "shape", e))
            assert torch.equal(got, base[idx] + e)
    e = torch.randn(E, 8)
    rows = lazy.LazyRows(x2, idx)
    got = torch.add(rows, e, alpha=2.0)                                             # alpha: not the plain add
    assert isinstance(got, torch.Tensor) and torch.equal(got, x2[idx] + 2.0 * e)
    second = (lazy.LazyRows(x2, idx) + e) + e                                       # a second add
    assert isinstance(second, torch.Tensor) and torch.equal(second, x2[idx] + e + e)
    twice = F.relu(F.relu(lazy.LazyRows(x2, idx) + e))                              # relu twice
    assert isinstance(twice, torch.Tensor) and torch.equal(twice, torch.relu(x2[idx] + e))
    inplace = F.relu(lazy.LazyRows(x2, idx) + e, inplace=True)
    assert isinstance(inplace, torch.Tensor) and torch.equal(inplace, torch.relu(x2[idx] + e))
    formed = lazy.LazyRows(x2, idx)
    lazy.materialise(formed)
    assert isinstance(formed + e, torch.Tensor)                                     # rows that exist already
    assert isinstance((lazy.LazyRows(x2, idx) + e) * 2.0, torch.Tensor)             # any other operator
    for switch in ("FUSE_EDGE_ROWS", "FUSE_LAZY_ROWS"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ops, switch, False)
            assert isinstance(lazy.LazyRows(x2, idx) + e, torch.Tensor)
    assert not stubbed


def test_scatter_hands_unformed_edge_rows_to_gather_add_scatter(stubbed):
    E = 6
    idx, index = torch.tensor([0, 2, 2, 1, 4, 0]), torch.tensor([1, 1, 0, 3, 3, 3])
    x2, e = torch.randn(5, 8), torch.randn(E, 8)
    plan = lambda: "the call's plan"                                                # noqa: E731
    assert ops.scatter(F.relu(lazy.LazyRows(x2, idx, plan=plan) + e), index, 4, "mean") == "fused"
    assert stubbed[-1][0] is x2 and stubbed[-1][1:4] == ("the call's plan", index, 4) and stubbed[-1][4] is e and stubbed[-1][5:] == ("relu", "mean")
    assert ops.scatter(e + lazy.LazyRows(x2, idx), index, 4, "add", plan="dst plan") == "fused"
    assert stubbed[-1][1] is idx and stubbed[-1][2] == "dst plan" and stubbed[-1][4] is e and stubbed[-1][5:] == (None, "add")
    out, arg = ops.scatter((lazy.LazyRows(x2, idx) + e).relu(), index, 4, return_arg=True)
    assert out == "fused" and arg is None and stubbed[-1][5:] == ("relu", "sum")
    n = len(stubbed)
    x2.add_(1.0)                                                                    # the base changed after the rows were asked for
    stale = lazy.LazyRows(x2, idx, base_version=x2._version - 1)
    with pytest.raises(RuntimeError, match="inplace"):
        ops.scatter(F.relu(stale + e), index, 4)
    for red in ("max", "min"):                                                      # these materialise (and then need the device)
        with pytest.raises(_lib.HipExtensionError):
            ops.scatter(F.relu(lazy.LazyRows(x2, idx) + e), index, 4, red)
    assert len(stubbed) == n


# ------------------------------------------------------------------------------------------------
# batches, layers, the model
# ------------------------------------------------------------------------------------------------
def _graph(n, edges, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.tensor(edges, dtype=torch.int64).view(-1, 2).t().contiguous()
    return saint.Data(x=torch.randint(0, 5, (n, 9), generator=g), edge_index=ei, edge_attr=torch.randint(0, 3, (ei.shape[1], 3), generator=g),
                      y=torch.rand(1, 1, generator=g), num_nodes=n)


def test_batch_from_data_list_offsets_batch_and_ptr():
    graphs = [_graph(3, [(0, 1), (1, 0), (1, 2), (2, 1)], 1), _graph(2, [], 2), _graph(0, [], 3), _graph(4, [(0, 3), (3, 0)], 4)]
    b = saint.Batch.from_data_list(graphs)
    assert b.num_graphs == 4 and b.num_nodes == 9
    assert b.ptr.tolist() == [0, 3, 5, 5, 9] and b.batch.tolist() == [0, 0, 0, 1, 1, 3, 3, 3, 3] and b.batch.dtype == torch.int64
    assert b.edge_index.tolist() == [[0, 1, 1, 2, 5, 8], [1, 0, 2, 1, 8, 5]]        # each graph's ids moved by the nodes before it
    assert torch.equal(b.x, torch.cat([g.x for g in graphs])) and torch.equal(b.edge_attr, torch.cat([g.edge_attr for g in graphs]))
    assert torch.equal(b.y, torch.cat([g.y for g in graphs])) and b.y.shape == (4, 1)
    assert not hasattr(saint.Batch.from_data_list([saint.Data(x=torch.zeros(2, 1))]), "edge_index")
    with pytest.raises(ValueError):
        saint.Batch.from_data_list([])


def test_molhiv_like_has_the_documented_shape():
    graphs = data.molhiv_like(200, seed=0)
    assert len(graphs) == 200 and all(6 <= g.x.shape[0] <= 50 for g in graphs)
    nodes, edges = sum(g.x.shape[0] for g in graphs), sum(g.edge_index.shape[1] for g in graphs)
    assert 2.0 <= edges / nodes <= 2.4                                              # mean degree ~2.2
    for g in graphs[:20]:
        n, ei = g.x.shape[0], g.edge_index
        assert g.x.shape == (n, 9) and g.edge_attr.shape == (ei.shape[1], 3) and g.y.shape == (1, 1) and float(g.y) in (0.0, 1.0)
        assert g.x.dtype == g.edge_attr.dtype == ei.dtype == torch.int64 and int(ei.min()) >= 0 and int(ei.max()) < n
        pairs = set(map(tuple, ei.t().tolist()))
        assert all((b, a) in pairs for a, b in pairs) and len(pairs) == ei.shape[1] and all(a != b for a, b in pairs)    # both directions, once
        assert all(int(g.x[:, k].max()) < d for k, d in enumerate(PN.ATOM_DIMS)) and all(int(g.edge_attr[:, k].max()) < d for k, d in enumerate(PN.BOND_DIMS))
    again = data.molhiv_like(200, seed=0)
    assert all(torch.equal(a.edge_index, b.edge_index) and torch.equal(a.x, b.x) for a, b in zip(graphs, again))


@pytest.mark.parametrize("cls", (PN.GINConv, PN.GINEConv))
def test_gin_convs_state_dict_and_reset(cls):
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 8))
    conv = cls(mlp, eps=0.5)
    assert list(conv.state_dict()) == ["eps", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]
    assert not isinstance(conv.eps, torch.nn.Parameter) and float(conv.eps) == 0.5 and conv.aggr == "add"
    trained = cls(mlp, eps=0.5, train_eps=True)
    assert isinstance(trained.eps, torch.nn.Parameter) and sorted(trained.state_dict()) == sorted(conv.state_dict())
    before = mlp[0].weight.detach().clone()
    with torch.no_grad():
        trained.eps.fill_(3.0)
    trained.reset_parameters()
    assert float(trained.eps.detach()) == 0.5 and not torch.equal(mlp[0].weight, before)     # nn's modules and eps are reset
    if cls is PN.GINEConv:
        with pytest.raises(ValueError, match="widths"):
            conv(torch.zeros(4, 8), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 5))


def test_the_new_names_resolve_through_the_dropin_path():
    dropin = os.path.join(ROOT, "efficient-gnns_amd", "dropin")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "torch_geometric" or k.startswith("torch_geometric.")}
    sys.path.insert(0, dropin)
    try:
        from torch_geometric.data import Batch
        from torch_geometric.nn import GINConv, GINEConv, global_add_pool, global_max_pool, global_mean_pool
        assert GINConv is PN.GINConv and GINEConv is PN.GINEConv and Batch is saint.Batch
        assert (global_add_pool, global_mean_pool, global_max_pool) == (PN.global_add_pool, PN.global_mean_pool, PN.global_max_pool)
    finally:
        sys.path.remove(dropin)
        for k in [k for k in sys.modules if k == "torch_geometric" or k.startswith("torch_geometric.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_categorical_encoder_shapes_and_errors():
    enc = PN.CategoricalEncoder((4, 7), 6)
    assert [tuple(p.shape) for p in enc.parameters()] == [(4, 6), (7, 6)] and list(enc.state_dict()) == ["embeddings.0.weight", "embeddings.1.weight"]
    for bad in ((), (3, 0), (-1,)):
        with pytest.raises(ValueError, match="cardinalities"):
            PN.CategoricalEncoder(bad, 6)
    with pytest.raises(ValueError, match="emb_dim"):
        PN.CategoricalEncoder((3,), 0)
    with pytest.raises(ValueError, match="int64"):
        enc(torch.zeros(5, 3, dtype=torch.int64))                                   # three columns for two tables
    with pytest.raises(ValueError, match="int64"):
        enc(torch.zeros(5, 2))
    with pytest.raises(_lib.HipExtensionError):
        enc(torch.zeros(5, 2, dtype=torch.int64))                                   # everything fits: refused as a CPU tensor, no fallback
    assert len(PN.ATOM_DIMS) == 9 and len(PN.BOND_DIMS) == 3


def test_molgnn_construction_and_state_dict_keys():
    gine = models.MolGNN("gine", num_layers=2, emb_dim=8)
    keys = set(gine.state_dict())
    want = {f"atom_encoder.embeddings.{k}.weight" for k in range(9)} | {f"bond_encoders.{l}.embeddings.{k}.weight" for l in range(2) for k in range(3)}
    want |= {f"convs.{l}.{name}" for l in range(2) for name in ("eps", "nn.0.weight", "nn.0.bias", "nn.1.weight", "nn.1.bias", "nn.3.weight", "nn.3.bias")}
    want |= {f"bns.{l}.{name}" for l in range(2) for name in ("weight", "bias")} | {"graph_pred_linear.weight", "graph_pred_linear.bias"}
    assert want <= keys and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in keys - want)
    assert all(isinstance(c, PN.GINEConv) for c in gine.convs) and gine.graph_pred_linear.weight.shape == (1, 8)
    gin = models.MolGNN("gin", num_layers=3, emb_dim=8, pool="add")
    assert all(isinstance(c, PN.GINConv) for c in gin.convs) and len(gin.bns) == 3 and not any(k.startswith("bond_encoders") for k in gin.state_dict())
    default = models.MolGNN()
    assert (default.conv, default.num_layers, default.emb_dim, default.dropout, default.pool) == ("gin", 5, 300, 0.5, "mean")
    for bad in (dict(conv="gcn"), dict(pool="median"), dict(num_layers=0)):
        with pytest.raises(ValueError):
            models.MolGNN(**bad)


def test_mol_batch_loss_refuses_other_modes():
    model = models.MolGNN("gin", num_layers=1, emb_dim=8)
    for mode in ("fitnet", "at", "gpw", "lpw", "nce", "bogus"):
        with pytest.raises(NotImplementedError, match=mode):
            models.mol_batch_loss(model, None, mode, {})
    with pytest.raises(ValueError, match="teacher_logits"):
        models.mol_batch_loss(model, None, "kd", {})


# ------------------------------------------------------------------------------------------------
# deferred inputs, nested resets, the edge rows' version
# ------------------------------------------------------------------------------------------------
class _Deferred(lazy._TensorLike):
    """A deferred activation as a ``BatchNorm1d`` hands one out under ``accel``: no ``Tensor``, and ``[1]`` is row 1."""

    def __init__(self, value):
        self._v, self._value, self.formed = value, None, 0

    shape = property(lambda self: self._v.shape)

    def _egnn_materialise(self, pick=None):
        self.formed += 1
        self._value = self._v
        return self._v if pick is None else self._v[pick]

    def __getitem__(self, idx):
        return self._egnn_materialise()[idx]


@pytest.mark.parametrize("cls", (PN.GINConv, PN.GINEConv))
def test_a_deferred_node_input_is_formed_not_indexed_as_a_pair(cls, monkeypatch):
    x, ei, e = torch.randn(5, 8), torch.zeros(2, 3, dtype=torch.int64), torch.randn(3, 8)
    seen = []

    def propagate(self, edge_index, size=None, **kw):
        seen.append(kw["x"])
        return torch.zeros(5, 8)
    monkeypatch.setattr(cls, "propagate", propagate)
    conv = cls(torch.nn.Identity(), eps=0.5)
    extra = (e,) if cls is PN.GINEConv else ()
    want = 1.5 * x                                                                  # every node's OWN row, not row 1 for all of them
    deferred = _Deferred(x)
    assert torch.equal(conv(deferred, ei, *extra), want) and deferred.formed == 1
    assert seen[-1][0] is x and seen[-1][1] is x                                    # propagate gets the real tensor on both sides
    target = torch.randn(5, 8)
    assert torch.equal(conv((_Deferred(x), _Deferred(target)), ei, *extra), 1.5 * target)
    assert seen[-1][0] is x and seen[-1][1] is target
    assert conv((x, None), ei, *extra).shape == (5, 8)                              # no target rows: no self term
    with pytest.raises(ValueError, match="pair"):
        conv((x, x, x), ei, *extra)
    with pytest.raises(TypeError):
        conv("x", ei, *extra)
    if cls is PN.GINEConv:
        assert torch.equal(conv(x, ei, _Deferred(e)), want) and seen[-1] == (x, x)  # a deferred edge_attr is formed too


def test_reset_prefers_a_modules_own_reset_parameters():
    enc = PN.CategoricalEncoder((50, 60), 16)
    conv = PN.GINConv(torch.nn.Sequential(enc, torch.nn.Linear(16, 16)))
    calls = []
    real = enc.reset_parameters
    enc.reset_parameters = lambda: calls.append("encoder") or real()
    conv.reset_parameters()
    assert calls == ["encoder"]                                                     # the encoder's own rule, not nn.Embedding's for its tables
    bound = (6.0 / (50 + 16)) ** 0.5
    assert float(enc.embeddings[0].weight.detach().abs().max()) <= bound                     # xavier-uniform, where Embedding's normal init would exceed it


def test_edge_rows_changed_in_place_before_they_are_consumed_raise(stubbed):
    idx, index = torch.tensor([0, 2, 2, 1, 4, 0]), torch.tensor([1, 1, 0, 3, 3, 3])
    x2, e = torch.randn(5, 8), torch.randn(6, 8)
    for spell in (lambda r: r + e, lambda r: F.relu(r + e), lambda r: (r + e).relu()):
        msg = spell(lazy.LazyRows(x2, idx))
        e.add_(1.0)
        with pytest.raises(RuntimeError, match="inplace"):
            ops.scatter(msg, index, 4)
        with pytest.raises(RuntimeError, match="inplace"):
            lazy.materialise(msg)
    assert not stubbed
    assert ops.scatter(F.relu(lazy.LazyRows(x2, idx) + e), index, 4) == "fused"     # unchanged since the add: consumed
