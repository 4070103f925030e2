"""``GraphSAINTRandomWalkSampler(..., rank=r, world=W)``: the per-rank samplers' batches, interleaved, are the batches of the one
stream that ``world=1`` yields -- node lists, edge lists and ``relations`` -- and a second epoch continues the same stream."""
import pytest
import torch

from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 7


def _graph():
    gen = torch.Generator().manual_seed(3)
    N, E = 300, 2400
    node_type = torch.sort(torch.randint(0, 3, (N,), generator=gen)).values
    local_idx = torch.cat([torch.arange(int((node_type == t).sum())) for t in range(3)])
    d = Data(edge_index=torch.randint(0, N, (2, E), generator=gen), edge_attr=torch.randint(0, 4, (E,), generator=gen), node_type=node_type,
             local_node_idx=local_idx, num_nodes=N)
    d.y = torch.randint(0, 5, (N, 1), generator=gen)
    d.train_mask = torch.rand(N, generator=gen) < 0.5
    return d.to(DEV)


def _sampler(data, **kw):
    return GraphSAINTRandomWalkSampler(data, batch_size=20, walk_length=2, num_steps=STEPS, sample_coverage=0, save_dir=None, seed=5, **kw)


def _same(a, b):
    for name in ("node_idx", "edge_index", "edge_idx", "edge_attr", "node_type", "local_node_idx", "y", "train_mask", "walks"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.num_nodes == b.num_nodes
    (adj_a, rows_a), (adj_b, rows_b) = a.relations, b.relations
    assert len(adj_a) == len(adj_b) and len(rows_a) == len(rows_b)
    for x, y in zip(adj_a, adj_b):
        assert (x is None) == (y is None)
        if x is not None:
            (rp_x, col_x, _), (rp_y, col_y, _) = x.csr(), y.csr()
            assert torch.equal(rp_x, rp_y) and torch.equal(col_x, col_y)
    for x, y in zip(rows_a, rows_b):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def stream():
    """Two epochs of the world-1 sampler: 14 batches of one stream."""
    s = _sampler(_graph())
    assert len(s) == STEPS and s.global_steps == STEPS
    return list(s) + list(s)


@pytest.mark.parametrize("world", [2, 3])
def test_rank_slices_interleave_to_the_one_stream(stream, world):
    data = _graph()
    samplers = [_sampler(data, rank=r, world=world) for r in range(world)]
    assert sum(len(s) for s in samplers) == STEPS and all(s.global_steps == STEPS for s in samplers)
    for epoch in range(2):
        per_rank = [list(s) for s in samplers]
        assert [len(b) for b in per_rank] == [len(s) for s in samplers]
        for b in range(STEPS):
            _same(per_rank[b % world][b // world], stream[epoch * STEPS + b])
    assert not torch.equal(stream[0].node_idx, stream[1].node_idx)


@pytest.mark.parametrize("world", [2, 3])
def test_exactly_len_next_calls_per_epoch_keep_the_ranks_on_the_one_stream(stream, world):
    """How ``dist.mag_dp_train_epoch`` consumes a sampler: ``len()`` calls of ``next()`` and the iterator is dropped, never run to its
    end.  The second epoch must still be batches 7 .. 13 of the world-1 stream on every rank."""
    data = _graph()
    samplers = [_sampler(data, rank=r, world=world) for r in range(world)]
    for epoch in range(2):
        for r, s in enumerate(samplers):
            it = iter(s)
            got = [next(it) for _ in range(len(s))]
            del it
            for k, batch in enumerate(got):
                _same(batch, stream[epoch * STEPS + r + k * world])
    # a sampler whose iterator was made but never advanced has moved on by one epoch too
    s = _sampler(data, rank=1, world=2)
    iter(s)
    _same(next(iter(s)), stream[STEPS + 1])


def test_rank_outside_the_world_raises():
    with pytest.raises(ValueError):
        _sampler(_graph(), rank=2, world=2)
