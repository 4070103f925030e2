"""``models.mag_accumulate_epoch(accumulate=k, seed=...)``: k GraphSAINT batches per optimisation step, the step's gradient the mean of the
batch-loss gradients, with the embedding tables under ``LazyRowAdam(duplicates="sum")`` -- against ``torch.optim.Adam`` (fused and
single-tensor) over the same accumulated and averaged gradients.  The batches come from ``sample(start, rand)`` with shared start
nodes, so consecutive batches provably name the same table rows (the case the summing row step exists for)."""
import functools

import numpy as np
import pytest
import torch

import efficient_gnns_amd as E
import efficient_gnns_amd.data as D
import efficient_gnns_amd.models as PM
import efficient_gnns_amd.utils as PU

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_BATCHES = 6


def ulp_at(x):
    return float(np.spacing(np.float32(x)))


@functools.lru_cache(maxsize=None)
def _mag_setup():
    """The recipe of test_gpu_lazy_adam.py::_mag_setup (mag_hetero_like(0.01, seed=2), RGCN 2 x 16, 6 batches), the batches drawn
    from injected walks: 20 start nodes that carry an embedding row are shared by all batches, 180 more are drawn per batch."""
    from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler
    d = D.mag_hetero_like(0.01, seed=2)
    eid = dict(d.edge_index_dict)
    for key, rev in ((("author", "affiliated_with", "institution"), ("institution", "to", "author")),
                     (("author", "writes", "paper"), ("paper", "to", "author")),
                     (("paper", "has_topic", "field_of_study"), ("field_of_study", "to", "paper"))):
        r, c = eid[key]
        eid[rev] = torch.stack([c, r])
    eid[("paper", "cites", "paper")] = PU.to_undirected(eid[("paper", "cites", "paper")])
    edge_index, edge_type, node_type, local_idx, l2g, key2int = PU.group_hetero_graph(eid, d.num_nodes_dict)
    N = node_type.numel()
    homo = Data(edge_index=edge_index, edge_attr=edge_type, node_type=node_type, local_node_idx=local_idx, num_nodes=N)
    homo.y = node_type.new_full((N, 1), -1)
    homo.y[l2g["paper"]] = d.y_dict["paper"]
    homo.train_mask = torch.zeros(N, dtype=torch.bool)
    homo.train_mask[l2g["paper"][d.split_idx["train"]["paper"]]] = True
    loader = GraphSAINTRandomWalkSampler(homo.to(DEV), batch_size=200, walk_length=2, num_steps=N_BATCHES, sample_coverage=0, save_dir=None,
                                         seed=7)
    gen = torch.Generator().manual_seed(9)
    paper = key2int["paper"]
    shared = (node_type != paper).nonzero().view(-1)[::37][:20]
    assert shared.numel() == 20
    batches = []
    for _ in range(N_BATCHES):
        start = torch.cat([shared, torch.randint(0, N, (180,), generator=gen)])
        batches.append(loader.sample(start, torch.rand(200, 2, generator=gen)))
    x_dict = {paper: d.x_dict["paper"].to(DEV)}
    nn_dict = {key2int[k]: n for k, n in d.num_nodes_dict.items()}
    for a, b in zip(batches, batches[1:]):                      # every pair of consecutive batches shares table rows
        ka = {(int(t), int(i)) for t, i in zip(a.node_type.tolist(), a.local_node_idx.tolist()) if t != paper}
        kb = {(int(t), int(i)) for t, i in zip(b.node_type.tolist(), b.local_node_idx.tolist()) if t != paper}
        assert len(ka & kb) >= 20
    assert all(int(b.train_mask.sum()) > 0 for b in batches)
    return d, eid, key2int, batches, x_dict, nn_dict


def _student(d, nn_dict, x_dict, eid, hidden=16):
    return PM.RGCN(128, hidden, d.num_classes, 2, 0.5, nn_dict, list(x_dict.keys()), len(eid)).to(DEV)


@pytest.mark.parametrize("mode", ["supervised", "kd"])
@pytest.mark.parametrize("accumulate", [2, 3])
def test_accumulated_epoch_equals_dense_adam(accumulate, mode):
    """Every parameter of the lazy run lies within 4 x the largest difference between torch's fused and single-tensor runs (the
    reference's own spread) plus one ulp of max |p| -- the model-level bound of test_gpu_lazy_adam.py; the accuracies are equal; no
    table ever gets a dense gradient; 6 batches make 6 / accumulate optimisation steps."""
    d, eid, key2int, batches, x_dict, nn_dict = _mag_setup()
    hp = dict(alpha=0.9, kd_T=4.0)
    eid_dev = {k: v.to(DEV) for k, v in eid.items()}
    teacher = None
    if mode == "kd":
        torch.manual_seed(5)
        teacher = _student(d, nn_dict, x_dict, eid, hidden=32)
        for p in teacher.parameters():
            p.requires_grad_(False)
    runs = {}
    for name in ("fused", "single", "lazy"):
        torch.manual_seed(0)
        model = _student(d, nn_dict, x_dict, eid)
        if name == "lazy":
            opt = PM.mag_optimizer(model, 0.005, duplicates="sum")
            assert isinstance(opt, E.LazyRowAdam)
        else:
            opt = torch.optim.Adam(model.parameters(), lr=0.005, **({"fused": True} if name == "fused" else {"foreach": False}))
        loss = PM.mag_accumulate_epoch(model, batches, x_dict, opt, mode, hp, teacher_model=teacher, accumulate=accumulate, seed=1)[0]
        assert loss == loss and loss > 0
        accs = PM.mag_test(model, x_dict, eid_dev, key2int, d.y_dict["paper"].to(DEV), d.split_idx)
        runs[name] = (model, opt, accs)
    lazy_model = runs["lazy"][0]
    steps = -(-N_BATCHES // accumulate)
    for emb in lazy_model.emb_dict.values():
        assert emb.grad is None and emb._egnn_rows.t == steps and emb._egnn_rows.flushed == steps
    assert runs["fused"][2] == runs["single"][2] == runs["lazy"][2]
    params = {k: [p.detach().double() for p in runs[k][0].parameters()] for k in runs}
    names = [n for n, _ in lazy_model.named_parameters()]
    spread = max(float((a - b).abs().max()) for a, b in zip(params["fused"], params["single"]))
    print(f"[mag accumulate k={accumulate} {mode}] spread of the two torch runs = {spread:.3e}")
    for n, a, b, c in zip(names, params["lazy"], params["fused"], params["single"]):
        err = max(float((a - b).abs().max()), float((a - c).abs().max()))
        bound = 4 * spread + ulp_at(float(b.abs().max()))
        print(f"[mag accumulate k={accumulate} {mode}] {n}: err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (n, err, bound)


def test_accumulate_with_the_default_optimiser_raises_before_any_step():
    d, eid, key2int, batches, x_dict, nn_dict = _mag_setup()
    torch.manual_seed(0)
    model = _student(d, nn_dict, x_dict, eid)
    opt = PM.mag_optimizer(model, 0.005)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(ValueError, match="duplicates='sum'"):
        PM.mag_accumulate_epoch(model, batches, x_dict, opt, "supervised", {}, accumulate=2)
    assert all(emb._egnn_rows.t == 0 for emb in model.emb_dict.values())
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


def test_seed_alone_keeps_the_plain_loop_with_the_default_optimiser():
    """``accumulate=1, seed=s`` is the plain loop with the generator reset before every batch: with unique rows per step the default
    (refusing) optimiser and the summing one give the same bits."""
    d, eid, key2int, batches, x_dict, nn_dict = _mag_setup()
    out = []
    for duplicates in ("refuse", "sum"):
        torch.manual_seed(0)
        model = _student(d, nn_dict, x_dict, eid)
        opt = PM.mag_optimizer(model, 0.005, duplicates=duplicates)
        PM.mag_accumulate_epoch(model, batches, x_dict, opt, "supervised", {}, seed=1)
        out.append([p.detach().clone() for p in model.parameters()])
    for a, b in zip(*out):
        assert torch.equal(a, b)
