"""A full-graph PyG training script for ogbn-arxiv-shaped data, written against the PyG / torch-sparse API only.

The drop-in tests import it with ``efficient-gnns_amd/dropin`` first on ``sys.path``, so ``torch_geometric``, ``torch_sparse`` and
``criterion`` resolve to the package: a user script that runs unchanged on the kernels.  Models: ``[conv -> BatchNorm1d -> ReLU ->
dropout] x (L-1) -> conv`` with the last hidden activation kept as ``out_feat``; ``train()`` = one step with the supervised, logit-KD
or feature-distillation loss of ``args.training``; ``test()`` = eval forward, argmax and the three split accuracies.
"""
import torch
import torch.nn.functional as F
from torch_geometric.nn import GCNConv, SAGEConv

from criterion import gpw_criterion, kd_criterion, lpw_criterion, nce_criterion


class _Net(torch.nn.Module):
    def __init__(self, conv, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.convs = torch.nn.ModuleList([conv(a, b) for a, b in zip(widths[:-1], widths[1:])])
        self.bns = torch.nn.ModuleList([torch.nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1)])
        self.dropout = dropout
        self.out_feat = None

    def forward(self, x, adj_t):
        for conv, bn in zip(self.convs[:-1], self.bns):
            x = conv(x, adj_t)
            x = bn(x)
            x = F.relu(x)
            x = F.dropout(x, p=self.dropout, training=self.training)
            self.out_feat = x
        return self.convs[-1](x, adj_t)


class GCN(_Net):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__(lambda a, b: GCNConv(a, b, cached=True), in_channels, hidden_channels, out_channels, num_layers, dropout)


class SAGE(_Net):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__(SAGEConv, in_channels, hidden_channels, out_channels, num_layers, dropout)


def feature_loss(model, out, labels, train_idx, args, teacher_out_feat, student_proj, teacher_proj, edge_index):
    """(loss, loss_cls, loss_aux) of a feature-distillation mode: the projected hidden rows (nce / gpw) or the raw ones (lpw)."""
    if args.training in ("nce", "gpw"):
        feat = student_proj(model.out_feat[train_idx])
        teacher_feat = teacher_proj(teacher_out_feat[train_idx])
    else:
        feat, teacher_feat = model.out_feat[train_idx], teacher_out_feat[train_idx]
    if args.training == "nce":
        return nce_criterion(out, labels, feat, teacher_feat, args.beta, args.nce_T, args.max_samples)
    if args.training == "gpw":
        return gpw_criterion(out, labels, feat, teacher_feat, args.kernel, args.beta, args.max_samples)
    if args.training == "lpw":
        return lpw_criterion(out, labels, feat, teacher_feat, edge_index, args.kernel, args.beta)
    raise ValueError(args.training)


def forward_train(model, data, train_idx, student_proj, teacher_proj):
    model.train()
    for head in (student_proj, teacher_proj):
        if head is not None:
            head.train()
    return model(data.x, data.adj_t)[train_idx], data.y.squeeze(1)[train_idx]


def step(optimizer, loss, loss_cls, loss_aux):
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.item(), loss_cls.item(), loss_aux.item()


def train(model, data, train_idx, optimizer, args, teacher_out_feat, teacher_logits, student_proj, teacher_proj, edge_index):
    out, labels = forward_train(model, data, train_idx, student_proj, teacher_proj)
    if args.training == "supervised":
        loss = F.cross_entropy(out, labels)
        return step(optimizer, loss, loss, loss * 0)
    if args.training == "kd":
        return step(optimizer, *kd_criterion(out, labels, teacher_logits[train_idx], args.alpha, args.kd_T))
    return step(optimizer, *feature_loss(model, out, labels, train_idx, args, teacher_out_feat, student_proj, teacher_proj, edge_index))


@torch.no_grad()
def test(model, data, split_idx, evaluator):
    model.eval()
    out = model(data.x, data.adj_t)
    y_pred = out.argmax(dim=-1, keepdim=True)
    accs = tuple(evaluator.eval({"y_true": data.y[split_idx[k]], "y_pred": y_pred[split_idx[k]]})["acc"] for k in ("train", "valid", "test"))
    return out, accs
