"""The same PyG training script with the combined objective: logit KD plus ``beta`` times the auxiliary term of the
feature-distillation mode ``args.training`` (nce / gpw / lpw).  Models and ``test()`` are those of ``arxiv_train.py``."""
from arxiv_train import GCN, SAGE, feature_loss, forward_train, step, test  # noqa: F401

from criterion import kd_criterion


def train(model, data, train_idx, optimizer, args, teacher_out_feat, teacher_logits, student_proj, teacher_proj, edge_index):
    out, labels = forward_train(model, data, train_idx, student_proj, teacher_proj)
    loss_aux = feature_loss(model, out, labels, train_idx, args, teacher_out_feat, student_proj, teacher_proj, edge_index)[2]
    loss_kd, loss_cls, _ = kd_criterion(out, labels, teacher_logits[train_idx], args.alpha, args.kd_T)
    return step(optimizer, loss_kd + args.beta * loss_aux, loss_cls, loss_aux)
