"""Evaluation helpers with the reference's signatures (cluster_gcn/utils.py:47-80)."""
import torch

from . import hip


def evaluate(model, g, labels, mask, method='acc'):
    """Full-graph forward in eval mode + accuracy (utils.py:70-80).

    micro-F1 of a single-label argmax prediction equals accuracy (utils.py:47-56 with
    average='micro'), so both methods share one kernel.

    The `base_model` of a gist_amd.ist.DistributedGNNWrapper is not run layer by layer: its
    logits come from the trainer's FullGraphEvaluator on the wrapper's base replica (the
    evaluator of the engine path, built at the first evaluation of `g`), so both paths
    report the same accuracies."""
    assert method in ['acc', 'f1'], 'invalid method'
    model.eval()
    with torch.no_grad():
        full_graph = model.__dict__.get('_gist_full_graph')
        logits = full_graph(g).forward() if full_graph is not None else model(g).contiguous()
        dev = logits.device
        lab = labels.to(dev).to(torch.int32).contiguous()
        msk = mask.to(dev).to(torch.uint8).contiguous()
        total = int(msk.sum().item())
        if total == 0:
            return -1
        correct = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.argmax_correct(logits, lab, msk, correct)
        return correct.item() / total
