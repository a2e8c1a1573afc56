"""GPU: `cluster_gcn --model-type graphsage --host-path step` -- the reference's CLI on one gist_graphsage_step per
iteration (gist_amd/graphsage_engine.py), with and without --use-pp, on the toy set."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
EPOCHS = 4


def _run(extra, monkeypatch):
    """-> (result, log lines, training-mode calls of the module path's tail op, per-step losses)"""
    from gist_amd import datasets, modules
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.scripts import cluster_gcn as cli
    calls, losses = [0], []
    real = modules.autograd.layer_norm_affine

    def counted(*a, **k):      # autograd.layer_norm_affine is torch.ops.gist.layer_norm_affine_fwd's only caller
        if torch.is_grad_enabled():           # (evaluate() runs the model under no_grad: not a training call)
            calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(modules.autograd, 'layer_norm_affine', counted)
    real_step = GraphSAGEEngine.train_step

    def recorded(self, *a, **k):
        loss = real_step(self, *a, **k)
        losses.append(loss.clone())
        return loss
    monkeypatch.setattr(GraphSAGEEngine, 'train_step', recorded)
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--model-type', 'graphsage', '--n-epochs', str(EPOCHS), '--batch-size', '4', '--n-hidden', '32',
         '--n-layers', '2', '--lr', '0.01', '--rnd-seed', '0', '--dropout', '0.2'] + extra)
    lines = []
    res = cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return res, lines, calls[0], losses


@pytest.mark.parametrize('use_pp', [False, True], ids=['plain', 'use-pp'])
def test_host_path_step_trains_on_the_fused_step(use_pp, monkeypatch):
    from gist_amd.modules import GraphSAGE
    res, lines, calls, losses = _run(['--host-path', 'step'] + (['--use-pp'] if use_pp else []), monkeypatch)
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    assert all(np.isfinite(float(l.split(':')[1])) for l in lines[-5:])
    assert calls == 0                                         # no tail op of the module path while training
    assert not any('has no fused step' in l for l in lines)
    model = res['model']
    assert isinstance(model, GraphSAGE) and model.layers[0].use_pp is use_pp
    assert model.layers[0].linear.weight.shape == (32, 2 * 32)      # in_feats is the width before pre-aggregation
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert len(res['val_accs']) == EPOCHS and all(0 <= a <= 1 for a in res['val_accs'] + res['test_accs'])
    assert res['total_time'] > 0 and len(losses) == EPOCHS * 6
    per_epoch = torch.cat(losses).reshape(EPOCHS, -1).mean(1).cpu()
    assert torch.isfinite(per_epoch).all() and per_epoch[-1] < per_epoch[0], per_epoch
    # the model the CLI returns is the engine's live view of the arena
    A = res['engine'].arena
    assert model.layers[0].linear.weight.data_ptr() == A.W[0].data_ptr()


def test_the_module_loop_still_counts(monkeypatch):
    """the counter above does count: --host-path module runs the tail op once per hidden layer and step"""
    _, lines, calls, losses = _run(['--host-path', 'module', '--n-epochs', '1'], monkeypatch)
    assert calls == 6 * 2 and losses == []
    assert sum('has no fused step' in l for l in lines) == 1


@pytest.mark.parametrize('model_type', ['sage', 'gat'])
def test_host_path_step_is_the_graphsage_familys(model_type):
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', model_type, '--n-epochs', '1',
                                          '--host-path', 'step'])
    with pytest.raises(SystemExit, match='--host-path step'):
        cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: None)
