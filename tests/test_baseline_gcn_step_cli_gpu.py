"""GPU: `cluster_gcn --model-type baseline --host-path step` on the toy dataset -- the five result lines, no
`has no fused step` note, no autograd tail with gradients enabled (the step is the whole iteration), res['engine'] with
the model's weights as the arena's views, a falling loss and a validation accuracy above chance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


def _toy():
    """datasets.toy() with labels its neighbourhoods determine, as tests/test_baseline_gcn_cli_gpu.py relabels it: the
    argmax over the first 5 feature columns of the sum over a node's in-neighbours (the stock toy labels are uniform
    random: no model beats chance on them)."""
    from gist_amd import datasets
    ds = datasets.toy()
    g = ds.g
    n = g.number_of_nodes()
    rp = g.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    agg = torch.zeros(n, ds.num_classes).index_add_(0, rows, g.ndata['feat'][g.col.long(), :ds.num_classes])
    g.ndata['label'] = agg.argmax(1).to(g.ndata['label'].dtype)
    return ds


def test_cluster_gcn_cli_trains_the_baseline_gcn_on_the_fused_step(monkeypatch):
    from gist_amd import autograd
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    from gist_amd.modules import BaselineGCN
    from gist_amd.scripts import cluster_gcn as cli
    losses, taped = [], []
    real_step, real_tail = BaselineGCNEngine.train_step, autograd.gcn_tail

    def recording_step(self, *a, **k):
        out = real_step(self, *a, **k)
        losses.append(out.detach().clone())
        return out

    def watched_tail(*a, **k):
        taped.append(torch.is_grad_enabled())
        return real_tail(*a, **k)

    monkeypatch.setattr(BaselineGCNEngine, 'train_step', recording_step)
    monkeypatch.setattr(autograd, 'gcn_tail', watched_tail)
    epochs = 5
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--model-type', 'baseline', '--host-path', 'step', '--n-epochs', str(epochs), '--batch-size',
         '4', '--n-hidden', '32', '--n-layers', '2', '--lr', '0.01', '--rnd-seed', '0', '--dropout', '0.2',
         '--use-layernorm'])
    lines = []
    ds = _toy()
    res = cli.main(args, dataset=ds, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    assert all(np.isfinite(float(l.split(':')[1])) for l in lines[-5:])
    assert not any('has no fused step' in l for l in lines)
    assert not any(taped), 'autograd.gcn_tail ran with gradients enabled: the module loop, not the step'
    model, engine = res['model'], res['engine']
    assert isinstance(engine, BaselineGCNEngine) and isinstance(model, BaselineGCN) and engine.model is model
    assert engine.use_layernorm and engine.p_drop == pytest.approx(0.2) and engine.seed == 0 and engine.prefetch
    assert engine.dims == [(32, 32), (32, 32), (32, ds.num_classes)]
    A = engine.arena
    for k, layer in enumerate(model.layers):
        assert layer.weight.data_ptr() == A.W[k].data_ptr() and layer.bias.data_ptr() == A.b[k].data_ptr(), k
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert A.step == len(losses) > 0 and len(losses) % epochs == 0
    assert len(res['val_accs']) == epochs and all(0 <= a <= 1 for a in res['val_accs'] + res['test_accs'])
    per_epoch = torch.stack(losses).reshape(epochs, -1).mean(1).cpu()
    assert torch.isfinite(per_epoch).all() and per_epoch[-1] < per_epoch[0], per_epoch
    assert res['val_accs'][-1] > 1.0 / ds.num_classes, res['val_accs']


def test_the_default_host_path_still_runs_the_module_loop():
    """--host-path engine (the default) keeps its one note and returns no engine: the step is opt-in"""
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', 'baseline', '--n-epochs', '1', '--batch-size',
                                          '8', '--n-hidden', '16'])
    lines = []
    res = cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert sum('has no fused step' in l for l in lines) == 1 and 'engine' not in res


def test_the_step_refuses_use_pp():
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', 'baseline', '--host-path', 'step',
                                          '--n-epochs', '1', '--use-pp'])
    with pytest.raises(SystemExit, match='--use-pp'):
        cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: None)
