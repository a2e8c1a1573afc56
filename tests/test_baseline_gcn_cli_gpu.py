"""GPU: `cluster_gcn --model-type baseline` on the toy dataset -- the five result lines, a finite and falling loss, a
validation accuracy above chance, and the refusal of --use-pp."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


def _toy():
    """datasets.toy() with labels its neighbourhoods determine, as tests/test_gat_cli_gpu.py relabels it: the argmax over
    the first 5 feature columns of the sum over a node's in-neighbours (the stock toy labels are uniform random: no model
    beats chance on them)."""
    from gist_amd import datasets
    ds = datasets.toy()
    g = ds.g
    n = g.number_of_nodes()
    rp = g.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    agg = torch.zeros(n, ds.num_classes).index_add_(0, rows, g.ndata['feat'][g.col.long(), :ds.num_classes])
    g.ndata['label'] = agg.argmax(1).to(g.ndata['label'].dtype)
    return ds


def test_cluster_gcn_cli_trains_the_baseline_gcn(monkeypatch):
    import gist_amd.nn
    from gist_amd.modules import BaselineGCN
    from gist_amd.scripts import cluster_gcn as cli
    losses = []

    class Recording(gist_amd.nn.CrossEntropyLoss):
        def forward(self, logits, labels):
            out = super().forward(logits, labels)
            losses.append(out.detach())
            return out

    monkeypatch.setattr(gist_amd.nn, 'CrossEntropyLoss', Recording)
    epochs = 5
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--model-type', 'baseline', '--n-epochs', str(epochs), '--batch-size', '4', '--n-hidden', '32',
         '--n-layers', '2', '--lr', '0.01', '--rnd-seed', '0', '--dropout', '0.2', '--use-layernorm'])
    lines = []
    ds = _toy()
    res = cli.main(args, dataset=ds, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    assert all(np.isfinite(float(l.split(':')[1])) for l in lines[-5:])
    assert sum('has no fused step' in l for l in lines) == 1       # --host-path engine (the default) runs the module loop
    model = res['model']
    assert isinstance(model, BaselineGCN) and model.tail == 'fused' and model._fused() and model.use_layernorm
    assert [tuple(l.weight.shape) for l in model.layers] == [(32, 32), (32, 32), (32, ds.num_classes)]
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert len(res['val_accs']) == epochs and all(0 <= a <= 1 for a in res['val_accs'] + res['test_accs'])
    per_epoch = torch.stack(losses).reshape(epochs, -1).mean(1).cpu()
    assert torch.isfinite(per_epoch).all() and per_epoch[-1] < per_epoch[0], per_epoch
    assert res['val_accs'][-1] > 1.0 / ds.num_classes, res['val_accs']


@pytest.mark.parametrize('flags', [['--use-pp'], ['--eval-path', 'blocked'], ['--eval-path', 'rows']],
                         ids=['use-pp', 'blocked', 'rows'])
def test_cluster_gcn_cli_refuses_what_the_family_does_not_have(flags):
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', 'baseline', '--n-epochs', '1'] + flags)
    with pytest.raises(SystemExit, match=flags[0]):
        cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: None)


def test_host_path_module_runs_the_same_loop_without_the_note():
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', 'baseline', '--n-epochs', '1', '--batch-size',
                                          '8', '--n-hidden', '16', '--host-path', 'module'])
    lines = []
    cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL and not any('has no fused step' in l for l in lines)
