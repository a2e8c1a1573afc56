"""GPU: `cluster_gcn --model-type gat --head-merge cat` on both host paths, and the default flag.

The runs go through `--dataset reddit-synth` on the reddit-synth generator at a test size (Reddit's feature width, class
count and degree on 6000 nodes in 60 parts, as tests/test_gat_step_gpu.py uses it): the full stand-in is 233 000 nodes
and would spend its time building the dataset, which is not what these tests are about."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


@pytest.fixture(scope='module')
def reddit_like():
    from gist_amd import datasets
    return lambda: datasets.reddit_synth(n=6000, n_blocks=60, train_frac=0.7)


def _run(make_ds, extra, epochs=2):
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(
        ['--dataset', 'reddit-synth', '--n-epochs', str(epochs), '--batch-size', '5', '--n-hidden', '8', '--n-layers',
         '2', '--lr', '0.01', '--rnd-seed', '0', '--model-type', 'gat', '--n-heads', '2'] + extra)
    lines = []
    res = cli.main(args, dataset=make_ds(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return res, lines


def _untimed(lines):
    return [l for l in lines if not l.startswith('Training Time')]


def _train_loss(model, make_ds):
    from gist_amd.nn import CrossEntropyLoss
    g = make_ds().g.to(torch.device('cuda', 0))
    tm, lab = g.ndata['train_mask'].bool(), g.ndata['label']
    with torch.no_grad():
        return float(CrossEntropyLoss()(model(g)[tm], lab[tm]))


def test_cat_cli_runs_on_both_host_paths_and_trains(reddit_like):
    from gist_amd.modules import GAT
    runs = {hp: _run(reddit_like, ['--head-merge', 'cat', '--host-path', hp]) for hp in ('engine', 'module')}
    (a, la), (b, lb) = runs['engine'], runs['module']
    for res, lines in runs.values():
        assert [l.split(':')[0] for l in lines[-5:]] == TAIL
        model = res['model']
        assert isinstance(model, GAT) and model.merge == 'cat' and len(res['val_accs']) == 2
        assert model.layers[1].heads[0].fc.in_features == 2 * 8
    # the two paths print the same accuracies and end on the same weights, so on the same losses
    assert _untimed(la) == _untimed(lb)
    assert a['val_accs'] == b['val_accs'] and a['test_accs'] == b['test_accs']
    for u, v in zip(a['model'].parameters(), b['model'].parameters()):
        assert torch.equal(u, v)
    # the training loss falls over the epochs: same-seed initial model, after one epoch, after two
    torch.manual_seed(0)
    ds = reddit_like()
    init = GAT(2, ds.g.ndata['feat'].shape[1], 8, ds.num_classes, 2, merge='cat').cuda()
    one, _ = _run(reddit_like, ['--head-merge', 'cat'], epochs=1)
    l0, l1, l2 = _train_loss(init, reddit_like), _train_loss(one['model'], reddit_like), _train_loss(a['model'], reddit_like)
    print('train loss: initial %.4f, one epoch %.4f, two epochs %.4f' % (l0, l1, l2))
    assert l2 < l1 < l0


@pytest.mark.parametrize('host_path', ['engine', 'module'])
def test_without_the_flag_the_output_is_the_mean_runs(reddit_like, host_path):
    a, la = _run(reddit_like, ['--host-path', host_path])
    b, lb = _run(reddit_like, ['--host-path', host_path, '--head-merge', 'mean'])
    assert _untimed(la) == _untimed(lb) and len(la) == len(lb)
    assert a['model'].merge == 'mean' and a['model'].layers[1].heads[0].fc.in_features == 8
    for u, v in zip(a['model'].parameters(), b['model'].parameters()):
        assert torch.equal(u, v)
