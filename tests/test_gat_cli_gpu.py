"""GPU: `cluster_gcn --model-type gat --n-heads 4` trains the reference's GAT (cluster_gcn_ist_distrib_gat.py:77-79)
on the reference's loop over the drop-in classes and keeps the five-line stdout tail (cluster_gcn.py:132-136)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


def _toy():
    """datasets.toy() with labels its neighbourhoods determine: the argmax over the first 5 feature columns of the
    sum over a node's in-neighbours (the stock toy labels are uniform random: no model beats chance on them)."""
    from gist_amd import datasets
    ds = datasets.toy()
    g = ds.g
    n = g.number_of_nodes()
    rp = g.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    agg = torch.zeros(n, ds.num_classes).index_add_(0, rows, g.ndata['feat'][g.col.long(), :ds.num_classes])
    g.ndata['label'] = agg.argmax(1).to(g.ndata['label'].dtype)
    return ds


def _run(host_path='engine', epochs=5):
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--n-epochs', str(epochs), '--batch-size', '4', '--n-hidden', '32', '--n-layers', '2',
         '--lr', '0.01', '--rnd-seed', '0', '--model-type', 'gat', '--n-heads', '4', '--host-path', host_path])
    lines = []
    res = cli.main(args, dataset=_toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return res, lines


def test_gat_cli_trains_and_keeps_the_tail():
    from gist_amd.modules import GAT
    from gist_amd.nn import CrossEntropyLoss
    res, lines = _run()
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    for l in lines[-5:]:
        float(l.split(':')[1])
    model = res['model']
    assert isinstance(model, GAT) and len(model.layers) == 2 and len(model.layers[0].heads) == 4
    assert len(res['val_accs']) == 5
    assert res['val_accs'][-1] > 1.0 / 5                         # above chance (5 classes)
    assert res['total_time'] > 0
    # the training loss falls: the trained model against the same-seed initial one on the full graph
    ds = _toy()
    g = ds.g.to(torch.device('cuda', 0))
    torch.manual_seed(0)
    init = GAT(2, g.ndata['feat'].shape[1], 32, ds.num_classes, 4).cuda()
    tm = g.ndata['train_mask'].bool()
    lab = g.ndata['label']
    with torch.no_grad():
        l0 = float(CrossEntropyLoss()(init(g)[tm], lab[tm]))
        l1 = float(CrossEntropyLoss()(model(g)[tm], lab[tm]))
    assert l1 < l0


def test_gat_cli_same_seed_bitwise_identical_weights_whatever_the_host_path():
    a, _ = _run(epochs=2)
    b, _ = _run(host_path='module', epochs=2)
    pa = list(a['model'].parameters())
    pb = list(b['model'].parameters())
    assert len(pa) == len(pb)
    for u, v in zip(pa, pb):
        assert torch.equal(u, v)
    assert a['val_accs'] == b['val_accs']
