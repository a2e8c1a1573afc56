"""CPU: GIST for the GAT family (gist_amd.ist.DistributedGATWrapper, cluster_gcn_ist_distrib_gat.py) -- dispatch and
sync under a real `gloo` process group (world sizes 2 and 4) against a float64 restatement of the reference's per-head
loops (tests/gat_ist_restatement.py), for n_layers 1, 2, 3 and n_heads 1, 3; construction in the reference's torch RNG
order over per-head views of the flat arenas; the script's flags and output contract.

The HIP block movers cannot run here: the wrapper gets a torch-indexing double (TorchBlocks); everything else is the
product code."""
import argparse
import pickle
import random

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.gat_ist_restatement import TorchBlocks, base_init_for, check_round

H, FIN, NCLS = 8, 5, 3
CONFIGS = [(L, nh) for L in (1, 2, 3) for nh in (1, 3)]


def _args(S, L, nh, rank):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_heads=nh, rank=rank, dropout=0.5,
                              use_layernorm=False)


def _worker(rank, S, port, q):
    from gist_amd import ist
    errs = []
    try:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        for ci, (L, nh) in enumerate(CONFIGS):
            dims = ist.gat_dims(FIN, H, NCLS, L, nh)
            base_init = base_init_for(dims, 100 + ci)
            w = ist.DistributedGATWrapper(_args(S, L, nh, rank), None, FIN, NCLS, torch.device('cpu'),
                                          base_init=base_init if rank == 0 else None, blocks=TorchBlocks())

            def all_base():
                out = [torch.empty_like(w.base.params) for _ in range(S)]
                dist.all_gather(out, w.base.params)
                return out
            errs += ['L=%d nh=%d: %s' % (L, nh, e)
                     for e in check_round([w], S, H, L, base_init, 7 + ci, all_base)]
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:          # surface the failure in the parent
        import traceback
        errs.append('EXC ' + repr(e) + traceback.format_exc())
    q.put((rank, errs))


@pytest.mark.parametrize('S,port', [(2, 29891), (4, 29892)])
def test_gat_dispatch_sync_gloo(S, port):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, S, port, q)) for r in range(S)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(S)]
    for p in procs:
        p.join(timeout=60)
    for rank, errs in sorted(res):
        assert errs == [], 'rank %d: %s' % (rank, errs[:8])


@pytest.mark.parametrize('L,nh', [(1, 4), (3, 3)])
@pytest.mark.parametrize('rank', [0, 1])
def test_construction_draws_the_reference_order(L, nh, rank):
    """Same seed: base_model (rank 0) and sub_model equal GAT(L, in, H, C, nh) then GAT(L, in, H/S, C, nh) drawn in
    that order; every head's parameters are views of the flat arenas."""
    from gist_amd import ist
    from gist_amd.modules import GAT
    S = 2
    torch.manual_seed(5)
    w = ist.DistributedGATWrapper(_args(S, L, nh, rank), None, FIN, NCLS, torch.device('cpu'), blocks=TorchBlocks())
    torch.manual_seed(5)
    want_base = GAT(L, FIN, H, NCLS, nh) if rank == 0 else None
    want_sub = GAT(L, FIN, H // S, NCLS, nh)
    assert (w.base_model is None) == (rank != 0)
    pairs = [(w.sub_model, want_sub, w.sub, True)] + ([(w.base_model, want_base, w.base, False)] if rank == 0 else [])
    for got, want, arena, grad in pairs:
        assert isinstance(got, GAT) and len(got.layers) == max(L, 2)
        gp, wp = dict(got.named_parameters()), dict(want.named_parameters())
        assert sorted(gp) == sorted(wp)
        for n in wp:
            assert torch.equal(gp[n], wp[n]), n
            assert gp[n].requires_grad == grad
        for k, layer in enumerate(got.layers):
            o = arena.dims[k][1]
            assert len(layer.heads) == arena.dims[k][2]
            for h, hd in enumerate(layer.heads):
                assert hd.fc.weight.data_ptr() == arena.W[k][h * o].data_ptr()
                assert hd.attn_fc.weight.data_ptr() == arena.A[k][h].data_ptr()
                assert hd.fc.weight.shape == (o, arena.dims[k][0]) and hd.attn_fc.weight.shape == (1, 2 * o)
        # in-place visibility, both ways
        before = arena.params.clone()
        arena.params.add_(1.0)
        assert torch.equal(got.layers[-1].heads[0].attn_fc.weight.detach(), before[-2 * NCLS:].view(1, -1) + 1.0)
        with torch.no_grad():
            got.layers[0].heads[-1].fc.weight.zero_()
        o0 = arena.dims[0][1]
        assert float(arena.W[0][(arena.dims[0][2] - 1) * o0:].abs().sum()) == 0.0
    assert w.sub.numel == sum(nh_ * o * i + nh_ * 2 * o for (i, o, nh_) in w.sub_dims)
    assert w.gathered.numel() == S * w.sub.numel


def test_partitions_draw_n_layers_shuffles():
    """n_layers create_partition calls per dispatch whatever the layer count (reading 4): n_layers = 2 draws a partition
    the model does not use."""
    from gist_amd import ist
    from tests.gat_ist_restatement import ref_sample
    for L in (1, 2, 3):
        w = ist.DistributedGATWrapper(_args(2, L, 2, 0), None, FIN, NCLS, torch.device('cpu'), base_init=None,
                                      blocks=TorchBlocks())
        random.seed(3)
        part = w.sample_partitions()
        state = random.getstate()
        random.seed(3)
        want = ref_sample(2, H, L)
        assert random.getstate() == state and len(part) == L
        for k in range(L):
            for s in range(2):
                assert np.array_equal(part[k][s][0].numpy(), want[k][s][0])
                assert np.array_equal(part[k][s][1].numpy(), want[k][s][1])
        assert w.n_bound == max(L, 2) - 1


REF_FLAGS = ['--dataset', 'toy', '--iter_per_site', '7', '--num_subnet', '2', '--dropout', '0.1', '--lr', '0.02',
             '--n-epochs', '4', '--n-hidden', '512', '--n-layers', '1', '--weight-decay', '0', '--use_layernorm',
             'False', '--dist-backend', 'gloo', '--dist-url', 'tcp://127.0.0.1:1234', '--rank', '1', '--cuda-id', '0',
             '--batch-size', '10', '--psize', '50', '--test-batch-size', '100', '--rnd-seed', '0', '--use-pp',
             '--normalize', '--save_results', '--n-heads', '8', '--exp_name', 'gat_sweep']


def test_cli_accepts_the_reference_flags():
    from gist_amd.scripts import cluster_gcn_ist_distrib_gat as cli
    d = cli.build_parser().parse_args([])
    assert (d.iter_per_site, d.num_subnet, d.dropout, d.lr, d.n_epochs, d.n_hidden, d.n_layers, d.weight_decay,
            d.use_layernorm, d.dist_backend, d.dist_url, d.rank, d.cuda_id, d.batch_size, d.psize,
            d.test_batch_size, d.rnd_seed, d.use_pp, d.normalize, d.save_results, d.n_heads, d.exp_name) == (
        5, 2, 0.5, 0.01, 20, 16, 1, 5e-4, False, 'nccl', 'tcp://127.0.0.1:9971', 0, 0, 20, 1500, 1000, 3, False,
        False, False, 4, 'distributed_gnn_ist')
    a = cli.build_parser().parse_args(REF_FLAGS)
    assert (a.iter_per_site, a.n_hidden, a.n_heads, a.exp_name, a.rank, a.use_pp, a.save_results) == (
        7, 512, 8, 'gat_sweep', 1, True, True)
    assert a.use_layernorm is True                       # type=bool, as in the reference
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--fig-dir', 'x'])   # not a flag of the GAT script


def test_cli_output_contract(tmp_path, monkeypatch):
    from gist_amd.scripts import cluster_gcn_ist_distrib_gat as cli
    res = dict(total_time=1.5, trn_losses=[1.2, 0.9], val_accs=[0.25, 0.5, 0.375], test_accs=[0.125, 0.75, 0.5])
    lines = []
    args = cli.build_parser().parse_args([])
    assert cli.report(args, res, log=lines.append) is None
    assert lines == ['Training Time: 1.5000', 'Last Test: 0.5000', 'Best Test: 0.7500', 'Best Val: 0.5000']
    monkeypatch.chdir(tmp_path)
    lines.clear()
    args = cli.build_parser().parse_args(['--save_results', '--exp_name', 'gat_s2'])
    path = cli.report(args, res, log=lines.append)
    assert lines == []
    assert (tmp_path / 'results' / 'gat_s2_result.pckl').exists()
    got = pickle.load(open(path, 'rb'))
    assert got == {'total_time': 1.5, 'trn_losses': [1.2, 0.9], 'val_accs': [0.25, 0.5, 0.375],
                   'test_accs': [0.125, 0.75, 0.5]}
