"""CPU: GIST for the BaselineGCN family (gist_amd.ist.DistributedBaselineGCNWrapper) -- dispatch and sync bit for bit
against the numpy restatement of its split table (tests/baseline_gcn_ist_restatement.py), all sites in one process and
under a real `gloo` process group; construction in the wrappers' torch RNG order over views of the flat arenas; what
train_baseline_gcn, the script and BaselineGCNEngine(x0=...) refuse; the script's flags; the unchanged ABI.

The HIP block movers cannot run here: the wrapper gets the torch-indexing double (TorchBlocks), which also selects the
per-tensor mover calls; everything else is the product code."""
import argparse
import os
import random
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.baseline_gcn_ist_restatement import TorchBlocks, base_init_for, check_round
from tests.test_graphsage_ist import ROOT

FIN, NCLS = 7, 5
CPU = torch.device('cpu')


def _args(S, H, L, rank, dropout=0.5, use_layernorm=True):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=rank, dropout=dropout,
                              use_layernorm=use_layernorm)


def local_wrappers(S, H, L, device, base_init, blocks, fin=FIN, ncls=NCLS, **kw):
    from gist_amd import ist
    grp = ist.LocalCommGroup(S)
    return [ist.DistributedBaselineGCNWrapper(_args(S, H, L, s, **kw), None, fin, ncls, device,
                                              base_init=base_init if s == 0 else None,
                                              blocks=blocks() if blocks else None, comm=grp.handle(s)) for s in range(S)]


@pytest.mark.parametrize('h', [4, 6])            # 6: no row of a sub weight is a multiple of 16 bytes
@pytest.mark.parametrize('L', [1, 2, 3])
@pytest.mark.parametrize('S', [2, 4])
def test_round_against_the_restatement(S, L, h):
    from gist_amd.arena import BaselineGCNArena, baseline_gcn_dims
    H = S * h
    base_init = base_init_for(baseline_gcn_dims(FIN, H, NCLS, L), 40 + L)
    ws = local_wrappers(S, H, L, CPU, base_init, TorchBlocks)
    assert not any(w.grouped for w in ws) and type(ws[0]).GROUPED
    assert [tuple(d) for d in ws[0].sub_dims] == baseline_gcn_dims(FIN, h, NCLS, L)
    assert [tuple(d) for d in ws[0].base_dims] == baseline_gcn_dims(FIN, H, NCLS, L)
    assert all(isinstance(a, BaselineGCNArena) for w in ws for a in (w.base, w.sub))
    assert all(o % 4 == 0 for w in ws for offs in w.sub.offsets for o in offs)       # every view on 16 bytes
    errs = check_round(ws, S, H, L, base_init, 11 + L, lambda: [w.base.params for w in ws])
    assert errs == [], errs[:8]


def test_the_split_table():
    """The plan of a site, read off the wrapper: rows / columns / bias indices per layer are the issue's table."""
    from gist_amd import ist
    S, H, L = 2, 8, 3
    w = ist.DistributedBaselineGCNWrapper(_args(S, H, L, 1), None, FIN, NCLS, CPU, base_init=None, blocks=TorchBlocks(),
                                          comm=ist.LocalCommGroup(S).handle(1))
    random.seed(1)
    part = w.sample_partitions()
    idx = [part[k][1][0] for k in range(L)]
    plan = w._site_plan(part, 1)
    assert len(plan) == L + 1
    assert plan[0][0] is None and plan[0][1] is idx[0] and plan[0][2] is idx[0]
    for k in (1, 2):
        assert plan[k][0] is idx[k - 1] and plan[k][1] is idx[k] and plan[k][2] is idx[k]
    assert plan[L][0] is idx[L - 1] and plan[L][1] is None and plan[L][2] is None


def _worker(rank, S, port, q):
    from gist_amd import ist
    from gist_amd.arena import baseline_gcn_dims
    errs = []
    try:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        for L, h in ((1, 6), (2, 4), (3, 6)):
            H = S * h
            base_init = base_init_for(baseline_gcn_dims(FIN, H, NCLS, L), 70 + L)
            w = ist.DistributedBaselineGCNWrapper(_args(S, H, L, rank), None, FIN, NCLS, CPU,
                                                  base_init=base_init if rank == 0 else None, blocks=TorchBlocks())

            def all_base():
                out = [torch.empty_like(w.base.params) for _ in range(S)]
                dist.all_gather(out, w.base.params)
                return out
            # two rounds (dispatch, train, sync; re-dispatch, train, sync), the replicas compared after each sync
            errs += ['L=%d: %s' % (L, e) for e in check_round([w], S, H, L, base_init, 5 + L, all_base)]
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:          # surface the failure in the parent
        import traceback
        errs.append('EXC ' + repr(e) + traceback.format_exc())
    q.put((rank, errs))


def test_dispatch_sync_gloo():
    S, port = 2, 29941
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


@pytest.mark.parametrize('use_layernorm', [True, False])
@pytest.mark.parametrize('rank', [0, 1])
def test_construction_draws_the_wrappers_order(rank, use_layernorm):
    """Same seed: base_model (rank 0) and sub_model equal BaselineGCN(in, H, ...) then BaselineGCN(in, H/S, ...) drawn in
    that order; every Parameter is a view of the flat arenas under its own name."""
    import torch.nn.functional as F
    from gist_amd import ist
    from gist_amd.modules import BaselineGCN
    S, H, L = 2, 12, 2
    torch.manual_seed(5)
    w = ist.DistributedBaselineGCNWrapper(_args(S, H, L, rank, use_layernorm=use_layernorm), None, FIN, NCLS, CPU,
                                          blocks=TorchBlocks(), seed=3)
    torch.manual_seed(5)
    want_base = BaselineGCN(FIN, H, NCLS, L, F.relu, 0.5, use_layernorm) if rank == 0 else None
    want_sub = BaselineGCN(FIN, H // S, NCLS, L, F.relu, 0.5, use_layernorm)
    assert (w.base_model is None) == (rank != 0)
    pairs = [(w.sub_model, want_sub, w.sub, True)] + ([(w.base_model, want_base, w.base, False)] if rank == 0 else [])
    keys = [n for k in range(L + 1) for n in ('layers.%d.weight' % k, 'layers.%d.bias' % k)]
    for got, want, arena, grad in pairs:
        assert isinstance(got, BaselineGCN) and len(got.layers) == L + 1 and got.use_layernorm == use_layernorm
        gp, wp = dict(got.named_parameters()), dict(want.named_parameters())
        assert list(gp) == list(wp) == keys and list(got.state_dict()) == list(want.state_dict()) == keys
        for n in wp:
            assert torch.equal(gp[n], wp[n]), n
            assert gp[n].requires_grad == grad
        assert [p.data_ptr() for p in got.parameters()] == [v.data_ptr() for v in arena.param_views()]
        assert got.__dict__['_gist_arena']() is arena
        before = arena.params.clone()
        arena.params.add_(1.0)                       # in-place visibility: no copy
        assert torch.equal(got.layers[-1].bias.detach(), before[arena.offsets[-1][1]:][:NCLS] + 1.0)
    assert w.sub_model.drop_seed == 3 * 131 + rank
    assert w.gathered.numel() == S * w.sub.numel and w.engine is None


def test_base_init_draws_nothing():
    from gist_amd import ist
    from gist_amd.arena import baseline_gcn_dims
    torch.manual_seed(9)
    state = torch.get_rng_state()
    w1 = ist.DistributedBaselineGCNWrapper(_args(2, 8, 2, 1), None, FIN, NCLS, CPU, base_init=None, blocks=TorchBlocks())
    assert torch.equal(torch.get_rng_state(), state)
    base_init = base_init_for(baseline_gcn_dims(FIN, 8, NCLS, 2), 3)
    torch.manual_seed(9)
    w0 = ist.DistributedBaselineGCNWrapper(_args(2, 8, 2, 0), None, FIN, NCLS, CPU, base_init=base_init,
                                           blocks=TorchBlocks())
    assert torch.equal(torch.get_rng_state(), state)
    assert w1.base_model is None and not w1.base.params.any() and not w1.sub.params.any()
    for k, (W, b) in enumerate(base_init):
        assert torch.equal(w0.base_model.layers[k].weight.detach(), W) and torch.equal(w0.base.b[k], b)
    assert list(w0.sub_model.state_dict()) == [n for k in range(3) for n in ('layers.%d.weight' % k, 'layers.%d.bias' % k)]
    assert [p.data_ptr() for p in w0.sub_model.parameters()] == [v.data_ptr() for v in w0.sub.param_views()]


def test_partitions_draw_n_layers_shuffles():
    from gist_amd import ist
    for L in (1, 3):
        S, H = 2, 12
        w = ist.DistributedBaselineGCNWrapper(_args(S, H, L, 0), None, FIN, NCLS, CPU, base_init=None,
                                              blocks=TorchBlocks())
        random.seed(3)
        part = w.sample_partitions()
        state = random.getstate()
        random.seed(3)
        want = [ist.create_partition(S, H) for _ in range(L)]
        assert random.getstate() == state and len(part) == L
        for k in range(L):
            for s in range(S):
                assert torch.equal(part[k][s][0], want[k][s][0]) and torch.equal(part[k][s][1], want[k][s][1])


class _OtherIter(object):
    """Not a sampler class."""
    n_max = 8


def test_train_baseline_gcn_refuses_what_it_cannot_run():
    from gist_amd import ist
    w = ist.DistributedBaselineGCNWrapper(_args(2, 8, 1, 0), None, FIN, NCLS, CPU, base_init=None, blocks=TorchBlocks())
    for bad in ('engine', 'phases'):
        with pytest.raises(ValueError, match="host_path must be 'module' or 'step'.*%s" % bad):
            ist.train_baseline_gcn(w, None, None, [], None, None, None, host_path=bad)
    with pytest.raises(ValueError, match="host_path='step'.*GPU-only"):
        ist.train_baseline_gcn(w, None, None, [], None, None, None, host_path='step')
    # the module loop too: the model's forward is torch.ops.gist.*, registered for the GPU alone (no CPU fallback)
    with pytest.raises(ValueError, match="host_path='module'.*GPU-only"):
        ist.train_baseline_gcn(w, None, None, [], None, None, None, host_path='module')
    with pytest.raises(TypeError):
        ist.train_baseline_gcn(w, None, None, [], None, None, None, eval_path='layers')
    # the iterator's class is looked at before anything touches the device: a stand-in that says it is on a GPU
    on_gpu = types.SimpleNamespace(device=torch.device('cuda', 0))
    with pytest.raises(ValueError, match="host_path='step'.*EngineClusterIter.*_OtherIter"):
        ist.train_baseline_gcn(on_gpu, None, None, _OtherIter(), None, None, None, host_path='step')
    with pytest.raises(ValueError, match="host_path='module'.*ClusterIter.*_OtherIter"):
        ist.train_baseline_gcn(on_gpu, None, None, _OtherIter(), None, None, None, host_path='module')


def test_script_refusals():
    from gist_amd.scripts import cluster_gcn_ist_distrib_baseline as cli
    with pytest.raises(SystemExit, match='--use-pp'):
        cli.main(cli.build_parser().parse_args(['--use-pp']), log=lambda *a, **k: None)
    with pytest.raises(SystemExit, match='--cuda-id'):
        cli.main(cli.build_parser().parse_args(['--cuda-id', '-1']), log=lambda *a, **k: None)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--host-path', 'phases'])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--eval-path', 'rows'])


@pytest.mark.parametrize('what,x0', [
    ('rows', lambda: torch.zeros(9, 7, device='meta')),
    ('columns', lambda: torch.zeros(8, 6, device='meta')),
    ('rank', lambda: torch.zeros(8 * 7, device='meta')),
    ('dtype', lambda: torch.zeros(8, 7, dtype=torch.float64, device='meta')),
    ('device', lambda: torch.zeros(8, 7)),
    ('not contiguous', lambda: torch.zeros(7, 8, device='meta').t()),
    ('not a tensor', lambda: [[0.0] * 7] * 8),
])
def test_engine_refuses_a_bad_x0(what, x0):
    """The check runs before anything is allocated or loaded: a meta tensor stands for a GPU one of the same kind, so the
    device named to the engine is 'meta' here (and a CPU tensor is then the one on the wrong device)."""
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    with pytest.raises(ValueError, match=r'shared x0 must be a contiguous fp32 \[8, 7\] tensor'):
        BaselineGCNEngine([(7, 4), (4, 5)], True, 0.0, 8, torch.device('meta'), x0=x0())
    # the neighbouring valid tensor is adopted as layer 0's input, and without x0 the engine allocates its own
    good = torch.zeros(8, 7, device='meta')
    engine = BaselineGCNEngine([(7, 4), (4, 5)], True, 0.0, 8, torch.device('meta'), x0=good)
    assert engine.X[0] is good and engine.z0_left(3).shape == (3, 7)
    own = BaselineGCNEngine([(7, 4), (4, 5)], True, 0.0, 8, torch.device('meta'))
    assert own.X[0] is not good and own.X[0].shape == (8, 7)


def test_cli_flags_and_output_contract(tmp_path, monkeypatch):
    import pickle
    from gist_amd import ist
    from gist_amd.scripts import cluster_gcn_ist_distrib_baseline as cli
    d = cli.build_parser().parse_args([])
    assert (d.host_path, d.use_pp, d.iter_per_site, d.num_subnet, d.use_layernorm, d.exp_name, d.save_results) == (
        'module', False, 5, 2, False, 'distributed_gnn_ist', False)
    assert not hasattr(d, 'eval_path')
    a = cli.build_parser().parse_args(['--host-path', 'step', '--use_layernorm', 'True', '--num_subnet', '4', '--n-hidden',
                                       '512', '--rank', '1'])
    assert (a.host_path, a.use_layernorm, a.num_subnet, a.n_hidden, a.rank) == ('step', True, 4, 512, 1)
    res = dict(total_time=1.5, trn_losses=[1.2, 0.9], val_accs=[0.25, 0.5, 0.375], test_accs=[0.125, 0.75, 0.5])
    lines = []
    assert cli.report(d, res, log=lines.append) is None
    assert lines == ['Training Time: 1.5000', 'Last Val: 0.3750', 'Best Val: 0.5000', 'Last Test: 0.5000',
                     'Best Test: 0.7500']
    monkeypatch.chdir(tmp_path)
    a = cli.build_parser().parse_args(['--save_results', '--exp_name', 'bl_s2'])
    path = cli.report(a, res, log=lines.append)
    assert len(lines) == 5 and (tmp_path / 'results' / 'bl_s2_result.pckl').exists()
    assert pickle.load(open(path, 'rb')) == res

    # main() end to end with the set-up, the iterator, the wrapper and the loop stood in for: what it hands to
    # train_baseline_gcn, and that rank 0 reports what the loop returned
    seen = {}

    class Wrapper(object):
        def __init__(self, args, g, in_feats, n_classes, device, comm=None, seed=0):
            seen['wrapper'] = (args.use_layernorm, in_feats, n_classes, seed)

        def ini_sync_dispatch_model(self):
            seen['dispatched'] = True

    def fake_train(ist_model, args, g, it, labels, val_mask, test_mask, log=print, host_path='module'):
        seen['train'] = (type(ist_model).__name__, type(it).__name__, host_path)
        return dict(res, losses=[[]], events=[])

    class G(object):
        ndata = dict(label=None, val_mask=None, test_mask=None)

        def to(self, device):
            return self

    class It(object):
        def __init__(self, *a, **k):
            seen['iter'] = sorted(k)
    import gist_amd.sampler as sampler
    monkeypatch.setattr(ist, 'DistributedBaselineGCNWrapper', Wrapper)
    monkeypatch.setattr(ist, 'train_baseline_gcn', fake_train)
    monkeypatch.setattr(sampler, 'EngineClusterIter', It)
    monkeypatch.setattr(cli, 'setup', lambda args, dataset, log: ('dev', None, G(), 32, 5, None, None, 3))
    monkeypatch.setattr(cli.dist, 'destroy_process_group', lambda: None)
    lines = []
    args = cli.build_parser().parse_args(['--host-path', 'step', '--use_layernorm', 'True', '--rnd-seed', '7'])
    out = cli.main(args, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert seen['wrapper'] == (True, 32, 5, 7) and seen['dispatched'] and seen['train'] == ('Wrapper', 'It', 'step')
    assert 'use_pp' not in seen['iter']
    assert [l.split(':')[0] for l in lines[-5:]] == ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
    assert isinstance(out['model'], Wrapper)


def test_abi_is_unchanged():
    """ABI 16, and the header declares the 81 launching exports it declared before: this feature adds no entry point."""
    from gist_amd import _lib, ist
    L = _lib.load()
    assert L.gist_abi_version() == 16
    from tests.test_scratch_guard import header_exports
    from tests.test_stream_order_coverage import stream_exports
    exports = header_exports()
    assert len(stream_exports(exports)) == 81
    # every declared function was bound before this feature: none is new (the bindings' table is unchanged too)
    assert set(exports) <= set(_lib.SIGNATURES), sorted(set(exports) - set(_lib.SIGNATURES))
    assert not [n for n in exports if 'baseline_gcn' in n and n not in (
        'gist_baseline_gcn_step', 'gist_baseline_gcn_step_workspace_bytes', 'gist_baseline_gcn_step_tail_ws_floats')]
    header = open(os.path.join(ROOT, 'include', 'gist_hip.h')).read()
    assert 'gist_baseline_gcn_step_phase' not in header
    assert callable(ist.train_baseline_gcn) and ist.DistributedBaselineGCNWrapper.GROUPED
