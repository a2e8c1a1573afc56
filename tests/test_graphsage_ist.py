"""CPU: GIST for the GraphSAGE family (gist_amd.ist.DistributedGraphSAGEWrapper) -- dispatch and sync against the numpy
float64 restatement of its split table (tests/graphsage_ist_restatement.py), all sites in one process and under a real
`gloo` process group; construction in the wrappers' torch RNG order over views of the flat arenas; the host-only table
packer of the grouped mover (gist_arena_moves_pack) with every rejection it documents; the script's flags.

The HIP block movers cannot run here: the wrapper gets the torch-indexing double (TorchBlocks), which also selects the
per-tensor mover calls; everything else is the product code."""
import argparse
import ctypes
import os
import random

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.graphsage_ist_restatement import TorchBlocks, base_init_for, check_round

H, FIN, NCLS = 16, 12, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(S, L, rank, use_pp=False, dropout=0.5):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=rank, dropout=dropout, use_layernorm=True,
                              use_pp=use_pp)


def local_wrappers(S, L, use_pp, device, base_init, blocks):
    from gist_amd import ist
    grp = ist.LocalCommGroup(S)
    return [ist.DistributedGraphSAGEWrapper(_args(S, L, s, use_pp), None, FIN, NCLS, device,
                                            base_init=base_init if s == 0 else None, blocks=blocks() if blocks else None,
                                            comm=grp.handle(s)) for s in range(S)]


@pytest.mark.parametrize('use_pp', [False, True])
@pytest.mark.parametrize('L', [1, 2, 3])
@pytest.mark.parametrize('S', [2, 4])
def test_round_against_the_restatement(S, L, use_pp):
    from gist_amd.arena import graphsage_dims
    base_init = base_init_for(graphsage_dims(FIN, H, NCLS, L), 40 + L)
    ws = local_wrappers(S, L, use_pp, torch.device('cpu'), base_init, TorchBlocks)
    assert not any(w.grouped for w in ws)
    assert [tuple(d) for d in ws[0].sub_dims] == graphsage_dims(FIN, H // S, NCLS, L)
    errs = check_round(ws, S, H, L, base_init, 11 + L, lambda: [w.base.params for w in ws])
    assert errs == [], errs[:8]


def _worker(rank, S, port, q):
    from gist_amd import ist
    from gist_amd.arena import graphsage_dims
    errs = []
    try:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        for L, use_pp in ((1, False), (2, True), (3, False)):
            base_init = base_init_for(graphsage_dims(FIN, H, NCLS, L), 70 + L)
            w = ist.DistributedGraphSAGEWrapper(_args(S, L, rank, use_pp), None, FIN, NCLS, torch.device('cpu'),
                                                base_init=base_init if rank == 0 else None, blocks=TorchBlocks())

            def all_base():
                out = [torch.empty_like(w.base.params) for _ in range(S)]
                dist.all_gather(out, w.base.params)
                return out
            errs += ['L=%d: %s' % (L, e) for e in check_round([w], S, H, L, base_init, 5 + L, all_base)]
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:          # surface the failure in the parent
        import traceback
        errs.append('EXC ' + repr(e) + traceback.format_exc())
    q.put((rank, errs))


def test_dispatch_sync_gloo():
    S, port = 2, 29913
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


@pytest.mark.parametrize('rank', [0, 1])
@pytest.mark.parametrize('use_pp', [False, True])
def test_construction_draws_the_wrappers_order(rank, use_pp):
    """Same seed: base_model (rank 0) and sub_model equal GraphSAGE(in, H, ...) then GraphSAGE(in, H/S, ...) drawn in that
    order; every Parameter is a view of the flat arenas under its own name."""
    import torch.nn.functional as F
    from gist_amd import ist
    from gist_amd.modules import GraphSAGE
    S, L = 2, 2
    torch.manual_seed(5)
    w = ist.DistributedGraphSAGEWrapper(_args(S, L, rank, use_pp), None, FIN, NCLS, torch.device('cpu'),
                                        blocks=TorchBlocks())
    torch.manual_seed(5)
    want_base = GraphSAGE(FIN, H, NCLS, L, F.relu, 0.5, use_pp) if rank == 0 else None
    want_sub = GraphSAGE(FIN, H // S, NCLS, L, F.relu, 0.5, use_pp)
    assert (w.base_model is None) == (rank != 0)
    pairs = [(w.sub_model, want_sub, w.sub, True)] + ([(w.base_model, want_base, w.base, False)] if rank == 0 else [])
    for got, want, arena, grad in pairs:
        assert isinstance(got, GraphSAGE) and len(got.layers) == L + 1
        gp, wp = dict(got.named_parameters()), dict(want.named_parameters())
        assert list(gp) == list(wp) and sorted(got.state_dict()) == sorted(want.state_dict())
        for n in wp:
            assert torch.equal(gp[n], wp[n]), n
            assert gp[n].requires_grad == grad
        views = arena.param_views()
        assert [p.data_ptr() for p in got.parameters()] == [v.data_ptr() for v in views]
        assert got.layers[0].use_pp == use_pp and not got.layers[1].use_pp
        before = arena.params.clone()
        arena.params.add_(1.0)                       # in-place visibility
        assert torch.equal(got.layers[-1].linear.bias.detach(), before[arena.offsets[-1][1]:][:NCLS] + 1.0)
    assert w.gathered.numel() == S * w.sub.numel and w.engine is None


def test_train_graphsage_refuses_what_it_cannot_run():
    from gist_amd import ist
    w = ist.DistributedGraphSAGEWrapper(_args(2, 1, 0), None, FIN, NCLS, torch.device('cpu'), base_init=None,
                                        blocks=TorchBlocks())
    with pytest.raises(ValueError, match='host_path'):
        ist.train_graphsage(w, None, None, [], None, None, None, host_path='engine')
    with pytest.raises(ValueError, match='eval_path'):
        ist.train_graphsage(w, None, None, [], None, None, None, eval_path='blocked')
    with pytest.raises(ValueError, match='GPU-only'):
        ist.train_graphsage(w, None, None, [], None, None, None, host_path='step')
    # the module loop too: the model's forward is torch.ops.gist.*, registered for the GPU alone (no CPU fallback)
    with pytest.raises(ValueError, match="host_path='module'.*GPU-only"):
        ist.train_graphsage(w, None, None, [], None, None, None, host_path='module')


# -- the grouped mover's host side ---------------------------------------------------------------------------------------
NAMES = ('gist_arena_moves_packed_bytes', 'gist_arena_moves_pack', 'gist_arena_moves_f32')


def test_new_symbols_are_exported():
    from gist_amd import _lib, hip, ist
    L = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'gist_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name + '(' in header, name
    assert 'struct gist_arena_move {' in header and L.gist_abi_version() == 16
    assert ctypes.sizeof(_lib.ArenaMove) == 72
    assert callable(hip.arena_moves) and callable(ist.train_graphsage)
    assert ist.DistributedGraphSAGEWrapper.GROUPED and not ist.DistributedGNNWrapper.GROUPED
    assert not ist.DistributedGATWrapper.GROUPED


def _pack(moves, src_numel=1000, dst_numel=1000, idx_len=64, out_bytes=None):
    """-> (rc, n_tiles, message)"""
    from gist_amd import _lib
    L = _lib.load()
    arr = (_lib.ArenaMove * max(len(moves), 1))()
    for a, m in zip(arr, moves):
        for f, v in m.items():
            setattr(a, f, v)
    need = L.gist_arena_moves_packed_bytes(len(moves))
    buf = ctypes.create_string_buffer(max(need, 16) + 64)
    tiles = ctypes.c_int64(-7)
    rc = L.gist_arena_moves_pack(arr, len(moves), src_numel, dst_numel, idx_len, buf,
                                 need if out_bytes is None else out_bytes, ctypes.byref(tiles))
    return rc, tiles.value, (L.gist_last_error() or b'').decode()


def _move(**kw):
    m = dict(src_off=0, dst_off=0, lds=10, ldd=10, n_rows=4, n_cols=10, row_idx=-1, col_idx=-1, kind=0)
    m.update(kw)
    return m


def test_pack_round_trips_a_valid_table():
    from gist_amd import _lib
    L = _lib.load()
    assert L.gist_arena_moves_packed_bytes(-1) < 0
    assert L.gist_arena_moves_packed_bytes(0) >= 4 and L.gist_arena_moves_packed_bytes(3) >= 3 * 64 + 16
    assert _pack([])[:2] == (0, 0)
    # tiles: 8 rows x 1024 columns per gather / scatter tile, 256 columns per mean tile; an empty move has none
    moves = [_move(),                                                             # 4 x 10: 1
             _move(n_rows=0),                                                     # nothing
             _move(kind=1, n_rows=9, n_cols=5, row_idx=3, col_idx=12, ldd=7),     # 9 x 5 scatter: 2 row groups
             _move(kind=2, n_rows=3, n_cols=257, lds=300, src_off=1, dst_off=5),  # mean of 257: 2
             _move(n_rows=1, n_cols=0),
             _move(src_off=0, lds=2000, ldd=1025, n_rows=17, n_cols=1025, col_idx=0, row_idx=0)]      # 3 x 2
    rc, tiles, msg = _pack(moves, src_numel=40000, dst_numel=20000, idx_len=1025)
    assert (rc, tiles) == (0, 1 + 0 + 2 + 2 + 0 + 6), msg


@pytest.mark.parametrize('what,moves,kw,code,text', [
    ('negative rows', [_move(n_rows=-1)], {}, -1, 'negative size'),
    ('negative cols', [_move(), _move(n_cols=-2)], {}, -1, 'move 1: negative size'),
    ('rows >= 2^31', [_move(n_rows=1 << 31)], {}, -1, '2^31'),
    ('unknown kind', [_move(kind=3)], {}, -1, 'unknown kind'),
    ('negative offset', [_move(dst_off=-1)], {}, -1, 'negative offset'),
    ('gather: dst pitch < block', [_move(ldd=9)], {}, -1, 'dst pitch'),
    ('gather: src pitch < block, identity columns', [_move(lds=9, row_idx=0)], {}, -1, 'src pitch'),
    ('scatter: src pitch < block', [_move(kind=1, lds=9)], {}, -1, 'src pitch'),
    ('scatter: dst pitch < block, identity columns', [_move(kind=1, ldd=9, row_idx=0)], {}, -1, 'dst pitch'),
    ('gather: dst extent', [_move(dst_off=961)], {}, -1, 'past dst_numel'),
    ('gather: src extent, identity', [_move(src_off=961)], {}, -1, 'past src_numel'),
    ('gather: src extent, identity rows only', [_move(src_off=970, col_idx=0)], {}, -1, 'past src_numel'),
    ('gather: src extent, identity columns only', [_move(src_off=991, row_idx=0)], {}, -1, 'past src_numel'),
    ('scatter: dst extent', [_move(kind=1, dst_off=961)], {}, -1, 'past dst_numel'),
    ('scatter: src extent', [_move(kind=1, src_off=961)], {}, -1, 'past src_numel'),
    ('row list past the pool', [_move(row_idx=61)], {}, -1, 'row index list'),
    ('column list past the pool', [_move(col_idx=55)], {}, -1, 'column index list'),
    ('index start below -1', [_move(col_idx=-2)], {}, -1, 'below -1'),
    ('mean with a list', [_move(kind=2, row_idx=0)], {}, -1, 'no index lists'),
    ('mean of no sources', [_move(kind=2, n_rows=0)], {}, -1, 'no sources'),
    ('mean: sources past the arena', [_move(kind=2, lds=400, n_rows=4, n_cols=10, src_off=0)], {'src_numel': 1209}, -1,
     'past src_numel'),
    ('mean: dst extent', [_move(kind=2, dst_off=991)], {}, -1, 'past dst_numel'),
    ('table buffer too small', [_move()], {'out_bytes': 64}, -3, 'out_bytes'),
])
def test_pack_rejections(what, moves, kw, code, text):
    rc, tiles, msg = _pack(moves, **kw)
    assert rc == code and text in msg, (what, rc, msg)
    # the neighbouring valid table is accepted: the rejection is this defect's
    assert _pack([_move()])[0] == 0


def test_pack_accepts_the_edges_of_every_rejection():
    assert _pack([_move(dst_off=960, src_off=960)])[0] == 0
    assert _pack([_move(row_idx=60, col_idx=54)])[0] == 0
    assert _pack([_move(src_off=999, row_idx=0, col_idx=0)])[0] == 0          # two lists: only the first cell is known
    assert _pack([_move(kind=2, lds=400, n_rows=4, src_off=0)], src_numel=1210)[0] == 0
    assert _pack([_move(kind=2, dst_off=990)])[0] == 0
    assert _pack([_move(n_rows=0, ldd=1, lds=1, dst_off=5000)])[0] == 0       # an empty move touches nothing


def test_cli_flags_and_output_contract(tmp_path, monkeypatch):
    import pickle
    from gist_amd.scripts import cluster_gcn_ist_distrib_graphsage as cli
    d = cli.build_parser().parse_args([])
    assert (d.host_path, d.eval_path, d.use_pp, d.iter_per_site, d.num_subnet, d.use_layernorm) == (
        'module', 'layers', False, 5, 2, False)
    a = cli.build_parser().parse_args(['--host-path', 'step', '--eval-path', 'rows', '--use-pp', '--use_layernorm', 'True',
                                       '--num_subnet', '4', '--n-hidden', '512', '--rank', '1'])
    assert (a.host_path, a.eval_path, a.use_pp, a.use_layernorm, a.num_subnet) == ('step', 'rows', True, True, 4)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--host-path', 'engine'])
    res = dict(total_time=1.5, trn_losses=[1.2, 0.9], val_accs=[0.25, 0.5, 0.375], test_accs=[0.125, 0.75, 0.5])
    lines = []
    assert cli.report(d, res, log=lines.append) is None
    assert lines == ['Training Time: 1.5000', 'Last Val: 0.3750', 'Best Val: 0.5000', 'Last Test: 0.5000',
                     'Best Test: 0.7500']
    monkeypatch.chdir(tmp_path)
    a = cli.build_parser().parse_args(['--save_results', '--exp_name', 'gs_s2'])
    path = cli.report(a, res, log=lines.append)
    assert len(lines) == 5 and (tmp_path / 'results' / 'gs_s2_result.pckl').exists()
    assert pickle.load(open(path, 'rb')) == res


def test_partitions_draw_n_layers_shuffles():
    from gist_amd import ist
    from tests.gat_ist_restatement import ref_sample
    import numpy as np
    for L in (1, 3):
        w = ist.DistributedGraphSAGEWrapper(_args(2, L, 0), None, FIN, NCLS, torch.device('cpu'), base_init=None,
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
