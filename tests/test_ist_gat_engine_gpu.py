"""GPU: gist_amd.ist.train_gat(host_path='engine') -- every site's step one gist_gat_step call on its wrapper's
GATEngine -- against host_path='module', the reference's loop on the drop-in classes.  The engine issues the module
path's launches in its order on its layouts, so every comparison is bitwise: events, per-iteration losses, accuracies,
mean training losses, every sub arena and the base arena.  No tolerance anywhere.

1. S sites in one process (LocalCommGroup): the sites share one extracted batch.  Sub widths 8 per head (the kernels'
   scalar lane layout) and 16 per head (vec4); n_layers 2 and 3 (3: a middle layer, rows and columns both partitioned);
   both head merges; with and without weight decay.
2. One process per rank (S = 2 on the one GPU, the collective host-staged over gloo): the single-site path with the next
   batch extracted by the optimiser launch; rank r equals site r of the module-path run of 1.
At most 2 child processes use the GPU at once.

Graph and schedule: tests/ist_gat_engine_common.py."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import ist_gat_engine_common as common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'ist_gat_engine_worker.py')
DEV = torch.device('cuda', 0)


def _local_run(host_path, S, H, L, nh, merge, wd):
    from gist_amd import ist
    ds = common.dataset()
    it = common.iterator(host_path, ds, DEV)
    fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
    group = ist.LocalCommGroup(S)
    init = common.base_init(ds, S, H, L, nh, merge)
    ws = [ist.DistributedGATWrapper(common.site_args(S, H, L, nh, merge, wd, r), None, fin, ncls, DEV,
                                    base_init=init if r == 0 else None, comm=group.handle(r)) for r in range(S)]
    out = common.run(host_path, ws, ds, it, DEV)
    out['wrappers'], out['iterator'] = ws, it
    return out


@functools.lru_cache(maxsize=None)
def _module_reference(S, H, L, nh, merge, wd):
    """The module-path run of a configuration: computed once, shared by the tests that compare against it."""
    out = _local_run('module', S, H, L, nh, merge, wd)
    del out['wrappers'], out['iterator']
    return out


def _assert_same_run(got, want, what):
    assert got['events'] == want['events'], what
    assert len(got['losses']) == len(want['losses'])
    for s, (a, b) in enumerate(zip(got['losses'], want['losses'])):
        assert a.shape == b.shape and a.numel() > 0
        assert torch.equal(a, b), '%s: losses of site %d: %r != %r' % (what, s, a.tolist(), b.tolist())
    assert got['loss_shapes'] == want['loss_shapes'], what
    for key in ('val_accs', 'test_accs', 'trn_losses'):
        assert len(got[key]) > 0
        assert torch.equal(torch.tensor(got[key], dtype=torch.float64), torch.tensor(want[key], dtype=torch.float64)), \
            '%s: %s %r != %r' % (what, key, got[key], want[key])


@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('merge', ['mean', 'cat'])
@pytest.mark.parametrize('L', [2, 3])
@pytest.mark.parametrize('S,H,nh', [(2, 16, 2), (4, 64, 4)])
def test_sites_of_one_process_bitwise_equal_to_the_module_path(S, H, nh, L, merge, wd):
    what = 'S=%d H=%d heads=%d L=%d %s wd=%g' % (S, H, nh, L, merge, wd)
    want = _module_reference(S, H, L, nh, merge, wd)
    got = _local_run('engine', S, H, L, nh, merge, wd)
    ws, it = got['wrappers'], got['iterator']
    # the schedule the shapes were chosen for: 2 local epochs of 4 uneven batches, periods of 3 iterations that straddle
    # the epoch boundary (syncs after iterations 3, 6 and the forced one after 8), the re-dispatch before iteration 7
    ev = want['events']
    assert len(it) == 4 and ev.count('step') == 8 and ev.count('dispatch') == 1 and ev.count('sync') == 3
    assert ev[-3:] == ['step', 'sync', 'eval'] and ev.index('dispatch') > ev.index('sync')
    sizes = [int(it._offsets[j + 1] - it._offsets[j]) for j in range(4)]
    assert len(set(sizes)) > 1 and any(n % 4 for n in sizes) and max(sizes) <= it.n_max
    assert ws[0].sub_dims[0][1] == H // S
    _assert_same_run(got, want, what)
    assert len(got['losses']) == S and all(l.numel() == 8 for l in got['losses'])
    for s in range(S):
        assert torch.equal(got['subs'][s], want['subs'][s]), '%s: sub arena of site %d' % (what, s)
        assert torch.equal(got['bases'][s], want['bases'][s]), '%s: base replica of site %d' % (what, s)
        assert torch.equal(got['bases'][s], got['bases'][0])
    assert torch.isfinite(got['bases'][0]).all() and not torch.equal(got['subs'][0], got['subs'][1])
    # one engine per wrapper over the adopted sub arena; sub_model and base_model still view the arenas
    assert got['aliases'] and want['aliases']
    for w in ws:
        assert w.engine is not None and w.engine.arena is w.sub and not w.engine.prefetch
        assert w.engine.X0 is ws[0].engine.X0                       # the sites share the extracted batch
        assert w.engine.merge == merge
    assert it.engine is ws[0].engine


def test_one_process_per_rank_bitwise_equal_to_the_sites_of_the_module_path(tmp_path):
    S, H, L, nh, merge, wd = 2, 16, 3, 2, 'mean', 5e-4
    want = _module_reference(S, H, L, nh, merge, wd)
    outs = [str(tmp_path / ('rank%d.pt' % r)) for r in range(S)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(S), '29896', outs[r], str(H), str(L), str(nh), merge,
                               repr(wd)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(S)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r in range(S):
        assert os.path.exists(outs[r]), 'rank %d wrote no result:\n%s' % (r, logs[r][-1500:])
        got = torch.load(outs[r])
        assert got['errors'] == [], 'rank %d: %s' % (r, got['errors'])
        assert got['prefetch'] and got['arena_adopted'] and got['aliases']
        assert got['events'] == want['events']
        assert len(got['losses']) == 1
        assert torch.equal(got['losses'][0], want['losses'][r]), 'rank %d: %r != %r' % (
            r, got['losses'][0].tolist(), want['losses'][r].tolist())
        assert torch.equal(got['subs'][0], want['subs'][r]), 'rank %d: sub arena' % r
        assert torch.equal(got['bases'][0], want['bases'][0]), 'rank %d: base replica' % r
        if r == 0:
            for key in ('val_accs', 'test_accs', 'trn_losses'):
                assert got[key] == want[key] and len(got[key]) > 0, key
    assert all(p.returncode == 0 for p in procs)
