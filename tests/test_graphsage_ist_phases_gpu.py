"""GPU: train_graphsage(host_path='phases') -- the reference's loop body on every site's `sub_model`, bound to the
iterator (module_engine.bind_graphsage) -- against host_path='step', the one-call step on the same wrappers' engines: 2
sites in this process on the toy graph, dropout 0.2.  The schedule is tests/graphsage_ist_step_check.py's (6 iterations
per epoch, iter_per_site 5, 2 local epochs: syncs at 5, 10 and 12, a re-dispatch at 10), so dispatch and sync write the
sub arenas between bound steps.  Every site's step losses and the base replica after every sync are torch.equal."""
import random

import numpy as np
import pytest
import torch

from tests.graphsage_ist_step_check import BATCH, H, SEED, expected_events, schedule_args, toy

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
S = 2


def _run(host_path, L, use_pp, p_drop=0.2):
    from gist_amd import ist
    from gist_amd.arena import graphsage_dims
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    from tests.graphsage_ist_restatement import base_init_for
    ds = toy()
    fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
    base_init = base_init_for(graphsage_dims(fin, H, ncls, L), 9)
    random.seed(SEED)
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = (EngineClusterIter if host_path == 'step' else ClusterIter)(
        'toy', ds.g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp, par_li=[p.copy() for p in ds.par_li], device=DEV)
    group = ist.LocalCommGroup(S)
    ws = [ist.DistributedGraphSAGEWrapper(schedule_args(S, L, p_drop, r, use_pp), None, fin, ncls, DEV,
                                          base_init=base_init if r == 0 else None, comm=group.handle(r), seed=SEED)
          for r in range(S)]
    bases, homes = [], [[p.data_ptr() for p in w.sub_model.parameters()] for w in ws]
    apply = ws[-1].sync_apply

    def sync_apply():                        # (the last site's: every replica has been written)
        apply()
        bases.append([w.base.params.clone() for w in ws])
    ws[-1].sync_apply = sync_apply
    part = ws[0].sample_partitions()
    for w in ws:
        w.ini_sync_dispatch_model(part)
    gd = ds.g.to(DEV)
    lines = []
    res = ist.train_graphsage(ws, ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'], gd.ndata['test_mask'],
                              log=lambda *a, **k: None, host_path=host_path)
    ist.print_results(res, log=lines.append)
    torch.cuda.synchronize(DEV)
    # dispatch and sync wrote the sub arenas in place: no Parameter was re-homed
    assert homes == [[p.data_ptr() for p in w.sub_model.parameters()] for w in ws]
    return dict(ws=ws, res=res, bases=bases, lines=lines, it=it)


@pytest.mark.parametrize('L,use_pp', [(2, False), (1, True)])
def test_phases_is_step_bit_for_bit(L, use_pp):
    a = _run('step', L, use_pp)
    b = _run('phases', L, use_pp)
    for w in b['ws']:
        me = w.sub_model.__dict__['_graphsage_engines'][id(b['it'])]
        assert me.engine is w.engine and me.engine.arena is w.sub                        # the wrapper's own engine
        assert not me.engine.prefetch                                                    # several models on the iterator
    assert not any(w.sub_model.__dict__.get('_graphsage_engines') for w in a['ws'])
    assert a['res']['events'] == b['res']['events'] == expected_events()
    assert b['res']['events'].count('sync') == 3 and b['res']['events'].count('dispatch') == 1
    for si in range(S):
        la, lb = a['res']['losses'][si], b['res']['losses'][si]
        assert len(la) == len(lb) == 12
        for j, (x, y) in enumerate(zip(la, lb)):
            assert torch.equal(x, y), 'site %d step %d: %r != %r' % (si, j, float(x), float(y))
    assert len(a['bases']) == len(b['bases']) == 3
    for k, (xs, ys) in enumerate(zip(a['bases'], b['bases'])):
        for r, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), 'base replica of rank %d after sync %d' % (r, k)
    for wa, wb in zip(a['ws'], b['ws']):
        assert torch.equal(wa.sub.params, wb.sub.params)
        assert wa.engine.drop_calls == wb.engine.drop_calls > 0
    assert a['res']['val_accs'] == b['res']['val_accs'] and a['res']['test_accs'] == b['res']['test_accs']
    # the five result lines
    for run in (a, b):
        assert [l.split(':')[0] for l in run['lines']] == ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
        for l in run['lines']:
            float(l.split(':')[1])
