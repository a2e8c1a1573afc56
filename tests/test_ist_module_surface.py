"""CPU, multi-process: the reference-shaped surface of gist_amd.ist.DistributedGNNWrapper -- the five-argument
constructor (cluster_gcn_ist_distrib.py:71-91), `sub_model` and `base_model` -- under a real `gloo` process group
(world size 2 and 4), against the golden vectors recorded from the reference's own wrapper (tests/golden/G4_ist_*.npz).

As in test_ist_gloo.py, the HIP block kernels cannot run here, so the wrapper is given a TEST DOUBLE for the three block
movers (torch indexing, tests/gat_ist_restatement.py).  Everything else is the product code: the torch-RNG draws of the
constructor, the modules over the arenas, the partition sampling, the packed all-gather over torch.distributed.
"""
import argparse
import os
import random

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.gat_ist_restatement import TorchBlocks

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def _args(S, H, L, rank):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=rank, dropout=0.0, use_layernorm=True)


def _is_view_of(p, t):
    return (p.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
            and p.storage_offset() == t.storage_offset() and p.shape == t.shape)


def _worker(rank, S, name, port, q):
    from gist_amd import ist
    try:
        d = np.load(os.path.join(GOLD, name))
        H, L = int(d['H']), int(d['L'])
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        random.seed(int(d['seed']))
        torch.manual_seed(int(d['seed']))
        w = ist.DistributedGNNWrapper(_args(S, H, L, rank), None, int(d['fin']), int(d['ncls']),
                                      torch.device('cpu'), blocks=TorchBlocks())
        errs = []

        def same(a, b, what, tol=0.0):
            a = a.detach().numpy()
            if a.shape != b.shape:
                errs.append(what + ' shape')
            elif tol == 0.0:
                if not np.array_equal(a, b):
                    errs.append(what)
            elif np.abs(a - b).max() > tol:
                errs.append(what)

        sub = [l.linear for l in w.sub_model.layers]
        if rank == 0:
            base = [l.linear for l in w.base_model.layers]
            for k in range(L + 1):                      # the reference's torch-RNG draw, with no base_init
                same(base[k].weight, d['base0_W%d' % k], 'base_model W%d' % k)
                same(base[k].bias, d['base0_b%d' % k], 'base_model b%d' % k)
                if not (_is_view_of(base[k].weight, w.base.W[k]) and _is_view_of(base[k].bias, w.base.b[k])):
                    errs.append('base_model layer %d is not a view of the base arena' % k)
        elif w.base_model is not None:
            errs.append('base_model on rank %d' % rank)
        for k in range(L + 1):
            if not (_is_view_of(sub[k].weight, w.sub.W[k]) and _is_view_of(sub[k].bias, w.sub.b[k])):
                errs.append('sub_model layer %d is not a view of the sub arena' % k)
        order = [p for l in sub for p in (l.weight, l.bias)]
        if len(list(w.sub_model.parameters())) != len(order) or any(
                a is not b for a, b in zip(w.sub_model.parameters(), order)):
            errs.append('sub_model.parameters() not in arena order')
        w.ini_sync_dispatch_model()
        for k in range(L + 1):
            same(sub[k].weight, d['r%d_sub_ini_W%d' % (rank, k)], 'sub_ini W%d' % k)
            same(sub[k].bias, d['r%d_sub_ini_b%d' % (rank, k)], 'sub_ini b%d' % k)
        # "training": the reference's perturbed sub-model of this rank, written into the module's parameters in place
        with torch.no_grad():
            for k in range(L + 1):
                sub[k].weight.copy_(torch.from_numpy(d['r%d_sub_pert_W%d' % (rank, k)]))
                sub[k].bias.copy_(torch.from_numpy(d['r%d_sub_pert_b%d' % (rank, k)]))
        w.sync_model()
        if rank == 0:
            base = [l.linear for l in w.base_model.layers]
            for k in range(L + 1):
                same(base[k].weight, d['base1_W%d' % k], 'base1 W%d' % k)
                same(base[k].bias, d['base1_b%d' % k], 'base1 b%d' % k, tol=0.0 if k < L else 1e-6)
        w.dispatch_model()
        for k in range(L + 1):
            same(sub[k].weight, d['r%d_sub_disp_W%d' % (rank, k)], 'sub_disp W%d' % k)
            if k < L:
                same(sub[k].bias, d['r%d_sub_disp_b%d' % (rank, k)], 'sub_disp b%d' % k)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, errs))
    except Exception as e:          # surface the failure in the parent
        import traceback
        q.put((rank, ['EXC ' + repr(e) + traceback.format_exc()]))


@pytest.mark.parametrize('name,S,port', [('G4_ist_S2_H16_L2.npz', 2, 29851),
                                         ('G4_ist_S4_H16_L2.npz', 4, 29852),
                                         ('G4_ist_S2_H8_L1.npz', 2, 29853),
                                         ('G4_ist_S4_H16_L3.npz', 4, 29854)])
def test_reference_shaped_wrapper_gloo(name, S, port):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, S, name, port, q)) for r in range(S)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(S)]
    for p in procs:
        p.join(timeout=60)
    for rank, errs in sorted(res):
        assert errs == [], 'rank %d: %s' % (rank, errs)


def test_explicit_base_init_draws_nothing():
    """base_init given -- even None, as the other ranks of every existing caller pass it -- keeps the torch RNG as it
    was; leaving it out draws the reference's initial weights."""
    from gist_amd import ist
    d = np.load(os.path.join(GOLD, 'G4_ist_S2_H16_L2.npz'))
    H, L, fin, C = int(d['H']), int(d['L']), int(d['fin']), int(d['ncls'])
    init = [(d['base0_W%d' % k], d['base0_b%d' % k]) for k in range(L + 1)]
    torch.manual_seed(7)
    for rank, base_init in ((1, None), (0, None), (0, init)):
        state = torch.get_rng_state()
        w = ist.DistributedGNNWrapper(_args(2, H, L, rank), None, fin, C, torch.device('cpu'), base_init=base_init,
                                      blocks=TorchBlocks())
        assert torch.equal(state, torch.get_rng_state()), (rank, base_init is None)
        assert (w.base_model is None) == (rank != 0)
        if base_init is not None:
            for k in range(L + 1):
                assert np.array_equal(w.base_model.layers[k].linear.weight.detach().numpy(), init[k][0])
    state = torch.get_rng_state()
    ist.DistributedGNNWrapper(_args(2, H, L, 1), None, fin, C, torch.device('cpu'), blocks=TorchBlocks())
    assert not torch.equal(state, torch.get_rng_state())          # rank 1 draws its sub GCN


def test_sub_model_records_its_arena_for_the_module_engine():
    """The module engine finds the wrapper's arena behind sub_model (and builds its step on it); a model whose
    parameters moved off that arena, or any other model, gets none."""
    import torch.nn.functional as F
    from gist_amd import ist
    from gist_amd.module_engine import shared_arena
    from gist_amd.modules import GCN
    w = ist.DistributedGNNWrapper(_args(4, 32, 2, 0), None, 10, 5, torch.device('cpu'), base_init=None,
                                  blocks=TorchBlocks())
    dims = [(l.linear.in_features // 2, l.linear.out_features) for l in w.sub_model.layers]
    assert dims == w.sub_dims and shared_arena(w.sub_model, dims) is w.sub
    assert shared_arena(w.base_model, w.base_dims) is None          # the replica keeps no gradients: never stepped
    other = GCN(10, 32, 5, 2, F.relu, 0.0, True, False, True, 4, True)
    assert shared_arena(other, dims) is None
    w.sub_model.layers[1].linear.weight.data = w.sub.W[1].clone()  # (the reference's dispatch assigns .data)
    assert shared_arena(w.sub_model, dims) is None
