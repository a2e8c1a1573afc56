"""GPU: the SEQUENCE the op-by-op twin issues (gist_amd/op_by_op.py behind SageEngine.forward, loss_and_backward and
adam_step), pinned -- what test_step_launch_sequence_gpu.py does for gist_sage_step.  The twin is compared with the native
step bit for bit elsewhere; a launch of it that moved or doubled is noticed there only if the bits change.  For a handful
of models that between them take every branch of the twin this records the library's own launch counter
(gist_launch_count) around each call of the first two batches and compares it with literals.

The literals were printed by the Python package of commit 3b5d9bc (the last one with the twin inside SageEngine), put in
front of this one on PYTHONPATH with the same libgist_hip.so loaded through GIST_LIB_PATH, not by the code under test.
They are integers and deterministic: the margin is zero.  A change that is MEANT to alter the sequence updates them and
says so."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# name -> (n_layers, LayerNorm, p_drop, n_feats, hidden, GIST_STEP_FUSE, how)
#   how: 'step' = train_step (one count per batch); 'masked' = forward, loss_and_backward with a mask and adam_step called
#   separately (the non-deferred path; three counts per batch); 'eval' = forward(b, training=False) (the narrowing class
#   layer's projection-first branch)
CASES = {
    'three_layers': (3, True, 0.2, 50, 96, '1', 'step'),
    'one_layer':    (1, False, 0.2, 50, 96, '1', 'step'),
    'no_dropout':   (2, True, 0.0, 50, 96, '1', 'step'),
    'narrow':       (2, True, 0.2, 302, 512, '1', 'step'),
    'unfused':      (2, True, 0.2, 302, 512, '0', 'step'),
    'masked':       (2, True, 0.2, 302, 512, '1', 'masked'),
    'eval':         (2, True, 0.2, 302, 512, '1', 'eval'),
}


def measure(name, monkeypatch):
    """The launches of every recorded call of the first two batches of an epoch, in call order."""
    from gist_amd import _lib, datasets, hip
    from gist_amd.engine import SageEngine, dims_for
    from gist_amd.sampler import EngineClusterIter
    n_layers, ln, p_drop, n_feats, hidden, fuse, how = CASES[name]
    monkeypatch.setenv('GIST_STEP_FUSE', fuse)
    L = _lib.load()
    prev = hip.gemm_mode()
    out = []
    try:
        hip.gemm_mode('f32')
        random.seed(4)
        ds = datasets.toy(seed=9, n=3000, n_blocks=30, n_feats=n_feats, n_classes=6, train_frac=1.0)
        g = ds.g
        it = EngineClusterIter('toy', g, len(ds.par_li), 5, np.arange(g.number_of_nodes(), dtype=np.int64),
                               par_li=[p.copy() for p in ds.par_li], device=DEV)
        dims = dims_for(n_feats, hidden, 6, n_layers)
        eng = SageEngine(dims, ln, p_drop, it.n_max, DEV, seed=11)
        gen = torch.Generator().manual_seed(1)
        for k, (i, o) in enumerate(dims):
            s_ = 1.0 / np.sqrt(2 * i)
            eng.arena.W[k].copy_((torch.rand(o, 2 * i, generator=gen) - 0.5) * 2 * s_)
            eng.arena.b[k].copy_((torch.rand(o, generator=gen) - 0.5) * 2 * s_)
        it.bind(eng, native=False)
        assert eng.plan is None      # (train_step runs the twin)

        def record(call):
            c0 = int(L.gist_launch_count())
            call()
            out.append(int(L.gist_launch_count()) - c0)

        for j, b in enumerate(it):
            assert b.n == 500
            if how == 'step':
                record(lambda: eng.train_step(b, 0.01, 5e-4))
            elif how == 'masked':
                mask = (torch.arange(b.n, device=DEV) % 3 != 0).to(torch.uint8)
                record(lambda: eng.forward(b, training=True))
                record(lambda: eng.loss_and_backward(b, mask, int(mask.sum().item())))
                record(lambda: eng.adam_step(0.01, 5e-4))
            else:
                record(lambda: eng.forward(b, training=False))
            if j == 1:
                break
        eng.check_extract()
        if how != 'eval':
            assert torch.isfinite(eng.loss).all()
        assert torch.isfinite(eng.logits(500)).all()
    finally:
        hip.gemm_mode(prev)
    return out


EXPECTED = {'eval': [12, 12],
            'masked': [11, 14, 1, 11, 14, 1],
            'narrow': [16, 16],
            'no_dropout': [15, 15],
            'one_layer': [10, 10],
            'three_layers': [26, 26],
            'unfused': [30, 30]}


@pytest.mark.parametrize('name', sorted(CASES))
def test_twin_issues_the_recorded_sequence(name, monkeypatch):
    assert name in EXPECTED, 'no literals for this model: print measure() under the package of the commit named above'
    assert measure(name, monkeypatch) == EXPECTED[name]
