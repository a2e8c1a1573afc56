"""CPU: the refusals gist_gat_step, gist_gat_step_phase and gist_graphsage_step share (csrc/step_host.h) return the same
code from each of them, under the name of the entry point that was called.  No device is needed: every case returns
before any device work, as in test_gat_step_exports.py.  Each case starts from a plan that passes every check -- two
layers, n_max = 8, every pointer a dummy that is never followed -- and breaks one thing."""
import ctypes

import pytest

N_MAX, N = 8, 4
DUMMY = 4096                                                # a non-null, 16-byte aligned address nobody dereferences
EINVAL, ENOSPACE = -1, -3                                  # include/gist_hip.h
WIDTHS = [(256, 8, 3), (1024, 16, 5), (4096, 64, 7)]        # (features, hidden, classes) tried for the split-K case


def _fill(struct, skip=()):
    """every pointer field of a ctypes struct -> DUMMY"""
    for name, ctype in struct._fields_:
        if ctype is ctypes.c_void_p and name not in skip:
            setattr(struct, name, DUMMY)


def _plan(entry, widths=WIDTHS[0]):
    from gist_amd import _lib
    f, h, c = widths
    gat = entry.startswith('gist_gat')
    P = _lib.GATStepPlan() if gat else _lib.GraphSAGEStepPlan()
    # no part tables (the remap extraction), no timer; GraphSAGE: no loss mask, no row blocks
    _fill(P, skip=('node_part', 'part_slot', 'extract_scratch', 'next_ids', 'timer', 'loss_mask', 'row_blocks'))
    P.n_layers, P.n_max = 2, N_MAX
    for k, (i, o) in enumerate(((f, h), (h, c))):
        _fill(P.layer[k])
        P.layer[k].n_in, P.layer[k].n_out = i, o
        if gat:
            P.layer[k].heads = 1
    if gat:
        P.d_out[0] = P.d_out[1] = DUMMY
        P.attn_partial_floats = 1 << 40
    else:
        P.ln_workspace_floats = 1 << 40
    P.workspace_bytes = 1 << 40
    P.n_params, P.ld_feat, P.col_capacity = 64, 2 * f, 64
    P.batch_index = P.next_batch_index = -1
    return P


def _call(entry, plan, n, flags, ids=DUMMY, adam_step=1):
    from gist_amd import _lib
    L = _lib.load()
    p = ctypes.byref(plan) if plan is not None else None
    if entry == 'gist_graphsage_step':
        rc = L.gist_graphsage_step(p, ids, n, 0, 0.01, 0.9, 0.999, 1e-8, 0.0, adam_step, flags, None)
    else:
        rc = getattr(L, entry)(p, ids, n, 0.01, 0.9, 0.999, 1e-8, 0.0, adam_step, flags, None)
    return rc, L.gist_last_error()


def _flags(entry, phase):
    """TRAIN, for the phase entry point with the bit of the phase that reads what the case breaks"""
    from gist_amd import _lib
    return _lib.GIST_STEP_TRAIN | (getattr(_lib, 'GIST_STEP_PHASE_' + phase) if entry.endswith('_phase') else 0)


def _set(**fields):
    def change(P):
        for k, v in fields.items():
            setattr(P, k, v)
    return change


# name -> (the phase that checks it, n, extra flag names, ids, adam_step, what to break in the plan)
CASES = {
    'n = 0': ('FORWARD', 0, (), DUMMY, 1, None),
    'n > n_max': ('FORWARD', N_MAX + 1, (), DUMMY, 1, None),
    'n_layers = 0': ('FORWARD', N, (), DUMMY, 1, _set(n_layers=0)),
    'n_layers = max + 1': ('FORWARD', N, (), DUMMY, 1, 'too many layers'),
    'unknown flag bit': ('FORWARD', N, (1 << 20,), DUMMY, 1, None),
    'EXTRACT | PREEXTRACTED': ('FORWARD', N, ('GIST_STEP_EXTRACT', 'GIST_STEP_PREEXTRACTED'), DUMMY, 1, None),
    'EXTRACT with null ids': ('FORWARD', N, ('GIST_STEP_EXTRACT',), None, 1, None),
    'EXTRACT without remap and part tables': ('FORWARD', N, ('GIST_STEP_EXTRACT',), DUMMY, 1, _set(remap=None)),
    'EXTRACT_NEXT without part tables': ('OPTIMIZER', N, ('GIST_STEP_EXTRACT_NEXT',), DUMMY, 1,
                                         _set(next_ids=DUMMY, next_n=N, next_batch_index=0)),
    'TRAIN with a null arena': ('OPTIMIZER', N, (), DUMMY, 1, _set(params=None)),
    'adam_step = 0': ('OPTIMIZER', N, (), DUMMY, 0, None),
}
# ... and the words of the check each case is meant to reach (the same from all three entry points)
SAYS = {
    'n = 0': b'empty batch', 'n > n_max': b'exceeds n_max = 8', 'n_layers = 0': b'bad n_layers',
    'n_layers = max + 1': b'bad n_layers', 'unknown flag bit': b'unknown flag bits',
    'EXTRACT | PREEXTRACTED': b'exclude each other', 'EXTRACT with null ids': b'null ids',
    'EXTRACT without remap and part tables': b'needs the part tables or remap',
    'EXTRACT_NEXT without part tables': b'GIST_STEP_EXTRACT_NEXT needs the part tables',
    'TRAIN with a null arena': b'null arena', 'adam_step = 0': b'adam_step is 1-based',
}
ENTRIES = ['gist_gat_step', 'gist_gat_step_phase', 'gist_graphsage_step']


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', sorted(CASES))
def test_shared_refusal(entry, case):
    from gist_amd import _lib
    phase, n, extra, ids, adam_step, change = CASES[case]
    P = _plan(entry)
    if change == 'too many layers':
        P.n_layers = _lib.GIST_MAX_LAYERS + 1
    elif change is not None:
        change(P)
    flags = _flags(entry, phase)
    for f in extra:
        flags |= getattr(_lib, f) if isinstance(f, str) else f
    before = _lib.load().gist_launch_count()
    rc, err = _call(entry, P, n, flags, ids, adam_step)
    assert rc == EINVAL and err.startswith(entry.encode() + b': ') and SAYS[case] in err, (rc, err)
    assert _lib.load().gist_launch_count() == before


@pytest.mark.parametrize('entry', ENTRIES)
def test_null_plan(entry):
    rc, err = _call(entry, None, N, _flags(entry, 'FORWARD'))
    assert rc == EINVAL and err.startswith(entry.encode() + b': null plan'), (rc, err)


@pytest.mark.parametrize('entry', ENTRIES)
def test_extract_next_without_train(entry):
    from gist_amd import _lib
    # (the phase entry point asks for GIST_STEP_TRAIN first, in words of its own: EINVAL under its name all the same)
    flags = _lib.GIST_STEP_EXTRACT_NEXT | (_lib.GIST_STEP_PHASE_OPTIMIZER if entry.endswith('_phase') else 0)
    rc, err = _call(entry, _plan(entry), N, flags)
    assert rc == EINVAL and err.startswith(entry.encode() + b':'), (rc, err)
    assert (b'GIST_STEP_TRAIN' if entry.endswith('_phase') else b'GIST_STEP_EXTRACT_NEXT') in err


@pytest.mark.parametrize('entry', ENTRIES)
def test_workspace_one_byte_short_is_enospace(entry):
    """layer 0's forward projection at N rows asks the library for split-K scratch: a plan whose workspace is one byte
    short of that is refused with GIST_ENOSPACE"""
    from gist_amd import _lib
    L = _lib.load()
    gat = entry.startswith('gist_gat')
    found = None
    for (f, h, c) in WIDTHS:
        need = L.gist_gemm_workspace_bytes(N, h, f if gat else 2 * f)
        if need > 0:
            found = ((f, h, c), need)
            break
    if found is None:
        # the only case of this file that may skip: no small plan makes the library ask for split-K scratch
        pytest.skip('gist_gemm_workspace_bytes is 0 for every small shape tried')
    widths, need = found
    P = _plan(entry, widths)
    size = L.gist_gat_step_workspace_bytes if gat else L.gist_graphsage_step_workspace_bytes
    assert size(ctypes.byref(P)) >= need
    P.workspace_bytes = need - 1
    before = L.gist_launch_count()
    rc, err = _call(entry, P, N, _flags(entry, 'FORWARD'))
    assert rc == ENOSPACE and err.startswith(entry.encode() + b': workspace too small'), (rc, err)
    assert str(need).encode() in err
    assert L.gist_launch_count() == before
