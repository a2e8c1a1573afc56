"""CPU: the guard-band helper itself (tests/scratch_guard.py), and the gate that keeps the scratch tests complete.

The gate reads include/gist_hip.h and the signature table of gist_amd/_lib.py, finds every export that takes
caller-owned scratch -- a pointer parameter named workspace*, slabs, partials, *_partials, scratch, *_workspace,
spmm_prepared or (the block structure gist_spmm_blocks_prepare fills) prepared -- and every scratch field of the three
step-plan structs (and of gist_extract_parts_desc), and wants each in the case table of tests/test_scratch_bounds_kernels_gpu.py or
tests/test_scratch_bounds_steps_gpu.py, or in the short exemption list below, with its reason (a const parameter can only be
read: it needs neither).  A new scratch consumer without a guard case fails here.

The last test is the capacity table's own check: for every GEMM case and capacity the kernel-level file runs, the plan
the launcher is handed (gist_gemm_plan_query, a host function) keeps its operands and its slabs inside the bytes the
test allocates -- the property a sizing bug in gemm_plan.cpp breaks, seen without a GPU."""
import fnmatch
import os
import re

import pytest
import torch

from tests.scratch_guard import LEFT_MIN, RIGHT_MIN, Guarded
from tests import test_scratch_bounds_kernels_gpu as KERNELS
from tests import test_scratch_bounds_steps_gpu as STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gist_hip.h')


# -- Guarded on the CPU -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nbytes', [1, 37, 4096, (1 << 20) + 3])
def test_guarded_layout(nbytes):
    g = Guarded(nbytes, 'cpu', align=256, name='buffer')
    assert g.ptr % 256 == 0 and g.nbytes == nbytes
    assert g.left_bytes >= LEFT_MIN and g.right_bytes >= max(nbytes, RIGHT_MIN)
    assert g.view().data_ptr() == g.ptr and g.view().numel() == nbytes
    assert g.ptr + nbytes == g._buf.data_ptr() + g._end           # the right band starts at the byte behind the interior
    assert g.check() is None
    band = g._buf[g._end:].clone()
    assert band.unique().numel() > 200 and not torch.equal(band[:-1], band[1:])      # a pattern, not a constant
    g.view().fill_(0x5A)                                           # writing all of the interior touches no band
    assert g.check() is None
    g.assert_intact()


def _flip(g, pos):
    g._buf[pos] = g._buf[pos] ^ 0xFF


def test_guarded_reports_side_and_offset():
    n = 1000
    g = Guarded(n, 'cpu', name='slab buffer')
    _flip(g, g._end)                                               # one byte past the end
    assert g.check() == [('right', 0, 0)]
    with pytest.raises(AssertionError, match=r'slab buffer: bytes 0 \.\. 0 PAST THE END of its 1000 bytes'):
        g.assert_intact()
    g = Guarded(n, 'cpu', name='slab buffer')
    _flip(g, g._start - 1)                                         # one byte before the start
    assert g.check() == [('left', -1, -1)]
    with pytest.raises(AssertionError, match=r'slab buffer: bytes 1 \.\. 1 BEFORE ITS START'):
        g.assert_intact()
    g = Guarded(n, 'cpu', name='slab buffer')
    far = g._buf.numel() - 1
    _flip(g, far)                                                  # the far end of the right band
    assert g.check() == [('right', g.right_bytes - 1, g.right_bytes - 1)] and g.right_bytes - 1 >= RIGHT_MIN - 1
    g = Guarded(n, 'cpu')
    _flip(g, g._end + 5)
    _flip(g, g._end + 70000)                                       # (beyond one period of the pattern)
    _flip(g, 3)
    assert g.check() == [('left', 3 - g._start, 3 - g._start), ('right', 5, 70000)]
    # a store of a band byte's own value goes unseen -- which is why the pattern is not a constant: the same value one
    # byte further is seen
    g = Guarded(n, 'cpu')
    v = int(g._buf[g._end + 9])
    g._buf[g._end + 9] = v
    assert g.check() is None
    g._buf[g._end + 10] = v
    assert (g.check() == [('right', 10, 10)]) == (int(Guarded(n, 'cpu')._buf[g._end + 10]) != v)


def test_guarded_poisons_read_back_as_intended():
    g = Guarded(4096, 'cpu')
    g.poison('nan')
    assert torch.isnan(g.view(torch.float32)).all() and torch.isnan(g.view(torch.bfloat16)).all()
    assert torch.isnan(g.view(torch.float16)).all() and (g.view(torch.int32) == -1).all()
    g.poison('zero')
    assert not g.view(torch.float32).any() and not g.view(torch.bfloat16).any() and not g.view(torch.int32).any()
    g.view(torch.int32).copy_(torch.arange(1024, dtype=torch.int32))
    g.poison('keep')
    assert torch.equal(g.view(torch.int32), torch.arange(1024, dtype=torch.int32))
    assert torch.equal(g.view(torch.float32).view(torch.int32), torch.arange(1024, dtype=torch.int32))
    with pytest.raises(ValueError):
        g.poison('ones')
    assert g.check() is None


# -- the coverage gate ----------------------------------------------------------------------------------------------------
SCRATCH_NAMES = ('workspace*', 'slabs', 'partials', '*_partials', 'scratch', '*_workspace', 'spmm_prepared', 'prepared')
# plan fields that are scratch under another name: the headers' "scratch" / "backward scratch shared by the layers"
PLAN_SCRATCH_EXTRA = {'StepPlan': ('dZ', 'extract_scratch'),
                      'GATStepPlan': ('dZ', 'g', 'ds_dst', 'dd', 'ds_src', 'd_out', 'extract_scratch'),
                      'GraphSAGEStepPlan': ('dZ', 'extract_scratch'), 'ExtractPartsDesc': ()}

# (export or plan struct, parameter or field) -> why no guard case
EXEMPT = {
    ('gist_class_dw_slabs_f32', 'slabs'):
        'tests/test_class_layer_gpu.py already checks the tail of its slab buffer (listed as covered there)',
    ('gist_ln_relu_bwd_colsum_class_dw_f32', 'slabs'):
        'the same slabs through the same launcher argument check (classlayer.hip); bit-equal to gist_class_dw_slabs_f32 in '
        'tests/test_class_layer_gpu.py',
    ('gist_ln_relu_bwd_colsum_f32', 'col_partials'):
        'an output, not scratch: [gist_row_chunks16(n)][d] chunk sums, every element defined by the call; held to float64 '
        'inside sentinels by tests/test_rowops_kernels_gpu.py',
    ('gist_ln_relu_bwd_colsum_class_dw_f32', 'col_partials'):
        'the same output of the same kernel body (tests/test_rowops_kernels_gpu.py CS_CASES with a rider)',
    ('gist_spmm_csr_drop_lnbwd_f32', 'col_partials'):
        'an output: [gist_spmm_lnb_units][d] rows the consumer sums, its row count checked by the entry point; compared in '
        'tests/test_fused_ops_gpu.py and tests/test_spmm_kernels_gpu.py',
    ('gist_b3_split_f32', 'col_partials'): 'an output: column sums per 64 rows, compared in tests/test_b3_split_gpu.py',
    ('gist_class_layer_f32', 'dlogits_col_partials'):
        'an output: [gist_row_chunks16(n)][n_classes] chunk sums, compared in tests/test_class_layer_gpu.py',
}


def header_exports(text=None):
    """{export: [(type text, parameter name)]} of every function the header declares"""
    text = open(HEADER).read() if text is None else text
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', ' ', text, flags=re.M)
    out = {}
    for m in re.finditer(r'\b(gist_\w+)\s*\(([^;{}()]*)\)\s*;', text):
        name, args = m.group(1), m.group(2).strip()
        params = []
        if args and args != 'void':
            for a in args.split(','):
                pm = re.match(r'^(.*?)(\w+)\s*$', a.strip(), flags=re.S)
                params.append((pm.group(1).strip(), pm.group(2)))
        out[name] = params
    return out


READ_ONLY = set()      # (filled by scratch_consumers) const parameters: the call can only read them -- the consumers of slabs,
                       # partial sums and block structures that another, guarded, call wrote


def is_scratch_name(name):
    return any(fnmatch.fnmatchcase(name, pat) for pat in SCRATCH_NAMES)


def scratch_consumers(exports=None, signatures=None):
    """[(export, parameter)] of the header + [(plan struct, field)] of the three step plans"""
    from gist_amd import _lib
    found = []
    signatures = _lib.SIGNATURES if signatures is None else signatures
    for name, params in sorted((header_exports() if exports is None else exports).items()):
        if name not in signatures:
            continue
        for type_text, p in params:
            if '*' in type_text and is_scratch_name(p):
                found.append((name, p))
                if 'const' in type_text:
                    READ_ONLY.add((name, p))
    for struct in ('StepPlan', 'GATStepPlan', 'GraphSAGEStepPlan', 'ExtractPartsDesc'):
        for field, ctype in getattr(_lib, struct)._fields_:
            pointer = ctype is _lib._p or (hasattr(ctype, '_type_') and getattr(ctype, '_type_', None) is _lib._p)
            if pointer and (is_scratch_name(field) or field in PLAN_SCRATCH_EXTRA[struct]):
                found.append((struct, field))
    return found


def test_header_and_signature_table_name_the_same_exports():
    from gist_amd import _lib
    exports = header_exports()
    missing = sorted(set(_lib.SIGNATURES) - set(exports))
    assert not missing, 'in gist_amd/_lib.py but not parsed from the header: %r' % missing
    for name, (res, args) in _lib.SIGNATURES.items():
        assert len(args) == len(exports[name]), (name, len(args), exports[name])


def test_every_scratch_consumer_has_a_guard_case_or_a_reason():
    consumers = scratch_consumers()
    covered = dict(KERNELS.COVERED)
    covered.update(STEPS.COVERED)
    rows, bad = [], []
    for key in consumers:
        if key in covered:
            rows.append('  %-42s %-22s covered by %s' % (key + (covered[key],)))
            module = KERNELS if key in KERNELS.COVERED else STEPS
            assert callable(getattr(module, covered[key], None)), (key, covered[key])
        elif key in EXEMPT:
            rows.append('  %-42s %-22s EXEMPT: %s' % (key + (EXEMPT[key],)))
        elif key in READ_ONLY:
            rows.append('  %-42s %-22s const: the call only reads what a guarded call wrote' % key)
        else:
            rows.append('  %-42s %-22s NO GUARD CASE' % key)
            bad.append(key)
    print('\ncaller-owned scratch of the C ABI:\n' + '\n'.join(rows))
    assert not bad, 'scratch consumers without a guard case or an exemption: %r' % bad
    # the tables name nothing that does not exist, nothing twice, and every exemption has its reason
    known = set(consumers)
    assert set(covered) <= known, sorted(set(covered) - known)
    assert set(EXEMPT) <= known, sorted(set(EXEMPT) - known)
    assert not set(EXEMPT) & set(covered)
    assert all(isinstance(r, str) and len(r) > 20 for r in EXEMPT.values())
    assert len(EXEMPT) <= 10
    # what the issue names must be found by the scan, whatever the patterns become
    for key in (('gist_gemm_nt_f32', 'workspace'), ('gist_gemm_slabs_f32', 'slabs'), ('gist_colsum_f32', 'partials'),
                ('gist_gemm_nn_dropout_colsum_f32', 'g_col_partials'), ('gist_extract_parts_batch', 'scratch'),
                ('gist_spmm_blocks_prepare', 'prepared'), ('gist_ln_affine_bwd_f32', 'workspace'),
                ('StepPlan', 'h3_workspace'), ('StepPlan', 'fused_workspace'), ('StepPlan', 'spmm_prepared'),
                ('StepPlan', 'col_partials'), ('GATStepPlan', 'attn_partials'), ('GraphSAGEStepPlan', 'ln_workspace')):
        assert key in known, key


def test_gate_sees_a_new_consumer():
    """the scan on a header with one more scratch-taking export: found, and neither covered nor exempt"""
    text = open(HEADER).read().replace('#ifdef __cplusplus\n}', 'int gist_new_thing_f32(const float *x, float *y, void *workspace, '
                                       'int64_t workspace_bytes, float *row_partials, gist_stream_t stream);\n#ifdef __cplusplus\n}')
    exports = header_exports(text)
    assert 'gist_new_thing_f32' in exports
    found = set(scratch_consumers(exports, dict.fromkeys(exports))) - set(scratch_consumers())
    assert found == {('gist_new_thing_f32', 'workspace'), ('gist_new_thing_f32', 'row_partials')}
    assert not found & (set(KERNELS.COVERED) | set(STEPS.COVERED) | set(EXEMPT))
    assert not is_scratch_name('params') and not is_scratch_name('slab_bytes') and not is_scratch_name('n_slabs')


# -- the capacity table hands no launcher a plan that leaves its bytes -------------------------------------------------------
def test_gemm_capacity_table_keeps_every_plan_inside_its_bytes():
    from gist_amd import _lib, hip
    L = _lib.load()
    prev = hip.gemm_mode()
    rows = 0
    try:
        for (mode, hooks, form, m, n, k, full, less) in KERNELS.PLAN_CASES:
            hip.gemm_mode(mode)
            for name, v in hooks.items():
                hip.tuning(name, v)
            try:
                table = KERNELS.gemm_capacities(L, form, m, n, k)
                assert table[0][0] == 'need' and table[0][2]['workspace_bytes'] == table[0][1]
                for kind, cap, plan in table:
                    rows += 1
                    assert KERNELS.plan_fits(plan, cap), (mode, form, m, n, k, kind, cap, plan)
                    assert plan['workspace_bytes'] <= cap or kind != 'need'
            finally:
                for name in hooks:
                    hip.tuning(name, 0)
    finally:
        hip.gemm_mode(prev)
    assert rows >= 40
