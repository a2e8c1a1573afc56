"""CPU: the gate that keeps tests/test_stream_order_gpu.py complete.

Every function of include/gist_hip.h with a gist_stream_t parameter must be a key of that file's COVERED table (export ->
the test that reaches it on a side stream) or of its EXEMPT table, which gives a reason -- admissible only for an export
with no device-visible result to compare.  A new launching export without a stream-order case fails here.  The second
test builds both input variants of every kernel-level case on the CPU and holds them to the rule the protocol rests on:
A and B have the same names, shapes, strides and dtypes, so both take the same kernel path."""
import torch

from tests.test_scratch_guard import HEADER, header_exports
from tests import test_stream_order_gpu as G


def stream_exports(exports=None):
    """the header's functions that take a gist_stream_t, sorted"""
    exports = header_exports() if exports is None else exports
    return sorted(name for name, params in exports.items() if any('gist_stream_t' in t for t, _ in params))


def test_every_stream_taking_export_has_a_case_or_a_reason():
    names = stream_exports()
    rows, bad = [], []
    for name in names:
        if name in G.COVERED:
            assert callable(getattr(G, G.COVERED[name], None)), (name, G.COVERED[name])
            cases = [c.name for c in G.CASES if name in c.exports] + [c[0] for c in G.STEP_CASES if name in c[3]]
            assert cases, name
            rows.append('  %-40s %-24s %s' % (name, G.COVERED[name], ', '.join(cases)))
        elif name in G.EXEMPT:
            rows.append('  %-40s EXEMPT: %s' % (name, G.EXEMPT[name]))
        else:
            rows.append('  %-40s NO STREAM-ORDER CASE' % name)
            bad.append(name)
    print('\n%d exports of the C ABI take a stream:\n%s' % (len(names), '\n'.join(rows)))
    assert not bad, 'stream-taking exports without a stream-order case or an exemption: %r' % bad
    assert len(names) == 81, 'the header now has %d stream-taking exports: say so in the GPU file\'s docstring too' % len(names)
    # the tables name nothing that does not exist, nothing twice, and every exemption has its reason
    assert set(G.COVERED) <= set(names), sorted(set(G.COVERED) - set(names))
    assert set(G.EXEMPT) <= set(names) and not set(G.EXEMPT) & set(G.COVERED)
    assert all(isinstance(r, str) and len(r) > 20 for r in G.EXEMPT.values())
    assert list(G.EXEMPT) == ['gist_empty_launches']
    # what the issue names must be reached, whatever the tables become
    for name in ('gist_gemm_nt_f32', 'gist_gemm_nn_f32', 'gist_gemm_tn_f32', 'gist_colsum_f32', 'gist_adam_segments_extract_f32',
                 'gist_standard_scaler_f32', 'gist_spmm_blocks_prepare', 'gist_publish_i64', 'gist_copy_i32', 'gist_sage_step',
                 'gist_gat_step_phase', 'gist_graphsage_step_phase', 'gist_baseline_gcn_step', 'gist_extract_parts_desc_batch'):
        assert name in G.COVERED, name
    assert len({c.name for c in G.CASES}) == len(G.CASES) and len({c[0] for c in G.STEP_CASES}) == len(G.STEP_CASES)


def test_gate_sees_a_new_export():
    text = open(HEADER).read().replace('#ifdef __cplusplus\n}', 'int gist_new_thing_f32(const float *x, float *y, gist_stream_t stream);\n'
                                       '#ifdef __cplusplus\n}')
    found = set(stream_exports(header_exports(text))) - set(stream_exports())
    assert found == {'gist_new_thing_f32'} and not found & (set(G.COVERED) | set(G.EXEMPT))


def test_both_variants_of_every_case_have_one_layout():
    rows = []
    for c in G.CASES:
        a, b = c.make('A'), c.make('B')
        assert list(a) == list(b), c.name
        differ = 0
        for k in a:
            if not torch.is_tensor(a[k]):
                assert type(a[k]) is type(b[k]), (c.name, k)      # a host argument of the call
                differ += a[k] != b[k]
                continue
            assert not a[k].is_cuda and a[k].shape == b[k].shape and a[k].stride() == b[k].stride() and a[k].dtype == b[k].dtype, \
                (c.name, k, a[k].shape, b[k].shape)
            differ += not torch.equal(a[k], b[k])
            if a[k].dtype.is_floating_point:
                assert torch.isfinite(a[k].float()).all() and torch.isfinite(b[k].float()).all(), (c.name, k)
        assert differ, c.name + ': the variants do not differ'
        assert set(c.pinned) <= set(a), c.name
        rows.append('  %-44s %2d buffers, %d differ' % (c.name, len(a), differ))
    print('\n' + '\n'.join(rows))
