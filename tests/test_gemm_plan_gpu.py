"""GPU: the launchers do what the plan says.  One small gist_gemm_* call per path and per form of it (one slice, k slices +
reduce, tail units + tail sum, the 256 x 256 tile, each kind of pre-pass), then each sliced or tailed one once more with a
workspace one byte smaller than the plan asks for: the library's launch counter (gist_launch_count) around the call equals
the launch count of the plan made for that workspace (gist_gemm_plan_query), and the result still equals a float64 product
within the bounds of the path's own test file (tests/test_kernels_gpu.py for the fp32 kernel, test_gemm_h3_gpu.py,
test_gemm_b3_gpu.py, test_gemm_b3c_gpu.py).

Path, slices, tail units and launch count of every case are literals, checked against the plan first; they were read from
the decision functions of commit 5d254ba (see tests/test_gemm_plan.py), not from the code under test."""
import numpy as np
import pytest
import torch

from tests.test_gemm_b3_gpu import _operands, _ref64

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = {'h3_min_tiles': 1, 'h3_min_gflop': 0.001}

# (mode, hooks, form, m, n, k) -> with all the workspace the plan asks for, and with one byte less (None: it asks for none, or
# the case has neither slices nor tail units): (path, tile_n, k slices, slices of a tail unit, launches)
CASES = [
    ('f32', {}, 'nt', 500, 256, 200, ('f32', 64, 1, 1, 1), None),
    ('bf16x3', {}, 'nt', 300, 200, 0, ('f32', 64, 1, 1, 1), None),                                       # an empty reduction: the bias
    ('f16x3', SMALL, 'tn', 300, 200, 0, ('f32', 64, 1, 1, 1), None),                                     # ... zeros
    ('f32', {}, 'nt', 300, 41, 2046, ('f32', 64, 32, 1, 2), ('f32', 64, 16, 1, 2)),                      # slices + reduce; halved
    ('f16x3', SMALL, 'nt', 200, 200, 96, ('f16x3', 128, 1, 1, 3), None),                                 # two row splits + main
    ('f16x3', SMALL, 'tn', 200, 200, 96, ('f16x3', 128, 1, 1, 5), None),                                 # 2 x (column maxima + transposing split)
    ('bf16x3', SMALL, 'nt', 300, 200, 256, ('bf16x3', 128, 1, 1, 3), None),                              # two splits + main
    ('bf16x3', SMALL, 'nt', 300, 200, 1024, ('bf16x3', 128, 4, 1, 4), ('f32', 64, 8, 1, 2)),             # + reduce; no room to split: fp32
    ('bf16x3', SMALL, 'nt', 2100, 4096, 512, ('bf16x3', 128, 1, 2, 4), ('bf16x3_load', 128, 1, 4, 2)),   # + tail sum; convert on load
    ('bf16x3', SMALL, 'nt', 2048, 8192, 64, ('bf16x3', 256, 1, 1, 3), None),                             # the 256 x 256 tile
    ('bf16x3', {'b3c': 2}, 'nt', 200, 200, 96, ('bf16x3_load', 64, 1, 1, 1), None),
    ('bf16x3', {'b3c': 2}, 'nn', 200, 200, 96, ('bf16x3_load', 64, 1, 1, 1), None),
    ('bf16x3', {'b3c': 2}, 'tn', 200, 200, 96, ('bf16x3_load', 64, 1, 1, 1), None),
    ('bf16x3', {'b3c': 2}, 'nt', 2100, 1024, 256, ('bf16x3_load', 64, 1, 2, 2), ('bf16x3_load', 64, 1, 1, 1)),   # tail units; whole tiles
]


def _call(L, form, a, b, k, bias, out, ws, ws_bytes):
    from gist_amd import hip
    m, n = out.shape
    wp = ws.data_ptr() if ws_bytes > 0 else None
    bp = bias.data_ptr() if bias is not None else None
    st = hip._stream()
    if form == 'nt':
        return L.gist_gemm_nt_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), bp, out.data_ptr(), out.stride(0), m, n, k, wp, ws_bytes, st)
    fn = L.gist_gemm_nn_f32 if form == 'nn' else L.gist_gemm_tn_f32
    return fn(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), m, n, k, wp, ws_bytes, st)


@pytest.mark.parametrize('mode,hooks,form,m,n,k,full,less', CASES,
                         ids=['%s-%s-%dx%dx%d' % (c[0], c[2], c[3], c[4], c[5]) for c in CASES])
def test_launches_follow_the_plan_and_the_product_holds(mode, hooks, form, m, n, k, full, less):
    from gist_amd import _lib, hip
    L = _lib.load()
    prev = hip.gemm_mode()
    try:
        hip.gemm_mode(mode)
        for name, v in hooks.items():
            hip.tuning(name, v)
        gen = torch.Generator(device=DEV).manual_seed(m + 3 * n + 7 * k)
        a, b = _operands(form, m, n, k, gen, 'normal')
        a_buf, b_buf = a, b
        if k == 0:      # (an empty tensor has no address: the call gets real buffers of which it may read nothing)
            a_buf, b_buf = (torch.ones(4, m, device=DEV), torch.ones(4, n, device=DEV)) if form == 'tn' else \
                           (torch.ones(m, 4, device=DEV), torch.ones(n, 4, device=DEV))
        bias = torch.randn(n, device=DEV, generator=gen) * 1e-3 if form == 'nt' else None
        rows = torch.arange(0, m, max(1, m // 192), device=DEV)
        ref, den = _ref64(form, a, b, rows)
        if bias is not None:
            ref = ref + bias.double()
        need = hip.gemm_plan(form, m, n, k)['workspace_bytes']
        assert (need > 0) == (less is not None or full[0] in ('f16x3', 'bf16x3')), need
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        for ws_bytes, want in ((need, full), (need - 1, less)):
            if want is None:
                continue
            plan = hip.gemm_plan(form, m, n, k, scratch_bytes=ws_bytes)
            print('%s %s %dx%dx%d workspace %d: %r' % (mode, form, m, n, k, ws_bytes, plan))
            assert (plan['path'], plan['tile_n'], plan['splits'], plan['tail_splits'], plan['launches']) == want
            out = torch.full((m, n), float('nan'), device=DEV)
            before = L.gist_launch_count()
            assert _call(L, form, a_buf, b_buf, k, bias, out, ws, ws_bytes) == 0, L.gist_last_error()
            issued = L.gist_launch_count() - before
            torch.cuda.synchronize()
            print('    launches issued %d, planned %d' % (issued, plan['launches']))
            assert issued == plan['launches']
            y = out[rows].double()
            assert torch.isfinite(y).all()
            if plan['path'] == 'f32':       # tests/test_kernels_gpu.py: test_gemm_nt
                err = (y - ref).abs().max().item()
                print('    max error %.3g' % err)
                assert err <= (2e-6 * np.sqrt(k) + 1e-6) * max(1.0, ref.abs().max().item())
                continue
            # the split paths: against the fp32 kernel's own error on the same operands
            hip.gemm_mode('f32')
            out1 = torch.full((m, n), float('nan'), device=DEV)
            assert _call(L, form, a_buf, b_buf, k, bias, out1, ws, need) == 0
            hip.gemm_mode(mode)
            y1 = out1[rows].double()
            e3 = ((y - ref).abs() / den).max().item()
            e1 = ((y1 - ref).abs() / den).max().item()
            rel = ref if plan['path'] == 'f16x3' else den
            r3 = ((y - ref).pow(2).mean().sqrt() / rel.pow(2).mean().sqrt()).item()
            r1 = ((y1 - ref).pow(2).mean().sqrt() / rel.pow(2).mean().sqrt()).item()
            print('    max %.3g (fp32 kernel %.3g), rms %.3g (%.3g)' % (e3, e1, r3, r1))
            if plan['path'] == 'f16x3':     # tests/test_gemm_h3_gpu.py
                assert e3 <= max(2.0 * e1, 5e-7) and r3 <= max(1.5 * r1, 1e-6), (e3, e1, r3, r1)
            else:                           # tests/test_gemm_b3_gpu.py, tests/test_gemm_b3c_gpu.py
                assert e3 <= max(3.0 * e1, 6e-7) and r3 <= max(1.25 * r1, 5e-8), (e3, e1, r3, r1)
    finally:
        for name in hooks:
            hip.tuning(name, 0)
        hip.gemm_mode(prev)
