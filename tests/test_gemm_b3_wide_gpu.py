"""GPU tests of the 256 x 256 output tile of the bf16x3 GEMM (gemm_b3_wide_kernel in
gist_amd/csrc/gemm_b3.hip).  Every accumulator sees the same k tiles and the same six terms in the same
order as in the 256 x 128 kernel, so on every shape the launcher sends to it the output must be the
256 x 128 kernel's (tuning hook b3_wide = 1) bit for bit -- with and without bias, from each source
layout of the operands, with rows past m in the last row tile (2046 rows; 1800 rows, where three of
the four wave rows of that tile have no rows at all) and ragged columns and k."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (m, n, k): dZ1 and dW1 of the H = 4096 step, the transposed dW1, ragged m / k, ragged n, mostly-empty last row tile
SHAPES = [(2046, 8192, 4096), (8192, 4096, 2046), (4096, 8192, 2046), (2040, 8192, 4104), (8192, 4000, 2046),
          (1800, 8192, 1024)]


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    prev = h.gemm_mode()
    h.gemm_mode('bf16x3')
    yield h
    h.gemm_mode(prev)
    h.tuning('b3_wide', 0)


def _operands(form, m, n, k, gen):
    sa = (m, k) if form in ('nt', 'nn') else (k, m)
    sb = (n, k) if form == 'nt' else (k, n)
    a = torch.randn(*sa, device=DEV, generator=gen)
    b = torch.randn(*sb, device=DEV, generator=gen)
    return a, b


def _run(hip, form, a, b, bias, m, n):
    out = torch.full((m, n), float('nan'), device=DEV)
    if form == 'nt':
        hip.gemm_nt(a, b, bias, out)
    elif form == 'nn':
        hip.gemm_nn(a, b, out)
    else:
        hip.gemm_tn(a, b, out)
    return out


def _both(hip, form, a, b, bias, m, n):
    hip.tuning('b3_wide', 0)
    wide = _run(hip, form, a, b, bias, m, n)
    hip.tuning('b3_wide', 1)
    try:
        narrow = _run(hip, form, a, b, bias, m, n)
    finally:
        hip.tuning('b3_wide', 0)
    return wide, narrow


@pytest.mark.parametrize('m,n,k', SHAPES)
@pytest.mark.parametrize('form,with_bias', [('nt', True), ('nt', False), ('nn', False), ('tn', False)])
def test_wide_tile_is_bitwise_the_narrow_tile(hip, form, with_bias, m, n, k):
    from gist_amd import _lib
    L = _lib.load()
    assert L.gist_gemm_workspace_bytes(m, n, k) >= (m + n) * k * 6, 'shape not on the bf16x3 path'
    gen = torch.Generator(device=DEV).manual_seed(m + 3 * n + 7 * k + (1 if with_bias else 0))
    a, b = _operands(form, m, n, k, gen)
    bias = torch.randn(n, device=DEV, generator=gen) if with_bias else None
    wide, narrow = _both(hip, form, a, b, bias, m, n)
    assert torch.isfinite(wide).all()
    assert torch.equal(wide.view(torch.int32), narrow.view(torch.int32))
    assert torch.equal(_run(hip, form, a, b, bias, m, n).view(torch.int32), wide.view(torch.int32))


@pytest.mark.parametrize('form,m,n,k', [('nt', 2046, 8192, 4096), ('tn', 8192, 4096, 2046), ('nn', 2040, 8192, 4104)])
def test_wide_tile_error_at_fp32_mfma_level(hip, form, m, n, k):
    """The bar test_gemm_b3_gpu.py applies: against float64, max error within 3x and rms within 1.25x
    of the fp32-MFMA kernel's on the same operands."""
    gen = torch.Generator(device=DEV).manual_seed(11 * m + n + k)
    a, b = _operands(form, m, n, k, gen)
    bias = torch.randn(n, device=DEV, generator=gen) * 1e-3 if form == 'nt' else None
    rows = torch.arange(0, m, max(1, m // 192), device=DEV)
    a64, b64 = a.double(), b.double()
    if form == 'nt':
        ref, den = a64[rows] @ b64.t(), a64[rows].abs() @ b64.abs().t()
    elif form == 'nn':
        ref, den = a64[rows] @ b64, a64[rows].abs() @ b64.abs()
    else:
        ref, den = a64[:, rows].t() @ b64, a64[:, rows].abs().t() @ b64.abs()
    if bias is not None:
        ref = ref + bias.double()
    y3 = _run(hip, form, a, b, bias, m, n)[rows].double()
    hip.gemm_mode('f32')
    try:
        y1 = _run(hip, form, a, b, bias, m, n)[rows].double()
    finally:
        hip.gemm_mode('bf16x3')
    den = den.clamp(min=1e-300)
    e3 = ((y3 - ref).abs() / den).max().item()
    e1 = ((y1 - ref).abs() / den).max().item()
    r3 = ((y3 - ref).pow(2).mean().sqrt() / den.pow(2).mean().sqrt()).item()
    r1 = ((y1 - ref).pow(2).mean().sqrt() / den.pow(2).mean().sqrt()).item()
    assert e3 <= max(3.0 * e1, 6e-7), (e3, e1)
    assert r3 <= max(1.25 * r1, 5e-8), (r3, r1)
