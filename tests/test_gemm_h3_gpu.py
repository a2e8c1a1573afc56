"""GPU tests of the f16x3 split projection path (gist_amd/csrc/gemm_h3.hip) through the C ABI:
its error against a float64 product must be the fp32-MFMA kernel's (mode 'f32') on the same
operands, on the shapes the training step runs, with operands of very different magnitudes
(activations, weights ~1e-2, gradients ~1e-6 with a wide row-to-row spread)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    prev = h.gemm_mode()
    h.tuning('h3_min_gflop', 1)      # also exercise shapes below the production threshold
    yield h
    h.gemm_mode(prev)
    h.tuning('h3_min_gflop', 0)


def _run(hip, form, a, w, bias, m, n):
    out = torch.full((m, n), float('nan'), device=DEV)
    if form == 'nt':
        hip.gemm_nt(a, w, bias, out)
    elif form == 'nn':
        hip.gemm_nn(a, w, out)
    else:
        hip.gemm_tn(a, w, out)
    return out


def _operands(form, m, n, k, gen, kind):
    def mk(r, c, which):
        x = torch.randn(r, c, device=DEV, generator=gen)
        if kind == 'train':
            if which == 'a':      # post-LayerNorm/ReLU/dropout activations
                x = torch.relu(x) * 1.25 * (torch.rand(r, c, device=DEV, generator=gen) > 0.2)
            else:                 # weights U(-b, b), b ~ 1/sqrt(fan_in)
                x = (torch.rand(r, c, device=DEV, generator=gen) - 0.5) * 0.022
        elif kind == 'grad' and which == 'a':   # tiny gradients, row scales spread over e^(+-4)
            x = x * 1e-6 * torch.exp(2 * torch.randn(r, 1, device=DEV, generator=gen))
        return x
    if form == 'nt':
        return mk(m, k, 'a'), mk(n, k, 'b')
    if form == 'nn':
        return mk(m, k, 'a'), mk(k, n, 'b')
    return mk(k, m, 'a'), mk(k, n, 'b')


def _ref64(form, a, w, rows):
    a64, w64 = a.double(), w.double()
    if form == 'nt':
        return a64[rows] @ w64.t(), a64[rows].abs() @ w64.abs().t()
    if form == 'nn':
        return a64[rows] @ w64, a64[rows].abs() @ w64.abs()
    return a64[:, rows].t() @ w64, a64[:, rows].abs().t() @ w64.abs()


SHAPES = [('nt', 2046, 4096, 1204), ('nt', 2046, 4096, 8192), ('nn', 2046, 8192, 4096),
          ('tn', 4096, 8192, 2046), ('tn', 4096, 1204, 2046), ('nt', 1030, 1100, 1000),
          ('nn', 1500, 1024, 777), ('tn', 1024, 1204, 2046)]


@pytest.fixture(params=['auto', 'a_tile_64', 'a_tile_128'])
def tile(request, hip):
    """Both A-tile heights of the main kernel on every shape (tuning hook h3_tm; 'auto' = the
    launcher's own choice)."""
    hip.tuning('h3_tm', 0 if request.param == 'auto' else int(request.param.split('_')[-1]))
    yield request.param
    hip.tuning('h3_tm', 0)


@pytest.mark.parametrize('form,m,n,k', SHAPES)
@pytest.mark.parametrize('kind', ['normal', 'train', 'grad'])
def test_split_error_matches_fp32_mfma(hip, tile, form, m, n, k, kind):
    from gist_amd import _lib
    L = _lib.load()
    hip.gemm_mode('f16x3')
    assert L.gist_gemm_workspace_bytes(m, n, k) >= (m + n) * k * 4, 'shape not on the split path'
    gen = torch.Generator(device=DEV).manual_seed(m + 3 * n + 7 * k)
    a, w = _operands(form, m, n, k, gen, kind)
    bias = torch.randn(n, device=DEV, generator=gen) * 1e-3 if form == 'nt' and kind == 'normal' else None
    rows = torch.arange(0, m, max(1, m // 192), device=DEV)      # a sample of output rows
    ref, den = _ref64(form, a, w, rows)
    if bias is not None:
        ref = ref + bias.double()
    y3 = _run(hip, form, a, w, bias, m, n)[rows].double()
    hip.gemm_mode('f32')
    y1 = _run(hip, form, a, w, bias, m, n)[rows].double()
    hip.gemm_mode('f16x3')
    e3 = ((y3 - ref).abs() / den).max().item()
    e1 = ((y1 - ref).abs() / den).max().item()
    r3 = ((y3 - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    r1 = ((y1 - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    # error relative to sum_k |a||b| (the fp32 rounding model).  Measured (profiles/
    # r01_gemm_h3_error_vs_float64.txt): the split path's rms error is BELOW the fp32 chain's on long k (the
    # f16 MFMA sums 16 products per rounding), its max error about equal; where mode 'f32' picks
    # split-K its chains are shorter and its max error smaller, hence the absolute floor.
    assert e3 <= max(2.0 * e1, 5e-7), (e3, e1)
    assert r3 <= max(1.5 * r1, 1e-6), (r3, r1)
    assert torch.isfinite(y3).all()


def test_split_is_exact_on_f16_representable_operands(hip, tile):
    """Small integers are exact f16 values (lo = 0) and every partial sum is an integer below
    2^24: both modes must return the exact product, bit for bit."""
    hip.gemm_mode('f16x3')
    gen = torch.Generator(device=DEV).manual_seed(3)
    m, n, k = 1030, 1100, 1000
    a = torch.randint(-8, 9, (m, k), device=DEV, generator=gen).float()
    w = torch.randint(-8, 9, (n, k), device=DEV, generator=gen).float()
    y = _run(hip, 'nt', a, w, None, m, n)
    ref = (a.double() @ w.double().t()).float()
    assert torch.equal(y, ref)
    # asymmetric operand against the identity: catches a swapped fragment / C-D map
    b = (torch.arange(1024 * 1152, device=DEV).reshape(1024, 1152) % 2039).float()
    eye = torch.eye(1024, device=DEV)
    assert torch.equal(_run(hip, 'nn', eye, b, None, 1024, 1152), b)
    assert torch.equal(_run(hip, 'tn', eye, b, None, 1024, 1152), b)


def test_split_zero_operand_and_output_window(hip, tile):
    """An all-zero operand (absmax 0) gives zeros; nothing outside the [m, n] window is written
    when m, n are not tile multiples and the output is a window of a wider buffer."""
    hip.gemm_mode('f16x3')
    gen = torch.Generator(device=DEV).manual_seed(5)
    m, n, k = 1030, 1100, 520
    a = torch.randn(m, k, device=DEV, generator=gen)
    w = torch.zeros(n, k, device=DEV)
    assert (_run(hip, 'nt', a, w, None, m, n) == 0).all()
    w = torch.randn(n, k, device=DEV, generator=gen)
    ybuf = torch.full((m + 3, n + 8), 7.0, device=DEV)
    hip.gemm_nt(a, w, None, ybuf[:m, 4:4 + n])
    ref = (a.double() @ w.double().t()).float()
    assert (ybuf[:m, 4:4 + n] - ref).abs().max().item() < 1e-4 * ref.abs().max().item()
    assert (ybuf[m:] == 7.0).all() and (ybuf[:, :4] == 7.0).all() and (ybuf[:, 4 + n:] == 7.0).all()


def test_split_non_finite_inputs_stay_in_their_row(hip):
    """A NaN or an Inf in one row of an operand makes that output row (A) / column (B)
    non-finite and leaves every other output exactly as without it: the scales are per row."""
    hip.gemm_mode('f16x3')
    gen = torch.Generator(device=DEV).manual_seed(11)
    m, n, k = 1030, 1100, 520
    a = torch.randn(m, k, device=DEV, generator=gen)
    w = torch.randn(n, k, device=DEV, generator=gen)
    clean = _run(hip, 'nt', a, w, None, m, n)
    a2 = a.clone()
    a2[7, 100] = float('nan')
    a2[500, 3] = float('inf')
    w2 = w.clone()
    w2[33, 17] = float('nan')
    y = _run(hip, 'nt', a2, w2, None, m, n)
    bad_rows = torch.zeros(m, dtype=torch.bool, device=DEV)
    bad_rows[[7, 500]] = True
    bad_cols = torch.zeros(n, dtype=torch.bool, device=DEV)
    bad_cols[33] = True
    touched = bad_rows[:, None] | bad_cols[None, :]
    assert not torch.isfinite(y[7]).any() and not torch.isfinite(y[:, 33]).any()
    assert not torch.isfinite(y[500]).any()                  # Inf row: Inf or NaN everywhere, as in fp32
    assert torch.equal(y[~touched], clean[~touched])


def test_mode_switch_and_small_shapes_stay_fp32(hip):
    from gist_amd import _lib
    L = _lib.load()
    hip.gemm_mode('f32')
    assert L.gist_gemm_workspace_bytes(2046, 4096, 8192) == 0
    hip.gemm_mode('f16x3')
    assert L.gist_gemm_workspace_bytes(2046, 4096, 8192) > 0
    assert L.gist_gemm_workspace_bytes(2046, 41, 8192) == L.gist_gemm_workspace_bytes(2046, 41, 8192)
    hip.gemm_mode('f32')
    small = L.gist_gemm_workspace_bytes(2046, 41, 8192)
    hip.gemm_mode('f16x3')
    assert L.gist_gemm_workspace_bytes(2046, 41, 8192) == small      # skinny: fp32 split-K either way
    with pytest.raises(ValueError):
        hip.gemm_mode('bf16')


@pytest.mark.parametrize('form,m,n,k', [('nt', 2046, 4096, 1204), ('nn', 1500, 1024, 777),
                                        ('tn', 1024, 1204, 2046)])
@pytest.mark.parametrize('kind', ['cancel', 'range17', 'range', 'clamp'])
def test_split_adversarial_operands_documented_limits(hip, form, m, n, k, kind):
    """What the 22-bit f16x3 split does on operands built against it (it is opt-in, and not the
    arithmetic behind the headline, because of exactly these):
      cancel   large terms that cancel: the error stays relative to sum |a||b| like fp32's;
      range17  in-row dynamic range 2^17: elements at the bottom of a row have a subnormal `lo`;
      range    in-row dynamic range 2^40: elements 2^-22 below their row maximum lose ALL bits
               (one scale per row) -- error relative to sum |a||b| is still bounded (they are
               small against the row), but it is 2^-22-level, not 2^-24-level;
      clamp    row maxima beyond the +-60 scale-exponent clamp (2^73 / 2^-75 magnitudes): the
               2^-75 operand cannot be scaled into f16's normal range any more and the split degrades
               to ~13 significant bits (1e-4 relative, measured) -- finite, but not fp32-level.
    Bounds are the measured behaviour with headroom; the bf16x3 mode holds fp32's level on all of
    these (tests/test_gemm_b3_gpu.py)."""
    from tests.test_gemm_b3_gpu import _operands as adv_operands
    hip.gemm_mode('f16x3')
    gen = torch.Generator(device=DEV).manual_seed(m + 3 * n + 7 * k + 1)
    if kind == 'range17':
        a, w = adv_operands(form, m, n, k, gen, 'normal')
        a = a * torch.exp2(torch.randint(-17, 1, a.shape, device=DEV, generator=gen).float())
        w = w * torch.exp2(torch.randint(-17, 1, w.shape, device=DEV, generator=gen).float())
    elif kind == 'clamp':
        a, w = adv_operands(form, m, n, k, gen, 'normal')
        a, w = a * 2.0 ** 73, w * 2.0 ** -75
    else:
        a, w = adv_operands(form, m, n, k, gen, kind)
    rows = torch.arange(0, m, max(1, m // 192), device=DEV)
    ref, den = _ref64(form, a, w, rows)
    y3 = _run(hip, form, a, w, None, m, n)[rows].double()
    hip.gemm_mode('f32')
    y1 = _run(hip, form, a, w, None, m, n)[rows].double()
    hip.gemm_mode('f16x3')
    assert torch.isfinite(y3).all()
    den = den.clamp(min=1e-300)
    e3 = ((y3 - ref).abs() / den).max().item()
    e1 = ((y1 - ref).abs() / den).max().item()
    bound = {'cancel': 1e-6, 'range17': 2e-6, 'range': 2e-6, 'clamp': 1e-3}[kind]
    assert e3 <= bound, (kind, e3, e1)
    assert e1 <= 2e-6, (kind, e1)
