"""GPU: the grid-wide whole-tensor LayerNorm (lnall.hip: gist_ln_all_fwd_f32 / gist_ln_all_bwd_f32, torch.ops.gist.
layer_norm_all, autograd.layer_norm_all) against numpy float64 restatements of the definitions

    yhat = (x - mean) / s,  s = sqrt(var + eps)  (biased variance, eps = float32(1e-5) as the kernel receives it)
    dx   = rstd * (g - mean(g) - yhat * mean(g * yhat))

Sizes: n in {1, 3, 255, 256, 257, 4097} and OVER = 1024 * 4096 + 4099, just past the cap of 1024 workgroups, where
every workgroup walks a slice of 1025 or 1026 quads (5 trips of 256 threads instead of 4); OVER again with every tensor
starting one float past a 16-byte boundary (a scalar head of 3 and a tail), and with the input alone misaligned (the
all-scalar kernels, 17 trips).  Inputs: standard normal; mean 1e4 with unit spread; a constant; one outlier of 1e6 among
zeros, at the FIRST element (where a first-element pivot would be worst) and, for n > 1, also in the middle.  Every
output is a window of a buffer of sentinel NaNs that must come back bit for bit around it.

Bounds, per element, from the operation counts.  u = eps32 / 2 is one rounding.  D = 20 bounds the roundings on an
addend's way into a slice sum: the subtraction of the pivot (1), the two levels of a quad's (a + b) + (c + d), and one
sequential add per trip (5 on the vector path, 17 on the scalar one, which has no quad levels).  The block tree and the
merge of the partials are fp64 and contribute nothing at this scale.

  forward.  (a) the fp32 mean is the fp64 merge rounded once: u |mean|; the slice means m + C / cnt under it carry the
  error of C = sum (x - m): D u mean|x - m| <= D u sigma.  Through 1 / s: u |mean| / s + D u.  (b) rstd: every (x - m)^2
  carries 3 roundings and D more into Q, all terms positive, the correction C^2 / cnt is second order: var is
  relative-exact to (3 + D) u, rstd to (3 + D) u / 2 + u for its own rounding = 12.5 u.  (c) x - mean and the product:
  2 u |yhat|.  Sum: u (14.5 |yhat| + 20 + |mean| / s) = eps32 (7.25 |yhat| + 10 + 0.5 |mean| / s) <=
      eps32 * (C0 * (1 + |yhat64|) + C1 * |mean| / s),  C0 = 10, C1 = 0.5.
  The second term is the cancellation in x - mean: the fp32 mean itself is only known to u |mean|; no fp32 evaluation
  avoids it.  stats: |mean32 - mean| <= eps32 (0.5 |mean| + 10 sigma), |rstd32 - rstd| <= 6.25 eps32 rstd.

  backward, against fp64 on the SAME fp32 g, yhat and rstd.  With G = sum|g| / n and GY = sum|g yhat| / n: m1 carries
  D u G and its rounding, m2 (one product more) (D + 1) u GY and its rounding; g - m1, yhat * m2, the second subtraction
  and the product with rstd are at most 3 roundings of |g| + |m1| + |yhat m2|:
      |dx32 - dx64| <= rstd * eps32 * (C0B * (G + |yhat| GY) + 1.5 * (|g| + |m1| + |yhat m2|)),  C0B = (D + 2) / 2 = 11.

  autograd against fp64 autograd of F.layer_norm(h, h.shape): the fp64 backward uses ITS yhat and rstd, so the forward's
  own error (bound Bf per element, 6.25 eps32 on rstd) propagates: + rstd * (G max Bf |yhat| + |m2| Bf) + 6.25 eps32 |dx|.

Worst error / bound on an MI355X (`pytest -s` prints them; 'row' = the one-workgroup row kernel on the same inputs as a
[1, n] row, recorded, not asserted):

    case         grid fwd   grid stats   row fwd    grid bwd   row bwd
    normal       0.068      0.073        0.399      0.632      0.632
    mean 1e4     0.786      0.786        3.651      0.611      0.611
    constant     0.000      0.056        2344.6     0.391      0.391
    outlier      0.049      0.077        0.071      0.423      0.423
    autograd     0.096 (forward), 0.110 (backward)

(The backward columns agree because their worst cases are the smallest sizes, where both paths round alike.  The row
kernel's forward exceeds the bound on the shifted and the constant input: its fp32 mean of n addends is further from the
true mean than one rounding, which the grid kernels' pivoted partial sums and fp64 merge avoid.)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
LN_EPS = float(np.float32(1e-5))
C0, C1, C0B = 10.0, 0.5, 11.0
OVER = 1024 * 4096 + 4099
SIZES = [1, 3, 255, 256, 257, 4 * 1024 + 1, OVER]
LAYOUTS = [(n, 'aligned') for n in SIZES] + [(OVER, 'off1'), (OVER, 'mixed'), (257, 'off1'), (3, 'off1')]
KINDS = ['normal', 'shift', 'const', 'outlier0', 'outlier_mid']
SENT_BITS = 0x7FC0DEAD
WORST = {}


def _ratio(fam, err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    m = float(r.max()) if r.size else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), m)
    return m


def make_input(kind, n, seed=0):
    rs = np.random.RandomState(seed + n % 1000)
    if kind == 'normal':
        return rs.randn(n).astype(F32)
    if kind == 'shift':
        return (1e4 + rs.randn(n)).astype(F32)
    if kind == 'const':
        return np.full(n, 3.7, F32)
    x = np.zeros(n, F32)
    x[0 if kind == 'outlier0' else n // 2] = 1e6
    return x


def window(n, off):
    """A float32 device buffer of sentinels and its window [off, off + n) (off = 1: one float past a 16-byte boundary)."""
    buf = torch.full((n + 8,), float('nan'), dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENT_BITS)
    return buf, buf[off:off + n]


def sentinels_intact(buf, n, off):
    b = buf.view(torch.int32)
    return bool((b[:off] == SENT_BITS).all()) and bool((b[off + n:] == SENT_BITS).all())


def put(x, off):
    buf, w = window(x.size, off)
    w.copy_(torch.from_numpy(x))
    return w


def forward_ref(x):
    x64 = x.astype(np.float64)
    mean = x64.mean()
    var = ((x64 - mean) ** 2).mean()
    s = np.sqrt(var + LN_EPS)
    return (x64 - mean) / s, mean, s, np.sqrt(var)


def forward_bound(yhat64, mean, s):
    return EPS32 * (C0 * (1 + np.abs(yhat64)) + C1 * abs(mean) / s)


def backward_ref(g, yhat, rstd):
    g64, y64 = g.astype(np.float64), yhat.astype(np.float64)
    m1, m2 = g64.mean(), (g64 * y64).mean()
    dx = float(rstd) * (g64 - m1 - y64 * m2)
    G, GY = np.abs(g64).mean(), np.abs(g64 * y64).mean()
    bound = float(rstd) * EPS32 * (C0B * (G + np.abs(y64) * GY) + 1.5 * (np.abs(g64) + abs(m1) + np.abs(y64 * m2)))
    return dx, bound, (m1, m2, G, GY)


def offsets(layout):
    return dict(aligned=(0, 0), off1=(1, 1), mixed=(1, 0))[layout]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,layout', LAYOUTS)
def test_forward_and_backward_against_float64(n, layout, kind):
    from gist_amd import hip
    if kind == 'outlier_mid' and n == 1:
        kind = 'outlier0'
    fam = kind.split('_')[0].rstrip('0')
    x = make_input(kind, n)
    off_in, off_out = offsets(layout)
    xd = put(x, off_in)
    ybuf, yd = window(n, off_out)
    stats = torch.zeros(2, dtype=torch.float32, device=DEV)
    hip.ln_all_fwd(xd, yd, stats)
    yhat = yd.cpu().numpy()
    mean32, rstd32 = (float(v) for v in stats.cpu().numpy())
    assert sentinels_intact(ybuf, n, off_out)
    y64, mean, s, sigma = forward_ref(x)
    r_f = _ratio(fam + ' grid fwd', np.abs(yhat - y64), forward_bound(y64, mean, s))
    r_m = _ratio(fam + ' grid stats', abs(mean32 - mean), EPS32 * (0.5 * abs(mean) + 10 * sigma) + 1e-300)
    r_r = _ratio(fam + ' grid stats', abs(rstd32 - 1 / s), 6.25 * EPS32 / s)
    if kind == 'const':
        assert not yhat.any()                                        # exactly zero
        assert mean32 == float(x[0])
    # two calls, the same bits
    ybuf2, yd2 = window(n, off_out)
    stats2 = torch.zeros_like(stats)
    hip.ln_all_fwd(xd, yd2, stats2)
    assert torch.equal(yd.view(torch.int32), yd2.view(torch.int32)) and torch.equal(stats.view(torch.int32),
                                                                                    stats2.view(torch.int32))
    # backward on the kernel's own yhat and rstd, gradients of mixed magnitude
    rs = np.random.RandomState(n % 997 + 5)
    g = (rs.randn(n) * np.where(rs.rand(n) < 0.1, 50.0, 1.0)).astype(F32)
    gd = put(g, off_in)
    dbuf, dd = window(n, off_out)
    hip.ln_all_bwd(gd, yd if layout != 'mixed' else put(yhat, off_in), stats, dd)
    dx = dd.cpu().numpy()
    assert sentinels_intact(dbuf, n, off_out)
    dx64, b_bound, _ = backward_ref(g, yhat, rstd32)
    r_b = _ratio(fam + ' grid bwd', np.abs(dx - dx64), b_bound + 1e-300)
    dbuf2, dd2 = window(n, off_out)
    hip.ln_all_bwd(gd, yd if layout != 'mixed' else put(yhat, off_in), stats, dd2)
    assert torch.equal(dd.view(torch.int32), dd2.view(torch.int32))
    # the 'row' path on the same inputs: recorded, not asserted
    xr = torch.from_numpy(x).to(DEV).reshape(1, -1)
    out_r = torch.empty_like(xr)
    rstd_r = torch.empty(1, dtype=torch.float32, device=DEV)
    hip.ln_relu_fwd(xr.clone(), out_r, rstd_r, True, False)
    _ratio(fam + ' row fwd', np.abs(out_r.cpu().numpy().ravel() - y64), forward_bound(y64, mean, s))
    dy_r = torch.empty_like(xr)
    hip.ln_relu_bwd(torch.from_numpy(g).to(DEV).reshape(1, -1), torch.from_numpy(yhat).to(DEV).reshape(1, -1),
                    stats[1:2].clone(), dy_r, True, False)
    _ratio(fam + ' row bwd', np.abs(dy_r.cpu().numpy().ravel() - dx64), b_bound + 1e-300)
    print('ln_all n=%d %s %s: fwd %.3f mean %.3f rstd %.3f bwd %.3f' % (n, layout, kind, r_f, r_m, r_r, r_b))
    assert r_f < 1 and r_m < 1 and r_r < 1 and r_b < 1


def test_empty_tensor_is_a_no_op():
    from gist_amd import hip
    x = torch.empty(0, dtype=torch.float32, device=DEV)
    stats = torch.full((2,), 7.0, device=DEV)
    hip.ln_all_fwd(x, torch.empty_like(x), stats)
    hip.ln_all_bwd(x, x, stats, torch.empty_like(x))
    assert stats.tolist() == [7.0, 7.0]


def test_custom_op_passes_opcheck():
    from torch.library import opcheck
    from gist_amd import ops  # noqa: F401
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    gen = torch.Generator(device=DEV).manual_seed(0)
    a = torch.randn(33, 20, device=DEV, generator=gen, requires_grad=True)
    opcheck(torch.ops.gist.layer_norm_all, (a,), test_utils=utils)
    opcheck(torch.ops.gist.layer_norm_all, (a.detach()[:, 1:],), test_utils=utils)          # not contiguous
    yhat, stats = torch.ops.gist.layer_norm_all(a.detach())
    opcheck(torch.ops.gist.layer_norm_all_bwd, (torch.randn_like(yhat), yhat, stats), test_utils=utils)


@pytest.mark.parametrize('shape,off', [((257, 16), 0), ((2708, 16), 0), ((301, 7), 1)])
def test_autograd_matches_float64_layer_norm(shape, off):
    """autograd.layer_norm_all(h) and its gradient against float64 autograd of F.layer_norm(h, h.shape); off = 1: h is
    a view one float past a 16-byte boundary (the op's outputs are aligned: the all-scalar kernels)."""
    import torch.nn.functional as Fn
    from gist_amd import autograd
    rs = np.random.RandomState(shape[0])
    n = shape[0] * shape[1]
    h = (rs.randn(*shape) * 2 + 0.5).astype(F32)
    w = rs.randn(*shape).astype(F32)
    hd = put(h.ravel(), off).view(*shape).requires_grad_()
    out = autograd.layer_norm_all(hd)
    (out * torch.from_numpy(w).to(DEV)).sum().backward()
    h64 = torch.from_numpy(h.astype(np.float64)).requires_grad_()
    ref = Fn.layer_norm(h64, h64.shape, eps=LN_EPS)
    (ref * torch.from_numpy(w.astype(np.float64))).sum().backward()
    y64, mean, s, _ = forward_ref(h.ravel())
    assert np.abs(ref.detach().numpy().ravel() - y64).max() < 1e-12
    Bf = forward_bound(y64, mean, s)
    r_f = _ratio('autograd fwd', np.abs(out.detach().cpu().numpy().ravel() - y64), Bf)
    dx64, b_bound, (m1, m2, G, GY) = backward_ref(w.ravel(), y64, 1 / s)
    assert np.abs(h64.grad.numpy().ravel() - dx64).max() < 1e-10
    bound = b_bound + (1 / s) * (G * Bf.max() * np.abs(y64) + abs(m2) * Bf) + 6.25 * EPS32 * np.abs(dx64)
    r_b = _ratio('autograd bwd', np.abs(hd.grad.cpu().numpy().ravel() - dx64), bound)
    print('ln_all autograd %s off %d: fwd %.3f bwd %.3f' % (shape, off, r_f, r_b))
    assert r_f < 1 and r_b < 1 and n == out.numel()


def test_grid_and_row_norm_are_the_same_function():
    from gist_amd import autograd
    h = torch.randn(2708, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    a, b = autograd.layer_norm_all(h), autograd.whole_tensor_layer_norm(h)
    assert float((a - b).abs().max()) < 1e-5


def test_print_worst_ratios():
    for fam in sorted(WORST):
        print('ln_all worst err / bound  %-22s %.3f' % (fam, WORST[fam]))
