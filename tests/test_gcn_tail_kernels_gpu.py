"""GPU: the BaselineGCN layer tail (gcntail.hip: gist_gcn_tail_fwd_f32 / _infer_f32 / _bwd_f32 through hip.gcn_tail_*)
against numpy float64 restatements on the same float32 inputs

    a = relu ? max(x + b, 0) : x + b;  yhat = norm ? (a - mean) / s : a,  s = sqrt(var + eps);  out = yhat * factor
    g = d_out * factor;  da = norm ? rstd * (g - mean(g) - yhat * mean(g * yhat)) : g;  dx = gate ? da : 0;  dbias = sum_r dx

with ONE mean and biased variance over the whole tensor, factor = gist_dropout_f32's (read off a tensor of ones), gate =
(x + b > 0) in float64 -- an fp32 add cannot round a non-zero sum to zero, so the fp32 gate is the same gate.  The method
is tests/test_ln_all_kernels_gpu.py's: every output is a window of a buffer of sentinels that must come back bit for bit
around it; the scratch of every call lies between tests/scratch_guard.py's guard bands and is poisoned first (NaN, and
zeros for the second backward call, whose bits must not differ).

Shapes (n_rows, d): (1, 1); (3, 7) an odd d below one unit; (16, 47) the class layer's width; (17, 64) one row past a
16-row chunk; (257, 16) several units; (1025, 4100) n * d just past 1024 * 4096, every workgroup walks a longer slice;
(1025, 4099) every unit straddles a row.  The two large shapes also one float past a 16-byte boundary ('off1': a scalar
head and tail; rows of the backward's row walk unaligned).  relu x norm in all four combinations; p = 0, and p = 0.5
with an even and an odd offset (the large shapes: the odd one).

Bounds, per element, from operation counts, u = eps32 / 2 one rounding.
  forward.  The kernel's a32 = fl(x + b) is the float64 a up to u |a|; on a32 the statistics and the normalisation are
  lnall.hip's, so test_ln_all_kernels_gpu.py's bound holds (C0 = 10, C1 = 0.5, derived there):
      eps32 * (C0 * (1 + |yhat|) + C1 * |mean| / s).
  The extra rounding moves a_i by u |a_i|, the mean by at most u A (A = mean|a|), the variance by at most 2 u M
  (M = mean(|a - mean| |a|)), s by u M / s; through yhat = (a - mean) / s:  + u ((|a_i| + A) / s + |yhat| M / s^2).
  stats: lnall's (eps32 (0.5 |mean| + 10 sigma); 6.25 eps32 / s) + u A resp. + u M / s^3.  Without norm yhat = a32: u |a|.
  out = yhat32 * factor, factor in {0, 2}: exact.
  backward, against float64 on the SAME fp32 d_out, yhat and rstd: g = d_out * factor is exact (factor 0 or 2), and da
  is lnall's backward on g, so its bound holds (C0B = 11):
      rstd * eps32 * (C0B * (G + |yhat| GY) + 1.5 * (|g| + |m1| + |yhat m2|));   without norm dx = g exactly.
  dbias: a column's dx pass through a tree of depth DB = ceil(chunks / 4) + 11 roundings -- a wave's 4 rows in order (3),
  the four waves (3), four interleaved running sums over the chunks (chunks / 4, and up to 3 left-over chunks), their
  pairwise sum (2) -- so |dbias32 - dbias64| <= sum_r bound(dx) + DB u sum_r |dx|.

Exact conditions, on 16-byte aligned dense buffers: yhat and stats are bitwise gist_ln_all_fwd_f32 of a stored relu(x + b);
out is bitwise gist_dropout_f32 of yhat; dx is bitwise gist_ln_all_bwd_f32 of a stored d_out * factor under the gate;
inference equals the training yhat, also in place; two backward calls leave the same bits.

Worst error / bound on an MI355X (`pytest -s` prints every case and, last, these):

    fwd 1.000   stats 0.260   bwd 0.563   dbias 0.213   autograd fwd 0.994, bwd 0.100

(fwd: the cases without norm, where yhat = fl(x + b) and the bound u |a| is the rounding itself -- the relative error
of one rounding is at most u / (1 + u), below u; with norm the worst case is 0.445.)
"""
import numpy as np
import pytest
import torch

from tests.scratch_guard import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
U = EPS32 / 2
LN_EPS = float(np.float32(1e-5))
C0, C1, C0B = 10.0, 0.5, 11.0
SENT_BITS = 0x7FC0DEAD
SMALL = [(1, 1), (3, 7), (16, 47), (17, 64), (257, 16)]
LARGE = [(1025, 4100), (1025, 4099)]
LAYOUTS = [(s, 0) for s in SMALL + LARGE] + [(s, 1) for s in LARGE]
FLAGS = [(1, 1), (1, 0), (0, 1), (0, 0)]
DROPS = {'p0': (0.0, 0, 0), 'even': (0.5, 11, 1000), 'odd': (0.5, 11, 1001)}
KINDS = ['normal', 'bias1e4', 'negative', 'zero', 'tiny', 'outlier0', 'outlier_mid']
WORST = {}


def _ratio(fam, err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    m = float(r.max()) if r.size else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), m)
    return m


def make_input(kind, n, d, seed=0):
    """x [n, d] and b [d] in float32"""
    rs = np.random.RandomState(seed + (n * d) % 1000)
    x = rs.randn(n, d).astype(F32)
    b = (0.3 * rs.randn(d)).astype(F32)
    if kind == 'bias1e4':                      # cancellation in a - mean
        b = (1e4 + rs.randn(d)).astype(F32)
    elif kind == 'negative':                   # x + b < 0 everywhere: with relu a is the constant 0
        x = -(np.abs(x) + 1).astype(F32)
        b = -np.abs(b)
    elif kind == 'zero':                       # x + b == 0 exactly: (-b) + b = +0, and -0 + -0 = -0 in every third column
        b[::3] = -0.0
        x = np.tile(-b, (n, 1))
        x[:, ::3] = -0.0
        assert not (x.astype(np.float64) + b).any() and np.signbit(x[:, ::3] + b[::3]).all()
    elif kind == 'tiny':                       # a few x + b = 1e-30 among values of mean about 1
        x = (1 + 0.1 * rs.randn(n, d)).astype(F32)
        b = np.zeros(d, F32)
        x.ravel()[::5] = 1e-30
    elif kind in ('outlier0', 'outlier_mid'):
        x = np.zeros((n, d), F32)
        b = np.zeros(d, F32)
        x.ravel()[0 if kind == 'outlier0' else (n * d) // 2] = 1e6
    return np.ascontiguousarray(x, F32), np.ascontiguousarray(b, F32)


def window(n, off):
    buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENT_BITS)
    return buf, buf[off:off + n]


def intact(buf, n, off):
    b = buf.view(torch.int32)
    return bool((b[:off] == SENT_BITS).all()) and bool((b[off + n:] == SENT_BITS).all())


def put(x, off):
    buf, w = window(x.size, off)
    w.copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    return w


def bits(t):
    return t.contiguous().view(torch.int32)


def scratch(floats, name, poison='nan'):
    g = Guarded(4 * int(floats), DEV, align=256, name=name)
    g.poison(poison)
    return g


def factors(n, d, drop):
    """gist_dropout_f32's factor of every element, float32 [n, d] on the device (ones at p = 0)"""
    from gist_amd import hip
    p, seed, offset = drop
    f = torch.ones(n, d, dtype=torch.float32, device=DEV)
    if p > 0:
        hip.dropout_(f, p, seed, offset)
    return f


def forward_ref(x, b, relu, norm):
    a = x.astype(np.float64) + b.astype(np.float64)
    gate = a > 0
    if relu:
        a = np.where(gate, a, 0.0)
    if not norm:
        return a, U * np.abs(a), gate, None
    mean = a.mean()
    var = ((a - mean) ** 2).mean()
    s = np.sqrt(var + LN_EPS)
    y = (a - mean) / s
    A, M = np.abs(a).mean(), (np.abs(a - mean) * np.abs(a)).mean()
    bound = EPS32 * (C0 * (1 + np.abs(y)) + C1 * abs(mean) / s) + U * ((np.abs(a) + A) / s + np.abs(y) * M / s ** 2)
    b_mean = EPS32 * (0.5 * abs(mean) + 10 * np.sqrt(var)) + U * A + 1e-300
    b_rstd = 6.25 * EPS32 / s + U * M / s ** 3
    return y, bound, gate, (mean, 1 / s, b_mean, b_rstd)


def backward_ref(g, yhat, rstd, gate, relu, norm, chunks):
    g64 = g.astype(np.float64)
    if norm:
        y64 = yhat.astype(np.float64)
        m1, m2 = g64.mean(), (g64 * y64).mean()
        da = float(rstd) * (g64 - m1 - y64 * m2)
        G, GY = np.abs(g64).mean(), np.abs(g64 * y64).mean()
        bound = float(rstd) * EPS32 * (C0B * (G + np.abs(y64) * GY) + 1.5 * (np.abs(g64) + abs(m1) + np.abs(y64 * m2)))
    else:
        da, bound = g64, np.zeros_like(g64)
    if relu:
        da, bound = np.where(gate, da, 0.0), np.where(gate, bound, 0.0)
    db_bound = bound.sum(0) + (-(-chunks // 4) + 11) * U * np.abs(da).sum(0)
    return da, bound, da.sum(0), db_bound


def run_case(n, d, off, relu, norm, drop, kind, tag):
    from gist_amd import _lib, hip
    L = _lib.load()
    p, seed, offset = drop
    nd = n * d
    x, b = make_input(kind, n, d)
    xd = put(x, off).view(n, d)
    bd = torch.from_numpy(b).to(DEV)
    ybuf, yd = window(nd, off)
    obuf, od = window(nd, off)
    stats = torch.full((2,), 7.0, dtype=torch.float32, device=DEV)
    ws_f = scratch(L.gist_ln_all_partials(nd), 'forward scratch')
    hip.gcn_tail_fwd(xd, bd, yd.view(n, d), od.view(n, d), stats, relu, norm, p, seed, offset, ws=ws_f.view(torch.float32))
    ws_f.assert_intact()
    assert intact(ybuf, nd, off) and intact(obuf, nd, off)
    assert torch.equal(bits(xd), bits(torch.from_numpy(x).to(DEV)))              # x is not overwritten
    yhat = yd.cpu().numpy().reshape(n, d)
    y64, f_bound, gate, st = forward_ref(x, b, relu, norm)
    r_f = _ratio('fwd', np.abs(yhat - y64), f_bound + 1e-300)
    r_s = 0.0
    if norm:
        mean32, rstd32 = (float(v) for v in stats.cpu().numpy())
        r_s = max(_ratio('stats', abs(mean32 - st[0]), st[2]), _ratio('stats', abs(rstd32 - st[1]), st[3]))
    else:
        assert stats.tolist() == [7.0, 7.0]
    fac = factors(n, d, drop)
    assert torch.equal(bits(od.view(n, d)), bits(yd.view(n, d) * fac))           # factor 0, 1 or 2: exact
    if p > 0:
        kept = float((fac > 0).float().mean())
        assert nd < 64 or abs(kept - 0.5) < 4 * 0.5 / np.sqrt(nd), kept
    # inference: the training yhat, into a buffer of its own and in place
    ibuf, idd = window(nd, off)
    hip.gcn_tail_infer(xd, bd, idd.view(n, d), relu, norm, ws=scratch(L.gist_ln_all_partials(nd), 'infer scratch').view(
        torch.float32))
    assert intact(ibuf, nd, off) and torch.equal(bits(idd), bits(yd))
    xbuf, xin = window(nd, off)
    xin.copy_(xd.view(-1))
    hip.gcn_tail_infer(xin.view(n, d), bd, xin.view(n, d), relu, norm)
    assert intact(xbuf, nd, off) and torch.equal(bits(xin), bits(yd))
    # backward, gradients of mixed magnitude
    rs = np.random.RandomState(nd % 997 + 5)
    go = (rs.randn(n, d) * np.where(rs.rand(n, d) < 0.1, 50.0, 1.0)).astype(F32)
    gd = put(go, off).view(n, d)
    need = int(L.gist_gcn_tail_bwd_workspace_floats(n, d))
    outs = []
    for poison in ('nan', 'zero'):
        dbuf, dd = window(nd, off)
        bbuf, db = window(d, off)
        ws_b = scratch(need, 'backward scratch', poison)
        hip.gcn_tail_bwd(gd, xd, bd, yd.view(n, d) if norm else None, stats if norm else None, dd.view(n, d), db, relu,
                         norm, p, seed, offset, ws=ws_b.view(torch.float32))
        ws_b.assert_intact()
        assert intact(dbuf, nd, off) and intact(bbuf, d, off)
        outs.append((dd, db))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    dx, dbias = outs[0][0].cpu().numpy().reshape(n, d), outs[0][1].cpu().numpy()
    g = (gd * fac).cpu().numpy()
    rstd32 = float(stats[1]) if norm else 1.0
    chunks = int(L.gist_row_chunks16(n))
    da64, b_bound, db64, db_bound = backward_ref(g, yhat, rstd32, gate, relu, norm, chunks)
    r_b = _ratio('bwd', np.abs(dx - da64), b_bound + 1e-300)
    r_d = _ratio('dbias', np.abs(dbias - db64), db_bound + 1e-300)
    if relu:
        assert not dx[~gate].any()                                               # closed: exactly zero
    exact = dict(fwd=True, bwd=True)
    if off == 0:
        # 16-byte aligned dense buffers: the bits of lnall.hip on stored intermediates
        a_pre = xd + bd
        if relu:
            a_pre = torch.where(a_pre > 0, a_pre, torch.zeros_like(a_pre))
        if norm:
            y2, s2 = torch.empty_like(a_pre), torch.empty(2, dtype=torch.float32, device=DEV)
            hip.ln_all_fwd(a_pre, y2, s2)
            exact['fwd'] = torch.equal(bits(y2), bits(yd.view(n, d))) and torch.equal(bits(s2), bits(stats))
            da = torch.empty_like(a_pre)
            hip.ln_all_bwd((gd * fac).contiguous(), yd.view(n, d), stats, da)
        else:
            exact['fwd'] = torch.equal(bits(a_pre), bits(yd.view(n, d)))
            da = gd * fac
        if relu:
            da = torch.where(torch.from_numpy(gate).to(DEV), da, torch.zeros_like(da))
        exact['bwd'] = torch.equal(bits(da), bits(outs[0][0].view(n, d)))
        if p > 0:
            dr = yd.view(n, d).clone()
            hip.dropout_(dr, p, seed, offset)
            exact['fwd'] = exact['fwd'] and torch.equal(bits(dr), bits(od.view(n, d)))
    print('gcn_tail %s (%d, %d) off %d relu %d norm %d %s: fwd %.3f stats %.3f bwd %.3f dbias %.3f exact %s'
          % (tag, n, d, off, relu, norm, kind, r_f, r_s, r_b, r_d, exact))
    assert r_f < 1 and r_s < 1 and r_b < 1 and r_d < 1
    assert exact['fwd'] and exact['bwd']
    return dict(yhat=yhat, stats=stats.cpu().numpy(), dx=dx, dbias=dbias, gate=gate)


CASES = [(s, off, relu, norm, drop) for s, off in LAYOUTS for relu, norm in FLAGS for drop in sorted(DROPS)
         if not (s in LARGE and drop == 'even')]


@pytest.mark.parametrize('shape,off,relu,norm,drop', CASES)
def test_every_shape_and_flag_against_float64(shape, off, relu, norm, drop):
    run_case(shape[0], shape[1], off, relu, norm, DROPS[drop], 'normal', drop)


@pytest.mark.parametrize('kind', KINDS[1:])
@pytest.mark.parametrize('shape,off', [((3, 7), 0), ((17, 64), 0), ((257, 16), 0), ((1025, 4099), 0), ((1025, 4099), 1)])
def test_numeric_edges_against_float64(shape, off, kind):
    n, d = shape
    r = run_case(n, d, off, 1, 1, DROPS['odd' if n > 16 else 'p0'], kind, 'edge')
    if kind == 'negative':
        # a is the constant 0: mean 0, rstd = 1 / sqrt(eps), everything else exactly zero
        assert not r['yhat'].any() and not r['dx'].any() and not r['dbias'].any() and not r['gate'].any()
        assert r['stats'][0] == 0 and r['stats'][1] == F32(1.0 / np.sqrt(np.float64(np.float32(LN_EPS))))
    if kind == 'zero':
        assert not r['gate'].any() and not r['dx'].any() and not r['dbias'].any()
    if kind == 'tiny':
        x, _ = make_input(kind, n, d)
        tiny = x == F32(1e-30)
        assert tiny.any() and r['gate'].all()
        assert np.all(r['yhat'][tiny] == r['yhat'][tiny].ravel()[0])            # a - mean rounds to -mean
        if n > 16:
            assert np.count_nonzero(r['dx'][tiny]) > 0.3 * tiny.sum()           # open (half of them dropped at p = 0.5)
        else:
            assert r['dx'][tiny].all()
    if kind != 'negative' and kind != 'zero':
        run_case(n, d, off, 1, 0, DROPS['p0'], kind, 'edge')


def test_empty_tensors_are_no_ops():
    from gist_amd import hip
    for n, d in ((0, 8), (5, 0)):
        x = torch.empty(n, d, dtype=torch.float32, device=DEV)
        b = torch.empty(d, dtype=torch.float32, device=DEV)
        stats = torch.full((2,), 7.0, device=DEV)
        db = torch.full((max(d, 1),), 7.0, device=DEV)
        hip.gcn_tail_fwd(x, b, torch.empty_like(x), torch.empty_like(x), stats, True, True, 0.5, 1, 0)
        hip.gcn_tail_infer(x, b, x, True, True, stats=stats)
        hip.gcn_tail_bwd(x, x, b, x, stats, torch.empty_like(x), db[:d], True, True, 0.5, 1, 0)
        assert stats.tolist() == [7.0, 7.0] and bool((db == 7.0).all())


def test_custom_ops_pass_opcheck():
    from torch.library import opcheck
    from gist_amd import ops  # noqa: F401
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    gen = torch.Generator(device=DEV).manual_seed(0)
    a = torch.randn(33, 20, device=DEV, generator=gen, requires_grad=True)
    b = torch.randn(20, device=DEV, generator=gen, requires_grad=True)
    for relu, norm, p in ((True, True, 0.0), (True, True, 0.5), (False, False, 0.0), (True, False, 0.5)):
        opcheck(torch.ops.gist.gcn_tail_fwd, (a, b, relu, norm, p, 3, 10), test_utils=utils)
        out, yhat, stats = torch.ops.gist.gcn_tail_fwd(a.detach(), b.detach(), relu, norm, p, 3, 10)
        assert yhat.numel() == (a.numel() if norm and p > 0 else 0)
        opcheck(torch.ops.gist.gcn_tail_bwd, (torch.randn_like(out), a.detach(), b.detach(),
                                              yhat if norm and p > 0 else out, stats, relu, norm, p, 3, 10), test_utils=utils)
    opcheck(torch.ops.gist.gcn_tail_fwd, (a.detach()[:, 1:], b.detach()[1:], True, True, 0.0, 0, 0), test_utils=utils)


@pytest.mark.parametrize('relu,norm,p', [(1, 1, 0.0), (1, 1, 0.5), (0, 1, 0.0), (1, 0, 0.5)])
def test_autograd_matches_float64_autograd(relu, norm, p):
    """autograd.gcn_tail and its gradients against float64 autograd of the composed definition under the same mask.  The
    float64 backward uses ITS yhat and rstd, so the forward's error (Bf per element, Br on rstd) propagates as in
    test_ln_all_kernels_gpu.py: + rstd * (G max Bf |yhat| + |m2| Bf) + (Br / rstd) |dx|."""
    import torch.nn.functional as Fn
    from gist_amd import _lib, autograd
    n, d = 301, 24
    x, b = make_input('normal', n, d, seed=3)
    w = np.random.RandomState(9).randn(n, d).astype(F32)
    xd, bd = torch.from_numpy(x).to(DEV).requires_grad_(), torch.from_numpy(b).to(DEV).requires_grad_()
    start = autograd._drop_counter[0]
    out = autograd.gcn_tail(xd, bd, relu, norm, p=p, seed=5)
    (out * torch.from_numpy(w).to(DEV)).sum().backward()
    assert autograd._drop_counter[0] == start + (n * d if p > 0 else 0)
    fac = factors(n, d, (p, 5, start)).cpu().numpy().astype(np.float64)
    x64, b64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(), torch.from_numpy(b.astype(np.float64)).requires_grad_()
    a64 = x64 + b64
    if relu:
        a64 = torch.relu(a64)
    y64t = Fn.layer_norm(a64, a64.shape, eps=LN_EPS) if norm else a64
    ref = y64t * torch.from_numpy(fac)
    (ref * torch.from_numpy(w.astype(np.float64))).sum().backward()
    y64, Bf, gate, st = forward_ref(x, b, relu, norm)
    r_f = _ratio('autograd fwd', np.abs(out.detach().cpu().numpy() - y64 * fac), Bf * fac + 1e-300)
    g = (w.astype(np.float64) * fac).astype(F32)
    chunks = int(_lib.load().gist_row_chunks16(n))
    da64, b_bound, db64, db_bound = backward_ref(g, y64, st[1] if norm else 1.0, gate, relu, norm, chunks)
    assert np.abs(x64.grad.numpy() - da64).max() < 1e-9 and np.abs(b64.grad.numpy() - db64).max() < 1e-9
    if norm:
        G, m2 = np.abs(g).mean(), abs((g.astype(np.float64) * y64).mean())
        extra = st[1] * (G * Bf.max() * np.abs(y64) + m2 * Bf) + (st[3] / st[1]) * np.abs(da64)
        b_bound = b_bound + np.where(gate, extra, 0.0) if relu else b_bound + extra
        db_bound = b_bound.sum(0) + (-(-chunks // 4) + 11) * U * np.abs(da64).sum(0)
    r_b = _ratio('autograd bwd', np.abs(xd.grad.cpu().numpy() - da64), b_bound + 1e-300)
    r_d = _ratio('autograd bwd', np.abs(bd.grad.cpu().numpy() - db64), db_bound + 1e-300)
    print('gcn_tail autograd relu %d norm %d p %.1f: fwd %.3f bwd %.3f dbias %.3f' % (relu, norm, p, r_f, r_b, r_d))
    assert r_f < 1 and r_b < 1 and r_d < 1


def test_print_worst_ratios():
    for fam in sorted(WORST):
        print('gcn_tail worst err / bound  %-14s %.3f' % (fam, WORST[fam]))
