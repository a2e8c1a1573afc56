"""GPU: gist_ln_affine_fwd_drop_f32 (lnaffine.hip, the DROP instantiations of ln_affine_fwd_kernel) through
hip.ln_affine_fwd_drop, against its bitwise contract:

  * yhat, rstd and out2 are the plain entry's yhat, rstd and out for pointers of the same alignment class;
  * out is gist_dropout_f32 applied to that out as a column window of a [n_rows, mask_ld] tensor (p = 0: out itself).

Every width regime carries the mask: a wave per row (d <= 1024), a workgroup per row in registers (<= 4096), the
three-read path above; with 16-byte and (d % 4 != 0, or a window at column offset 1) scalar accesses; quads at even
and odd mask indices.  Everything outside the window keeps its sentinel."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = [1, 3, 4, 20, 256, 260, 1024, 1028, 4096, 4100]
SENTINEL = -7.0


def _inputs(n, d):
    gen = torch.Generator().manual_seed(1000 * d + n)
    x = (torch.randn(n, d, generator=gen) * 2.0 + 0.5).to(DEV)
    lb, gamma, beta = (torch.randn(d, generator=gen).to(DEV) for _ in range(3))
    return x, lb, gamma, beta


def _window(n, d, layout):
    """(the [n, mask_ld] tensor, its window `out`, the window's first column)"""
    T = torch.full((n, 2 * d + (2 if layout == 'offset1' else 0)), SENTINEL, device=DEV)
    c0 = 1 if layout == 'offset1' else 0
    return T, T[:, c0:c0 + d], c0


@pytest.mark.parametrize('layout', ['left', 'offset1'])
@pytest.mark.parametrize('d', WIDTHS)
def test_drop_tail_is_the_plain_tail_then_dropout(d, layout):
    from gist_amd import hip
    seed = 11
    for n in ((1, 4, 5, 37) if d <= 260 else (5,)):
        x, lb, gamma, beta = _inputs(n, d)
        for relu in (0, 1):
            # the plain entry on the same layout of `out` (the same alignment class), once per (n, relu)
            T0, out0, c0 = _window(n, d, layout)
            yhat0, rstd0 = torch.empty(n, d, device=DEV), torch.empty(n, device=DEV)
            hip.ln_affine_fwd(x, lb, gamma, beta, yhat0, out0, rstd0, relu)
            mask_ld = T0.shape[1]
            for with_out2 in (True, False):
                for base in (6, 9):
                    for p in (0.0, 0.5):
                        what = 'n=%d d=%d %s relu=%d out2=%s base=%d p=%g' % (n, d, layout, relu, with_out2, base, p)
                        T, out, _ = _window(n, d, layout)
                        yhat, rstd = torch.full((n, d), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
                        out2 = torch.full((n, d), SENTINEL, device=DEV) if with_out2 else None
                        hip.ln_affine_fwd_drop(x, lb, gamma, beta, yhat, out, out2, rstd, relu, p, seed, base + c0, mask_ld)
                        assert torch.equal(yhat, yhat0) and torch.equal(rstd, rstd0), what
                        if with_out2:
                            assert torch.equal(out2, out0), what
                        want = T0.clone()
                        if p > 0.0:
                            hip.dropout_(want, p, seed, base)
                            if n * d >= 64:      # the mask is a mask: it drops and keeps
                                kept = (want[:, c0:c0 + d] != 0).float().mean().item()
                                live = (out0 != 0).float().mean().item()
                                assert 0.2 * live < kept < 0.8 * live + 1e-9, what
                        assert torch.equal(out, want[:, c0:c0 + d]), what
                        # nothing outside the window was written
                        outside = torch.ones_like(T, dtype=torch.bool)
                        outside[:, c0:c0 + d] = False
                        assert bool((T[outside] == SENTINEL).all()), what


def test_no_mask_and_no_copy_is_the_plain_launch():
    """p = 0 and out2 = None run the plain instantiations: the same bits as gist_ln_affine_fwd_f32, one launch"""
    from gist_amd import _lib, hip
    L = _lib.load()
    for d in (20, 1028, 4100):
        x, lb, gamma, beta = _inputs(5, d)
        a = [torch.empty(5, d, device=DEV), torch.empty(5, d, device=DEV), torch.empty(5, device=DEV)]
        b = [torch.empty(5, d, device=DEV), torch.empty(5, d, device=DEV), torch.empty(5, device=DEV)]
        hip.ln_affine_fwd(x, lb, gamma, beta, a[0], a[1], a[2], 1)
        before = L.gist_launch_count()
        hip.ln_affine_fwd_drop(x, lb, gamma, beta, b[0], b[1], None, b[2], 1, 0.0, 3, 5, 2 * d)
        assert L.gist_launch_count() - before == 1
        assert all(torch.equal(u, v) for u, v in zip(a, b))
