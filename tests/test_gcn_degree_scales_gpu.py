"""GPU: gist_gcn_degree_scales_f32 -- GraphConv's two degree scales in one launch -- bit for bit against numpy's
np.float32(1) / np.sqrt(deg.astype(np.float32)) with deg clamped to at least 1, on synthetic non-decreasing rowptr arrays
(the kernel never reads a column array) whose degrees include 0, 1, 2, 3, 5, 7, 2^24 - 1, 2^24 + 1 and 2^30 with a sum
below 2^31; the outputs between guard bands, under a NaN and under a zero poison; n_rows = 0 touches nothing."""
import numpy as np
import pytest
import torch

from tests.scratch_guard import Guarded, assert_all_intact

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SIZES = [1, 255, 256, 257, 1025]
# 2^30 + (2^24 - 1) + (2^24 + 1) + the small ones stays below 2^31
SPECIAL = [0, 1, 2, 3, 5, 7, (1 << 24) - 1, (1 << 24) + 1, 1 << 30]


def _degrees(n, seed):
    """n degrees: the special ones first as far as they fit (rotated by `seed`, so a one-row case still meets a large
    one), then small random ones with many zeros"""
    rs = np.random.RandomState(seed)
    special = SPECIAL[seed % len(SPECIAL):] + SPECIAL[:seed % len(SPECIAL)]
    deg = np.concatenate([np.array(special[:n], np.int64), rs.randint(0, 9, max(n - len(special), 0)).astype(np.int64)])
    deg = deg[rs.permutation(n)] if n > 1 else deg
    assert int(deg.sum()) < (1 << 31)
    return deg


def _rowptr(deg):
    rp = np.zeros(len(deg) + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    return torch.from_numpy(rp.astype(np.int32)).to(DEV)


def _want(deg):
    return np.float32(1) / np.sqrt(np.maximum(deg, 1).astype(np.float32))


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


@pytest.mark.parametrize('n', SIZES)
def test_bitwise_numpy_between_guard_bands_under_both_poisons(n):
    from gist_amd import hip
    deg_in, deg_out = _degrees(n, 8 if n == 1 else 0), _degrees(n, 6 if n == 1 else 3)
    if n >= len(SPECIAL):
        assert set(SPECIAL) <= set(deg_in.tolist()) and set(SPECIAL) <= set(deg_out.tolist())
    rp, trp = _rowptr(deg_in), _rowptr(deg_out)
    want_d, want_s = _want(deg_in), _want(deg_out)
    assert want_d.dtype == np.float32 and bool((want_d[deg_in == 0] == 1.0).all())
    got = []
    for poison in ('nan', 'zero'):
        gd, gs = Guarded(4 * n, DEV, name='nd'), Guarded(4 * n, DEV, name='ns')
        gd.poison(poison)
        gs.poison(poison)
        nd, ns = hip.gcn_degree_scales(rp, trp, gd.view(torch.float32), gs.view(torch.float32))
        torch.cuda.synchronize()
        assert_all_intact((gd, gs))
        assert np.array_equal(_bits(nd), want_d.view(np.int32)), (poison, 'nd')
        assert np.array_equal(_bits(ns), want_s.view(np.int32)), (poison, 'ns')
        got.append((nd.clone(), ns.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    # degree 0 gives exactly 1.0; the inputs are untouched
    assert bool((got[0][0].cpu()[torch.from_numpy(deg_in == 0)] == 1.0).all())
    assert torch.equal(rp, _rowptr(deg_in)) and torch.equal(trp, _rowptr(deg_out))


def test_every_special_degree_alone():
    """each special degree as a one-row graph: n_rows = 1 with every value, not only the two of the case above"""
    from gist_amd import hip
    for d in SPECIAL:
        deg = np.array([d], np.int64)
        nd, ns = hip.gcn_degree_scales(_rowptr(deg), _rowptr(deg[::-1].copy()))
        assert np.array_equal(_bits(nd), _want(deg).view(np.int32)), d
        assert np.array_equal(_bits(ns), _want(deg).view(np.int32)), d


def test_outputs_allocated_by_the_wrapper():
    """nd = None, ns = None: the wrapper allocates both; one rowptr for both sides gives one vector twice"""
    from gist_amd import hip
    deg = _degrees(257, 1)
    rp = _rowptr(deg)
    nd, ns = hip.gcn_degree_scales(rp, rp)
    assert nd.shape == ns.shape == (257,) and nd.dtype == torch.float32 and torch.equal(nd, ns)
    assert np.array_equal(_bits(nd), _want(deg).view(np.int32))


def test_no_rows_touch_nothing():
    from gist_amd import _lib, hip
    L = _lib.load()
    gd, gs = Guarded(64, DEV, name='nd'), Guarded(64, DEV, name='ns')
    gd.poison('nan')
    gs.poison('nan')
    rp = torch.zeros(1, dtype=torch.int32, device=DEV)
    before = L.gist_launch_count()
    rc = L.gist_gcn_degree_scales_f32(rp.data_ptr(), rp.data_ptr(), 0, gd.ptr, gs.ptr, hip._stream())
    assert rc == 0 and L.gist_launch_count() == before
    nd, ns = hip.gcn_degree_scales(rp, rp)
    assert nd.numel() == 0 and ns.numel() == 0 and L.gist_launch_count() == before
    torch.cuda.synchronize()
    assert_all_intact((gd, gs))
    assert bool((gd.view() == 0xFF).all()) and bool((gs.view() == 0xFF).all())
