"""GPU tests of the bf16x3 pre-pass (b3_split_kernel in gist_amd/csrc/gemm_b3.hip, through the diagnostic
entry point gist_b3_split_f32): both split layouts, their zero padding, the dropout stream and the per-64-row
column sums must equal, byte for byte, a construction of the same in torch / numpy on the CPU (float32 ->
bfloat16 is round-to-nearest-even there too) -- on the six splits of the H = 4096 step, ragged shapes,
ld > cols, a source that is not 16-byte aligned, and one-layout calls."""
import numpy as np
import pytest
import torch

from tests import dropout_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    return h


def _kpad(k):
    return -(-k // 64) * 64


def _dropped(x, p, seed, offset):
    """x under gist_dropout_f32's mask (element index offset + r * cols + c), float32 like the kernel"""
    if p <= 0.0:
        return x
    n, d = x.shape
    return x * dropout_ref.factors(n, d, p, seed, offset)


def _split_ref(x):
    """x [rows, k] float32 -> int16 [rows, kpad(k) * 3]: 16-byte chunks of 8 k of one piece, pieces 1, 2, 3"""
    rows, k = x.shape
    kp = _kpad(k)
    t = torch.zeros((rows, kp), dtype=torch.float32)
    t[:, :k] = torch.from_numpy(np.ascontiguousarray(x))
    b1 = t.to(torch.bfloat16)
    r1 = t - b1.float()
    b2 = r1.to(torch.bfloat16)
    r2 = r1 - b2.float()
    b3 = r2.to(torch.bfloat16)
    pieces = torch.stack([b.view(torch.int16).reshape(rows, kp // 8, 8) for b in (b1, b2, b3)], dim=2)
    return pieces.reshape(rows, kp * 3)


def _partials_ref(x):
    """column sums per 64 rows, s_j over rows r = j mod 4 in increasing order, (s0 + s1) + (s2 + s3)"""
    rows, d = x.shape
    out = np.zeros((-(-rows // 64), d), dtype=np.float32)
    for ch in range(out.shape[0]):
        t = np.zeros((64, d), dtype=np.float32)
        blk = x[64 * ch:64 * ch + 64]
        t[:blk.shape[0]] = blk
        s = [np.zeros(d, dtype=np.float32) for _ in range(4)]
        for r in range(0, 64, 4):
            for j in range(4):
                s[j] = s[j] + t[r + j]
        out[ch] = (s[0] + s[1]) + (s[2] + s[3])
    return out


def _source(rows, cols, ld, seed, shift=0):
    rs = np.random.RandomState(seed)
    buf = (rs.randn(rows, ld + shift) * np.exp(rs.uniform(-6, 6, (rows, ld + shift)))).astype(np.float32)
    buf[rs.rand(rows, ld + shift) < 0.01] = 0.0                # exact zeros and bf16-exact values too
    buf[rs.rand(rows, ld + shift) < 0.01] = 1.5
    dev = torch.from_numpy(buf).to(DEV)
    x = dev[:, shift:shift + cols]
    return x, buf[:, shift:shift + cols]


def _check(hip, rows, cols, ld=None, shift=0, want_r=True, want_t=True, p=0.0, seed=0, offset=0, partials=False):
    ld = cols if ld is None else ld
    x, xh = _source(rows, cols, ld, rows * 7 + cols + shift)
    dr, dt, cp = hip.b3_split(x, rows=want_r, transposed=want_t, p=p, seed=seed, offset=offset,
                              col_partials=partials)
    torch.cuda.synchronize()
    xd = _dropped(xh, p, seed, offset)
    if want_r:
        assert torch.equal(dr.cpu(), _split_ref(xd)), 'rows layout differs'
    else:
        assert dr is None
    if want_t:
        assert torch.equal(dt.cpu(), _split_ref(np.ascontiguousarray(xd.T))), 'transposed layout differs'
    else:
        assert dt is None
    if partials:
        got = cp.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), _partials_ref(xd).view(np.uint32)), 'column sums differ'


# the splits of the H = 4096 step (W0, W1, Z0 and Z1 with dropout, dY1 with both layouts, dY0 transposed only)
@pytest.mark.parametrize('rows,cols,want_r,p,partials', [
    (4096, 1204, True, 0.0, False), (4096, 8192, True, 0.0, False), (2046, 1204, True, 0.2, False),
    (2046, 8192, True, 0.2, False), (2046, 4096, True, 0.0, True), (2046, 4096, False, 0.0, True)])
def test_step_shapes(hip, rows, cols, want_r, p, partials):
    _check(hip, rows, cols, want_r=want_r, p=p, seed=11, offset=2046 * 1204 * 3, partials=partials)


@pytest.mark.parametrize('rows,cols,ld,shift', [
    (1, 1, 1, 0), (63, 65, 65, 0), (130, 77, 80, 0), (200, 129, 136, 0), (65, 64, 64, 1), (100, 70, 75, 3),
    (333, 41, 44, 0)])
def test_ragged_and_unaligned(hip, rows, cols, ld, shift):
    _check(hip, rows, cols, ld=ld, shift=shift, partials=True)


@pytest.mark.parametrize('want_r,want_t', [(True, False), (False, True)])
def test_one_layout(hip, want_r, want_t):
    _check(hip, 150, 190, ld=196, want_r=want_r, want_t=want_t)


@pytest.mark.parametrize('rows,cols,shift', [(257, 300, 0), (129, 67, 1)])
def test_dropout_odd_offset(hip, rows, cols, shift):
    _check(hip, rows, cols, ld=cols + 5, shift=shift, p=0.3, seed=12345, offset=1001, partials=True)


@pytest.mark.parametrize('want_r,want_t', [(True, True), (False, True)])
def test_dropout_odd_offset_on_the_16_byte_loads(hip, want_r, want_t):
    # 65 x 68, ld = 68, aligned: one whole 64-column tile on the float4 loads, the row and the column edge; every quad's
    # first mask index is odd (68 is even); p = 0 on the same call
    _check(hip, 65, 68, p=0.3, seed=12345, offset=1001, want_r=want_r, want_t=want_t, partials=True)
    _check(hip, 65, 68, p=0.0, seed=12345, offset=1001, want_r=want_r, want_t=want_t, partials=True)


def test_nothing_past_the_padding(hip):
    # the kernel writes [rows][kpad] exactly: canaries around both outputs stay put
    x, xh = _source(100, 70, 70, 5)
    L = __import__('gist_amd._lib', fromlist=['load']).load()
    kr, kt = _kpad(70) * 3, _kpad(100) * 3
    big_r = torch.full((100 * kr + 64,), 0x5A5A, dtype=torch.int16, device=DEV)
    big_t = torch.full((70 * kt + 64,), 0x5A5A, dtype=torch.int16, device=DEV)
    rc = L.gist_b3_split_f32(x.data_ptr(), 70, 100, 70, 0.0, 0, 0, big_r.data_ptr(), big_t.data_ptr(), None,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(big_r[:100 * kr].cpu().reshape(100, kr), _split_ref(xh))
    assert torch.equal(big_t[:70 * kt].cpu().reshape(70, kt), _split_ref(np.ascontiguousarray(xh.T)))
    assert bool((big_r[100 * kr:] == 0x5A5A).all()) and bool((big_t[70 * kt:] == 0x5A5A).all())
