"""GPU: the grouped block mover (gist_arena_moves_f32, gist_amd/csrc/arena_moves.hip) against the per-tensor entry points
it replaces -- gist_block_gather_f32, gist_block_scatter_f32, gist_mean_rows_f32 -- bit for bit (torch.equal), inside a
guarded destination (tests/scratch_guard.py) whose untouched cells and bands keep their bits.

Every case is ONE grouped launch over a list of moves laid out back to back in two flat arenas, and the same moves one
by one through the per-tensor calls on a clone of the destination.  The shapes are the smallest that reach every path: a
tile is 8 rows x 1024 columns (a MEAN tile 256 columns), the 16-byte path needs identity columns and offsets, pitches
and width in multiples of four floats."""
import numpy as np
import pytest
import torch

from tests.scratch_guard import Guarded

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


class Layout(object):
    """Moves laid out back to back in a src and a dst arena; `odd`: the next block starts at an odd float offset."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.src_len = self.dst_len = 0
        self.pool = []
        self.pool_len = 0
        self.moves = []          # (kind, src_off, dst_off, lds, ldd, n_rows, n_cols, row start, col start)
        self.refs = []           # the same move for the per-tensor entry points

    def _take(self, side, n, odd):
        off = getattr(self, side)
        off += (1 - off % 2) if odd else (-off) % 4
        setattr(self, side, off + n)
        return off

    def _list(self, n, upper):
        idx = self.rs.permutation(upper)[:n].astype(np.int32)
        start = self.pool_len
        self.pool.append(idx)
        self.pool_len += n
        return start, idx

    def block(self, kind, nr, nc, rows=False, cols=False, odd=False, pad=None):
        """A gather or scatter of an [nr, nc] block; the indexed side has 3 more rows / 5 more columns than the block
        where it has a list; pad: extra floats of both pitches (default: odd -> 3, else 4)."""
        pad = (3 if odd else 4) if pad is None else pad
        R, C = nr + (3 if rows else 0), nc + (5 if cols else 0)
        ld_ix, ld_dense = C + pad, nc + pad
        ix_side, dense_side = ('src_len', 'dst_len') if kind == 'gather' else ('dst_len', 'src_len')
        ix_off = self._take(ix_side, max(R * ld_ix, 1), odd)
        dense_off = self._take(dense_side, max(nr * ld_dense, 1), odd)
        rs, ri = self._list(nr, R) if rows else (-1, None)
        cs, ci = self._list(nc, C) if cols else (-1, None)
        if kind == 'gather':
            self.moves.append((kind, ix_off, dense_off, ld_ix, ld_dense, nr, nc, rs, cs))
        else:
            self.moves.append((kind, dense_off, ix_off, ld_dense, ld_ix, nr, nc, rs, cs))
        self.refs.append((kind, ix_off, (R, C, ld_ix), dense_off, (nr, nc, ld_dense), ri, ci))
        return self

    def mean(self, n_src, n, odd=False):
        stride = n + (3 if odd else 4)
        s = self._take('src_len', n_src * stride, odd)
        d = self._take('dst_len', max(n, 1), odd)
        self.moves.append(('mean', s, d, stride, 0, n_src, n, -1, -1))
        self.refs.append(('mean', s, stride, d, n_src, n))
        return self


def strided(flat, off, rows, cols, ld):
    return flat.as_strided((rows, cols), (ld, 1), flat.storage_offset() + off)


def run_case(hip, lay, shift=0):
    """Both movers over the layout; returns (the table, the guarded destination, the per-tensor destination).  shift: both
    arenas start that many floats behind a 256-byte boundary (1: bases that allow no 16-byte access, whatever the
    table's moves allow)."""
    src = torch.randn(max(lay.src_len, 4) + shift, device=DEV)[shift:]
    n_dst = max(lay.dst_len, 4)
    guard = Guarded((n_dst + shift) * 4, DEV, name='dst arena')
    got = guard.view(torch.float32)[shift:]
    assert src.data_ptr() % 256 == 4 * shift == got.data_ptr() % 256
    got.copy_(torch.randn(n_dst, device=DEV))
    want = got.clone()
    pool = torch.from_numpy(np.concatenate(lay.pool)).to(DEV) if lay.pool else None
    table = hip.ArenaMoves(lay.moves, src.numel(), n_dst, lay.pool_len, DEV)
    hip.arena_moves(table, pool, src, got)
    for ref in lay.refs:
        if ref[0] == 'mean':
            _, s, stride, d, n_src, n = ref
            hip.mean_rows(src[s:], stride, n_src, n, want[d:d + n])
            continue
        kind, ix_off, (R, C, ld_ix), dense_off, (nr, nc, ld_dense), ri, ci = ref
        if nr == 0 or nc == 0:
            continue
        ri = None if ri is None else torch.from_numpy(ri).to(DEV)
        ci = None if ci is None else torch.from_numpy(ci).to(DEV)
        if kind == 'gather':
            hip.block_gather(strided(src, ix_off, R, C, ld_ix), ri, ci, strided(want, dense_off, nr, nc, ld_dense))
        else:
            hip.block_scatter(strided(src, dense_off, nr, nc, ld_dense), ri, ci, strided(want, ix_off, R, C, ld_ix))
    torch.cuda.synchronize()
    guard.assert_intact()
    return table, got, want


def mixed(n_moves, seed):
    """n_moves moves of mixed kinds, sizes, lists and alignments."""
    lay = Layout(seed)
    rs = np.random.RandomState(seed + 100)
    sizes = [(1, 1), (1, 37), (37, 1), (9, 3), (5, 255), (3, 256), (2, 257), (17, 12), (8, 64), (4, 1028)]
    for m in range(n_moves):
        nr, nc = sizes[rs.randint(len(sizes))]
        k = rs.randint(5)
        if k == 4:
            lay.mean(int(rs.randint(1, 6)), nc, odd=bool(rs.randint(2)))
        else:
            lay.block('gather' if k < 2 else 'scatter', nr, nc, rows=bool(rs.randint(2)), cols=bool(rs.randint(2)),
                      odd=bool(rs.randint(2)))
    return lay


def shapes(kind):
    """Every shape, list combination and alignment the issue names, in one call per kind."""
    lay = Layout(7)
    for nr, nc in ((1, 1), (1, 300), (300, 1)):                          # 1 x 1, 1 x n, n x 1
        lay.block(kind, nr, nc, rows=True, cols=True, odd=True)
        lay.block(kind, nr, nc)
    for nc in (3, 255, 256, 257, 1025):                                  # around a wave, a workgroup, a tile's columns
        for rows, cols in ((False, True), (True, False), (True, True), (False, False)):
            lay.block(kind, 3, nc, rows=rows, cols=cols, odd=nc % 2 == 1)
    for nr in (7, 8, 9, 17):                                             # across a tile's row group
        lay.block(kind, nr, 20, rows=True, cols=True)
        lay.block(kind, nr, 20, rows=True)                               # identity columns, multiples of four: 16-byte path
        lay.block(kind, nr, 20, odd=True)                                # the same block at an odd offset and pitch: scalar
    lay.block(kind, 9, 2052, rows=True)                                  # 16-byte path over three column chunks
    lay.block(kind, 9, 2052, pad=6)                                      # pitches 2 mod 4: scalar
    return lay


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as _hip
    return _hip


@pytest.mark.parametrize('shift', [0, 1, 2])
@pytest.mark.parametrize('kind', ['gather', 'scatter'])
def test_every_shape_against_the_per_tensor_mover(hip, kind, shift):
    """shift 1, 2: the arenas themselves start 4 / 8 bytes behind a 16-byte boundary, as a slice of a larger tensor
    does: the moves whose offsets, pitches and width allow 16-byte accesses take the scalar path all the same."""
    lay = shapes(kind)
    table, got, want = run_case(hip, lay, shift)
    assert table.n_moves == len(lay.moves) and table.n_tiles >= table.n_moves
    assert torch.equal(got, want)


@pytest.mark.parametrize('n_moves', [0, 1, 2, 37])
def test_mixed_moves_in_one_call(hip, n_moves):
    from gist_amd import _lib
    lay = mixed(n_moves, 20 + n_moves)
    before = _lib.load().gist_launch_count()
    table, got, want = run_case(hip, lay)
    assert table.n_moves == n_moves and (table.n_tiles == 0) == (n_moves == 0)
    assert torch.equal(got, want)
    if n_moves == 0:                   # no tiles: no launch at all
        assert _lib.load().gist_launch_count() == before


def test_a_zero_sized_move_between_two_real_ones(hip):
    for empty in ((0, 9), (9, 0), (0, 0)):
        lay = Layout(3).block('gather', 9, 33, rows=True, cols=True)
        lay.block('scatter', empty[0], empty[1]).mean(1, 0)
        lay.block('scatter', 5, 40, rows=True, odd=True)
        table, got, want = run_case(hip, lay)
        assert table.n_moves == 4 and table.n_tiles == 2 + 0 + 0 + 1
        assert torch.equal(got, want)


@pytest.mark.parametrize('n_src', [1, 2, 3, 64, 65])
def test_mean_has_the_bits_of_mean_rows(hip, n_src):
    lay = Layout(n_src)
    for n, odd in ((1, False), (255, True), (257, False), (600, True)):
        lay.mean(n_src, n, odd=odd)
    lay.block('gather', 4, 8)                                            # (a MEAN beside another kind)
    table, got, want = run_case(hip, lay)
    assert table.n_tiles == 1 + 1 + 2 + 3 + 1
    assert torch.equal(got, want)
    # identical copies, a power-of-two count: the mean is the copy, bit for bit
    if n_src in (1, 2, 64):
        row = torch.randn(260, device=DEV)
        src = row.repeat(n_src)
        out = torch.zeros(260, device=DEV)
        t = hip.ArenaMoves([('mean', 0, 0, 260, 0, n_src, 260, -1, -1)], src.numel(), 260, 0, DEV)
        hip.arena_moves(t, None, src, out)
        assert torch.equal(out, row)


def test_a_destination_beyond_2_to_the_31_floats(hip):
    """All offset arithmetic is 64-bit: one scatter and one gather whose dst_off lies beyond 2^31 floats (the ultra-wide
    base has 2.2 G), in an uninitialised buffer; only the blocks are read back."""
    far = (1 << 31) + 12345
    nr, nc, R, C = 9, 70, 12, 75
    ld = C + 2
    dst = torch.empty(far + R * ld + 8 + nr * nc, dtype=torch.float32, device=DEV)
    src = torch.randn(nr * nc + R * ld, device=DEV)
    rs = np.random.RandomState(1)
    ri, ci = rs.permutation(R)[:nr].astype(np.int32), rs.permutation(C)[:nc].astype(np.int32)
    pool = torch.from_numpy(np.concatenate([ri, ci])).to(DEV)
    far2 = far + R * ld + 8
    moves = [('scatter', 0, far, nc, ld, nr, nc, 0, nr),
             ('gather', nr * nc, far2, ld, nc, nr, nc, 0, nr)]
    strided(dst, far, R, C, ld).fill_(-1.0)
    table = hip.ArenaMoves(moves, src.numel(), dst.numel(), pool.numel(), DEV)
    hip.arena_moves(table, pool, src, dst)
    want = torch.full((R, C), -1.0, device=DEV)
    hip.block_scatter(src[:nr * nc].view(nr, nc), pool[:nr], pool[nr:], want)
    assert torch.equal(strided(dst, far, R, C, ld), want)
    want2 = torch.empty(nr, nc, device=DEV)
    hip.block_gather(strided(src, nr * nc, R, C, ld), pool[:nr], pool[nr:], want2)
    assert torch.equal(dst[far2:far2 + nr * nc].view(nr, nc), want2)
    assert table.n_tiles == 4


def test_the_wrapper_refuses_what_the_table_was_not_built_for(hip):
    t = hip.ArenaMoves([('gather', 0, 0, 8, 8, 2, 8, 0, -1)], 64, 64, 4, DEV)
    src, dst = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match='idx is None'):
        hip.arena_moves(t, None, src, dst)
    with pytest.raises(ValueError, match='too small'):
        hip.arena_moves(t, torch.zeros(4, dtype=torch.int32, device=DEV), src[:32], dst)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.arena_moves(t, torch.zeros(4, dtype=torch.int32, device=DEV), src.cpu(), dst)
    both = torch.zeros(200, device=DEV)                  # one arena as both: refused (the contract: no overlap at all)
    with pytest.raises(ValueError, match='overlap'):
        hip.arena_moves(t, torch.zeros(4, dtype=torch.int32, device=DEV), both[:64], both[63:127])
    hip.arena_moves(t, torch.zeros(4, dtype=torch.int32, device=DEV), both[:64], both[64:128])      # adjacent: fine
