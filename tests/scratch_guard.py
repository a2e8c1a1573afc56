"""Guard bands and poisons for the memory the library borrows (a plain helper module, imported by the scratch tests).

include/gist_hip.h promises two things about every buffer a caller lends a call: the call writes nothing outside the
bytes it was told about, and its results do not depend on what the buffer held before.  A Guarded buffer makes both
visible:

    [ left band >= 64 KiB | interior: nbytes | right band >= max(nbytes, 1 MiB) ]

one uint8 allocation; the interior starts at an address aligned to `align` and the right band at exactly ptr + nbytes
(byte granularity: a one-byte overrun is seen).  The right band is as long as the interior again, so a whole extra slab
or an extra transposed operand still lands inside it and not in a neighbouring allocation.  Both bands hold a fixed byte
pattern with a prime period (no constant: a stray store of one value cannot match it except by a 1/256 accident per
byte); check() compares them with the pattern and reports the first and last changed byte of each side.

poison(kind) fills the interior: 'nan' = 0xFF bytes (a NaN as fp32, fp16 and bf16, -1 as an integer: NEVER for a buffer
that holds indices, offsets or counts, where a stale read would turn into a wild gather), 'zero' = zero bytes, 'keep' =
whatever the previous call left."""
import torch

LEFT_MIN = 64 << 10
RIGHT_MIN = 1 << 20
POISONS = ('nan', 'zero', 'keep')
_PERIOD = 65521      # the largest prime below 2^16: the pattern lines up with no power-of-two stride

_tiles = {}


def _tile(device):
    """One period of the band pattern on `device`: the high byte of a multiplicative hash of the position."""
    key = str(device)
    t = _tiles.get(key)
    if t is None:
        i = torch.arange(_PERIOD, dtype=torch.int64)
        t = (((i * 40503 + 12345) >> 7) & 0xFF).to(torch.uint8).to(device)
        _tiles[key] = t
    return t


def _pattern(first, length, device):
    """Pattern bytes of the allocation's positions [first, first + length)."""
    if length == 0:
        return torch.empty(0, dtype=torch.uint8, device=device)
    tile = _tile(device)
    r = first % _PERIOD
    reps = (r + length + _PERIOD - 1) // _PERIOD
    return tile.repeat(reps)[r:r + length]


class Guarded(object):
    """nbytes of device (or CPU) memory between two patterned guard bands; see the module docstring.

    .ptr      address of the interior (what the library is given), aligned to `align`
    .nbytes   its true capacity: no caller may tell the library more
    .view(dtype)   the interior as a 1-D tensor
    .poison(kind)  'nan' | 'zero' | 'keep'
    .check()       None, or [(side, first, last)]: side 'left' with offsets < 0 relative to ptr, side 'right' with
                   offsets >= 0 relative to ptr + nbytes (0 = the first byte past the end)
    .assert_intact()   raises AssertionError naming the buffer and the distance from its end"""

    def __init__(self, nbytes, device, align=256, name='scratch'):
        nbytes = int(nbytes)
        if nbytes < 0 or align <= 0 or align & (align - 1):
            raise ValueError('Guarded: nbytes >= 0 and a power-of-two align')
        self.nbytes, self.align, self.name = nbytes, int(align), name
        self.device = torch.device(device)
        right = max(nbytes, RIGHT_MIN)
        self._buf = torch.empty(LEFT_MIN + align + nbytes + right, dtype=torch.uint8, device=self.device)
        base = self._buf.data_ptr()
        self._start = LEFT_MIN + (-(base + LEFT_MIN)) % align
        self._end = self._start + nbytes
        self.ptr = base + self._start
        assert self.ptr % align == 0 and self._end + right <= self._buf.numel()
        self.left_bytes, self.right_bytes = self._start, self._buf.numel() - self._end
        self._buf[:self._start].copy_(_pattern(0, self._start, self.device))
        self._buf[self._end:].copy_(_pattern(self._end, self.right_bytes, self.device))

    def view(self, dtype=torch.uint8):
        t = self._buf[self._start:self._end]
        return t if dtype == torch.uint8 else t.view(dtype)

    def poison(self, kind):
        if kind == 'nan':
            self.view().fill_(0xFF)
        elif kind == 'zero':
            self.view().zero_()
        elif kind != 'keep':
            raise ValueError('Guarded.poison: %r is none of %r' % (kind, POISONS))
        return self

    def _changed(self, lo, hi):
        band = self._buf[lo:hi]
        want = _pattern(lo, hi - lo, self.device)
        if torch.equal(band, want):
            return None
        at = (band != want).nonzero().flatten()
        return lo + int(at[0].item()), lo + int(at[-1].item())

    def check(self):
        found = []
        hit = self._changed(0, self._start)
        if hit is not None:
            found.append(('left', hit[0] - self._start, hit[1] - self._start))
        hit = self._changed(self._end, self._buf.numel())
        if hit is not None:
            found.append(('right', hit[0] - self._end, hit[1] - self._end))
        return found or None

    def message(self, found):
        parts = []
        for side, first, last in found:
            if side == 'right':
                parts.append('bytes %d .. %d PAST THE END of its %d bytes were written' % (first, last, self.nbytes))
            else:
                parts.append('bytes %d .. %d BEFORE ITS START were written (%d .. %d bytes before its end)'
                             % (-first, -last, self.nbytes - first, self.nbytes - last))
        return '%s: %s' % (self.name, '; '.join(parts))

    def assert_intact(self):
        found = self.check()
        assert found is None, self.message(found)


def assert_all_intact(buffers):
    """Every Guarded of an iterable (None entries skipped); one message for all that were overrun."""
    bad = []
    for g in buffers:
        if g is not None:
            found = g.check()
            if found is not None:
                bad.append(g.message(found))
    assert not bad, '\n'.join(bad)
