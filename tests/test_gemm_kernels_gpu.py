"""GPU: every kernel instantiation of the GEMM family (gemm.hip, gemm_h3.hip, gemm_b3.hip, gemm_b3c.hip) against a float64
restatement, at the smallest shapes at which it can go wrong.  The slow GEMM files (test_gemm_b3_gpu.py, test_gemm_h3_gpu.py,
test_gemm_b3c_gpu.py, ...) measure the error level at the benchmark's shapes; this one is the file to run after touching a
kernel: a few hundred small cases that fail on an index, mask, fragment or slice error in any instantiation.

The case tables are module-level data and everything but the launches is a pure function, so that
test_gemm_dispatch_coverage.py (no GPU) proves that the cases reach every instantiation (insts() against
every_instantiation()), that float32 arithmetic passes the comparators and that wrong restatements fail them.

A case is (path, mode, hooks, form, m, n, k, place, bias, call, kind, want):
  path   the plan's path name ('f32', 'f16x3', 'bf16x3', 'bf16x3_load'); mode / hooks: hip.gemm_mode and hip.tuning values
  form   'nt' / 'nn' / 'tn', or 'dual' (gist_gemm_nn_tn_dual_f32: m rows of dy, n = n1, k = k1)
  place  'tight/16', 'tight/odd', 'window/16', 'window/odd': see geom().  A window case also runs its tight twin.
  call   'call' (gist_gemm_*_f32, which reduces its own k slices) or 'slabs' (gist_gemm_slabs_f32: slices left as slabs)
  kind   the operand class of the accuracy run; every case also runs the integer class
  want   (tile_m, tile_n, splits, tail_splits) the plan must show -- a hook change then fails instead of testing another kernel

Which kernel a case runs is read from the LIBRARY (hip.gemm_plan under the case's mode and hooks: path, tile, splits > 1,
tail_splits > 1); insts() adds what the plan does not say: the layout, bias, the call form, the k tiles of every slice --
and the `aligned` predicate of the placement, which is the ONE predicate restated here by hand (aligned_of(): gemm.hip's
launch_gemm: base pointer % 16 == 0, ld % 4 == 0, ld >= 4, for both operands; the GPU tests check the base pointers).

Bounds.  fp32 kernel: DERIVED.  An fp32 MFMA is a k-ordered fmaf chain, so a term passes through at most k + s + 1 roundings
(s slices: the slab sum) and one more for the bias: |y - ref64| <= gamma (sum |a||b| + |bias|) + k 2^-149 with
gamma = N u / (1 - N u), u = 2^-24, N = k + s + 2, per output element, every element.  Split paths: the project's own bars
(test_gemm_b3_gpu.py, test_gemm_h3_gpu.py), unchanged: error relative to sum |a||b| against the fp32 kernel's on the same
operands."""
import collections
import contextlib
import zlib

import numpy as np
import pytest
import torch

from tests.test_gemm_b3_gpu import _operands, _ref64, _run, _shape

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
U = 2.0 ** -24

Case = collections.namedtuple('Case', 'path mode hooks form m n k place bias call kind want')
FORMS = ('nt', 'nn', 'tn')
HOST_KINDS = ('normal', 'integers', 'identity', 'subnormal')
DEVICE_KINDS = ('train', 'grad', 'cancel', 'range', 'edge')          # test_gemm_b3_gpu._operands, built on the GPU


def _id(c):
    hooks = ','.join('%s=%g' % h for h in c.hooks)
    return '-'.join([c.path, hooks, c.form, '%dx%dx%d' % (c.m, c.n, c.k), c.place, c.call, c.kind] + (['bias'] if c.bias else []))


# -- placement --------------------------------------------------------------------------------------------------------
def geom(rows, cols, place):
    """(elements of the flat buffer, ld, offset of element (0, 0)) of a [rows, cols] operand.
    tight/16   ld = cols rounded up to 4 (contiguous when cols % 4 == 0), zeros in the padding
    tight/odd  contiguous, one element into its buffer: a misaligned base
    window/16  ld = cols rounded up to 4, plus 4; four columns before the window, two rows before and after it
    window/odd an odd ld >= cols + 5; three columns before the window, two rows before and after it
    Everything of a window's buffer outside the window is NaN / +Inf / -Inf (poison(): read, perhaps, but never used)."""
    up4 = max(4, -(-cols // 4) * 4)
    if place == 'tight/16':
        return max(rows, 1) * up4, up4, 0
    if place == 'tight/odd':
        return 1 + max(rows, 1) * max(cols, 1) + 3, max(cols, 1), 1
    if place == 'window/16':
        return (rows + 4) * (up4 + 4), up4 + 4, 2 * (up4 + 4) + 4
    if place == 'window/odd':
        ld = (cols + 5) | 1
        return (rows + 4) * ld, ld, 2 * ld + 3
    raise ValueError(place)


def operand_shapes(c):
    if c.form == 'dual':                                  # dy [m, k1], w [k1, n1]  (z, dz [m, n1]: as the output)
        return (c.m, c.k), (c.k, c.n)
    return _shape(c.form, c.m, c.n, c.k)


def aligned_of(c, place=None):
    """gemm.hip launch_gemm's `aligned` for this case's operands in this placement (the allocation itself is 16-byte aligned)"""
    ok = True
    for rows, cols in operand_shapes(c):
        _, ld, off = geom(rows, cols, place or c.place)
        ok = ok and off % 4 == 0 and ld % 4 == 0 and ld >= 4
    return ok


def is_window(c):
    return c.place.startswith('window')


def tight_twin(c):
    return 'tight/' + c.place.split('/')[1]


def poison(n):
    return np.resize(np.array([np.nan, np.inf, -np.inf], F32), n)


# -- plans and instantiation keys ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def configured(hip, c, mode=None):
    """the case's mode and hooks; what was set before comes back afterwards (so uses may nest)"""
    prev, before = hip.gemm_mode(), [(knob, hip.tuning(knob)) for knob, _ in c.hooks]
    hip.gemm_mode(mode or c.mode)
    for knob, value in c.hooks:
        hip.tuning(knob, value)
    try:
        yield
    finally:
        for knob, value in before:
            hip.tuning(knob, value)
        hip.gemm_mode(prev)


def plan_of(hip, c, call=None, place=None):
    """the library's plan of the case (call inside configured())"""
    call = call or c.call
    if c.form == 'dual':                                  # plan_gemm_dual: dz as one NN slice, dW as the deferred TN product
        return hip.gemm_plan('tn', c.k, c.n, c.m, aligned=True, call='slabs', deferred=True)
    return hip.gemm_plan(c.form, c.m, c.n, c.k, aligned=aligned_of(c, place), call='slabs' if call == 'slabs' else 'splits',
                         deferred=call == 'slabs')


def plan_key(plan):
    return plan['tile_m'], plan['tile_n'], plan['splits'], plan['tail_splits']


def slices_of(k, k_per, bk):
    """[(k tiles, 'full' | 'ragged')] of the slices of a k range cut every k_per"""
    out = []
    for k0 in range(0, k, k_per):
        kk = min(k, k0 + k_per) - k0
        out.append((-(-kk // bk), 'full' if kk % bk == 0 else 'ragged'))
    return out


def insts(hip, c):
    """Every instantiation key the case reaches; the first is THE kernel (inst())."""
    with configured(hip, c):
        plan = plan_of(hip, c)
    tm, tn, splits, tails = plan_key(plan)
    al = aligned_of(c)
    way = 'tail units' if tails > 1 else 'one slice' if splits == 1 else 'reduced' if c.call == 'call' else 'slabs'
    win = [('window', plan['path'], c.form)] if is_window(c) else []
    if c.form == 'dual':
        return [('gemm_f32_dual_kernel', 'one slab' if splits == 1 else 'slabs')] + win
    if plan['path'] == 'f32':
        if c.k == 0:
            return [('gemm_f32_kernel', c.form, tm, False), ('f32 k == 0', 'bias' if c.bias else 'zeros')]
        keys = [('gemm_f32_kernel', c.form, tm, al), ('f32 run', c.form, tm, way)]
        keys += [('f32 k loop', tm, al) + s for s in slices_of(c.k, plan['k_per_split'], 64 if tm == 64 else 32)]
        if way == 'reduced':
            keys.append(('splitk_reduce_kernel', 'bias' if c.bias else 'no bias'))
        if c.bias:
            keys.append(('f32 bias', 'one slice' if splits == 1 else 'slices'))
        return keys + win
    if plan['path'] == 'f16x3':
        pre = {'nt': ['h3_split_rows_kernel'], 'nn': ['h3_split_rows_kernel', 'h3_colmax_kernel + h3_split_t_kernel'],
               'tn': ['h3_colmax_kernel + h3_split_t_kernel']}[c.form]
        return [('gemm_h3_kernel', tm, c.form)] + [(p,) for p in pre] + win
    if plan['path'] == 'bf16x3':
        kernel = 'gemm_b3_wide_kernel' if tn == 256 else 'gemm_b3_kernel'
        keys = [(kernel, way, c.form, 'vec4 pre-pass' if al else 'scalar pre-pass')]
        if tails > 1:
            keys.append(('gemm_b3_tail_sum_kernel',))
        if splits > 1:
            keys.append(('splitk_reduce_kernel after b3', 'bias' if c.bias else 'no bias'))
        return keys + win
    keys = [('gemm_b3c_kernel', c.form, tm, tn, way),
            ('b3c stagers', c.form, 'ragged last tile' if c.k % 32 else 'full tiles only')]
    if tails > 1:
        keys.append(('gemm_b3c_tail_sum_kernel', tm, tn))
    return keys + win


def inst(hip, c):
    return insts(hip, c)[0]


def every_instantiation():
    """Enumerated by hand from gemm.hip, gemm_h3.hip, gemm_b3.hip and gemm_b3c.hip.
    gemm.hip: gemm_f32_kernel<A_KC, B_KC, ALIGNED, T> (3 layouts x 2 x 2 = 12), each layout and tile as one slice, as
    slices reduced by the call (splitk_reduce_kernel, with and without bias) and as slabs; the k loop of gemm_f32_body per
    tile and alignment with 1 .. 6 k tiles in a slice ending in a full and in a ragged tile (cur 0 / 1, the next tile by
    DMA / through registers / none, the DMA steady loop and n_dma); bias at one slice and at several; k == 0;
    gemm_f32_dual_kernel<64> with dW as one slab and as slabs.
    gemm_h3.hip: gemm_h3_kernel<64 | 128> in the three layouts; the row split (h3_split_rows_kernel) and column maxima +
    transposing split (h3_colmax_kernel, h3_split_t_kernel).
    gemm_b3.hip: gemm_b3_kernel as one slice, as k slices (+ splitk_reduce_kernel) and with tail units
    (+ gemm_b3_tail_sum_kernel), gemm_b3_wide_kernel; each in the three layouts and with the split pre-pass
    (b3_split_kernel) on its float4 and on its scalar loads.
    gemm_b3c.hip: gemm_b3c_kernel<A_KC, B_KC, TM, TN> (3 layouts x 3 tiles = 9) as one slice, reduced, as slabs and with
    tail units (+ gemm_b3c_tail_sum_kernel per tile); the FULL and the ragged stagers per layout.
    A window placement for every path in every layout.
    NOT reachable from here (no C entry point of their own; test_e2e_gpu.py compares them with per-call splits): the step's
    kept pre-split operands -- the GEMM_CALL_KEPT host path, h3_dual_split_kernel and h3_absmax_kernel.  They run the same
    main kernels."""
    want = set()
    for form in FORMS:
        for t in (64, 128):
            want |= {('gemm_f32_kernel', form, t, al) for al in (True, False)}
            want |= {('f32 run', form, t, way) for way in ('one slice', 'reduced', 'slabs')}
            want.add(('gemm_h3_kernel', t, form))
        for way in ('one slice', 'reduced', 'tail units'):
            want |= {('gemm_b3_kernel', way, form, pre) for pre in ('vec4 pre-pass', 'scalar pre-pass')}
        want |= {('gemm_b3_wide_kernel', 'one slice', form, pre) for pre in ('vec4 pre-pass', 'scalar pre-pass')}
        for tm, tn in ((64, 64), (128, 64), (128, 128)):
            want |= {('gemm_b3c_kernel', form, tm, tn, way) for way in ('one slice', 'reduced', 'slabs', 'tail units')}
        want |= {('b3c stagers', form, s) for s in ('ragged last tile', 'full tiles only')}
        want |= {('window', path, form) for path in ('f32', 'f16x3', 'bf16x3', 'bf16x3_load')}
    for t in (64, 128):
        for al in (True, False):
            want |= {('f32 k loop', t, al, n_kt, last) for n_kt in range(1, 7) for last in ('full', 'ragged')}
    want |= {('splitk_reduce_kernel', b) for b in ('bias', 'no bias')}
    want |= {('splitk_reduce_kernel after b3', b) for b in ('bias', 'no bias')}
    want |= {('f32 bias', w) for w in ('one slice', 'slices')}
    want |= {('f32 k == 0', b) for b in ('bias', 'zeros')}
    want |= {('gemm_f32_dual_kernel', w) for w in ('one slab', 'slabs')}
    want |= {('window', 'f32', 'dual')}
    want |= {('h3_split_rows_kernel',), ('h3_colmax_kernel + h3_split_t_kernel',), ('gemm_b3_tail_sum_kernel',)}
    want |= {('gemm_b3c_tail_sum_kernel', tm, tn) for tm, tn in ((64, 64), (128, 64), (128, 128))}
    return want


# -- the case tables -------------------------------------------------------------------------------------------------------
def _edges(t):
    return (1, t - 1, t, t + 1, 2 * t + 1)


def _f32(form, t, hook_splits, m, n, k, place, splits, bias=False, call='call', kind='normal'):
    return Case('f32', 'f32', (('gemm_tile', t), ('gemm_splits', hook_splits)), form, m, n, k, place, bias and form == 'nt',
                call, kind, (t, t, splits, 1))


def _f32_cases():
    cases = []
    for t in (64, 128):
        bk, e = (64 if t == 64 else 32), _edges(t)
        for ai, al in enumerate(('16', 'odd')):
            # the k loop: one slice of 1 .. 6 k tiles, ending full and ragged (k = BK - 1, BK, BK + 1 among them)
            for j in range(1, 7):
                for ragged in (0, 1):
                    r = (1, bk - 1, 5, bk - 3, 2, bk // 2)[j - 1] if ragged else 0
                    i = j + ai + t // 64 + ragged
                    cases.append(_f32(FORMS[i % 3], t, 1, e[(i + 1) % 5], e[(2 * i + ragged) % 5], bk * j - r, 'window/' + al, 1,
                                      bias=j % 2 == 0))
            for i, k in enumerate((1, 3, 4, 5)):
                cases.append(_f32(FORMS[(i + ai) % 3], t, 1, e[(i + 3) % 5], e[(i + ai) % 5], k, 'window/' + al, 1, bias=i == 1))
            # k slices: reduced by the call (200 -> 128 + 72, 193 -> 128 + 65; 320 -> 128 + 128 + 64) and left as slabs
            for fi, form in enumerate(FORMS):
                k2 = 200 if t == 128 else 193
                cases.append(_f32(form, t, 3 if t == 128 else 2, e[(fi + ai + 2) % 5], e[(fi + 3) % 5], k2, 'window/' + al, 2,
                                  bias=ai == 0))
                cases.append(_f32(form, t, 3, e[(fi + 4) % 5], e[(fi + ai + 1) % 5], 320, 'window/' + al, 3, bias=ai == 1))
                cases.append(_f32(form, t, 3, e[(fi + ai + 3) % 5], e[(fi + 2) % 5], 320 - 9 * ai, 'window/' + al, 3, bias=fi == 0,
                                  call='slabs'))
    # the adversarial operand classes, each in every layout
    for i, kind in enumerate(DEVICE_KINDS):
        for fi, form in enumerate(FORMS):
            t = (64, 128)[(i + fi) % 2]
            cases.append(_f32(form, t, 2, t + 1, 2 * t + 1, 300, 'tight/' + ('16', 'odd')[(i + fi // 2) % 2], 2, kind=kind))
    return cases


K0_CASES = [Case('f32', 'f32', (('gemm_tile', t), ('gemm_splits', 1)), form, m, n, 0, 'window/16', bias, 'call', 'normal', (t, t, 1, 1))
            for form, t, m, n, bias in (('nt', 64, 65, 129, True), ('nt', 128, 129, 1, False), ('nn', 64, 1, 65, False),
                                        ('tn', 128, 257, 130, False))]

DUAL_CASES = [Case('f32', 'f32', (), 'dual', m, n1, k1, place, False, 'slabs', 'normal', (64, 64, slabs, 1))
              for m, n1, k1, place, slabs in ((65, 130, 70, 'window/16', 1), (96, 65, 129, 'tight/16', 1),
                                              (300, 130, 70, 'window/16', 3), (513, 200, 100, 'tight/16', 5))]

H3_HOOKS = (('h3_min_tiles', 1), ('h3_min_gflop', 1e-6))


def _h3_cases():
    cases = []
    shapes = ((129, 130), (65, 257), (130, 63), (257, 129), (1, 200), (129, 129))
    for ti, tm in enumerate((64, 128)):
        for fi, form in enumerate(FORMS):
            for i, k in enumerate((1, 31, 32, 33, 65)):
                m, n = shapes[(i + fi + ti) % len(shapes)]
                cases.append(Case('f16x3', 'f16x3', H3_HOOKS + (('h3_tm', tm),), form, m, n, k, ('window/16', 'tight/16')[i % 2],
                                  form == 'nt' and i % 2 == 0, 'call', ('normal', 'train', 'grad')[(i + fi) % 3],
                                  (tm, 128, 1, 1)))
        cases.append(Case('f16x3', 'f16x3', H3_HOOKS + (('h3_tm', tm),), 'nt', 129, 129, 33, 'window/16', True, 'call', 'normal',
                          (tm, 128, 1, 1)))
    return cases


def _b3_cases():
    cases = []
    ways = (((257, 129, 65), (256, 128, 1, 1)), ((300, 200, 1024), (256, 128, 4, 1)), ((5, 32770, 450), (256, 128, 1, 2)),
            ((3, 65300, 65), (256, 256, 1, 1)))
    for wi, ((m, n, k), want) in enumerate(ways):
        for fi, form in enumerate(FORMS):
            for ai, al in enumerate(('16', 'odd')):
                big = m * n * k > 1e8 or n > 60000
                place = ('tight/' if big and al == 'odd' else 'window/') + al
                cases.append(Case('bf16x3', 'bf16x3', H3_HOOKS, form, m, n, k, place, form == 'nt' and ai == 0, 'call', 'normal', want))
    for i, kind in enumerate(DEVICE_KINDS):                  # the adversarial classes: one slice and k slices, every layout
        form = FORMS[i % 3]
        cases.append(Case('bf16x3', 'bf16x3', H3_HOOKS, form, 257, 129, 65, 'tight/16', False, 'call', kind, (256, 128, 1, 1)))
        cases.append(Case('bf16x3', 'bf16x3', H3_HOOKS, FORMS[(i + 1) % 3], 300, 200, 1024, 'tight/odd', False, 'call', kind,
                          (256, 128, 4, 1)))
    cases.append(Case('bf16x3', 'bf16x3', H3_HOOKS, 'nt', 129, 129, 65, 'window/16', True, 'call', 'normal', (256, 128, 1, 1)))
    return cases


B3C_TILES = ((64, 64, 64), (128, 128, 64), (128128, 128, 128))      # gemm_tile hook -> TM, TN
B3C_KS = (64, 65, 67, 96, 100, 127, 129)


def _b3c_cases():
    cases = []
    for ti, (hook, tm, tn) in enumerate(B3C_TILES):
        ms, ns = (64, 65, tm + 1, 2 * tm + 1), (64, 65, tn + 1, 2 * tn + 1)
        for fi, form in enumerate(FORMS):
            for i, way in enumerate(('one', 'one', 'one', 'reduced', 'reduced', 'slabs', 'slabs')):
                k = B3C_KS[(i + fi + ti) % 7]
                hooks = (('b3c', 2), ('gemm_tile', hook)) + ((('b3c_splits', 2),) if way != 'one' else ())
                kind = 'normal' if i % 3 else DEVICE_KINDS[(i // 3 + fi + ti) % 5]
                cases.append(Case('bf16x3_load', 'bf16x3', hooks, form, ms[(i + fi) % 4], ns[(i + ti + 1) % 4], k, 'window/16',
                                  form == 'nt' and i % 2 == 1, 'slabs' if way == 'slabs' else 'call', kind,
                                  (tm, tn, 1 if way == 'one' else 2, 1)))
            # tail units: just over one round of workgroup slots, two k slices per tail tile
            m, n = {64: (65, 16400), 128: (129, 16400), 128128: (129, 16512)}[hook]
            cases.append(Case('bf16x3_load', 'bf16x3', (('b3c', 2), ('gemm_tile', hook)), form, m, n, 256, 'window/16', form == 'nt',
                              'call', 'normal', (tm, tn, 1, 2)))
        cases.append(Case('bf16x3_load', 'bf16x3', (('b3c', 2), ('gemm_tile', hook)), 'nt', 65, 65, 67, 'window/16', True, 'call',
                          'normal', (tm, tn, 1, 1)))
    return cases


F32_CASES = _f32_cases()
H3_CASES = _h3_cases()
B3_CASES = _b3_cases()
B3C_CASES = _b3c_cases()


# The block -> tile map every kernel here shares (kernel_kit.h: xcd_linear, tile_of_linear) goes wrong only at particular tile
# counts, which the edge shapes above (at most 3 tile rows) do not reach: 9 x 1 tiles of the kernel's own tile -- a second
# super-tile, one tile row deep, and 9 workgroups dealt unevenly to the 8 XCDs -- with k of two tiles; 3 x 3 tiles where no
# case above has more than 8 tiles that are no multiple of 8.  The 256 x 256 tile runs from 256 tiles on: 9 x 29.
def _tile_map_cases():
    f32 = lambda t, form, m, n, k, bias: _f32(form, t, 1, m, n, k, 'tight/16', 1, bias=bias)
    h3 = lambda tm, form, m, n, bias: Case('f16x3', 'f16x3', H3_HOOKS + (('h3_tm', tm),), form, m, n, 64, 'tight/16', bias, 'call',
                                           'normal', (tm, 128, 1, 1))
    b3 = lambda form, m, n, bias, tn: Case('bf16x3', 'bf16x3', H3_HOOKS, form, m, n, 64, 'tight/16', bias, 'call', 'normal',
                                           (256, tn, 1, 1))
    b3c = lambda hook, tm, tn, form, m, n, bias: Case('bf16x3_load', 'bf16x3', (('b3c', 2), ('gemm_tile', hook)), form, m, n, 64,
                                                      'window/16', bias, 'call', 'normal', (tm, tn, 1, 1))
    return {'f32': [f32(64, 'nt', 513, 64, 128, True), f32(128, 'nn', 1025, 128, 64, False)],
            'f16x3': [h3(64, 'nt', 513, 128, True), h3(128, 'nn', 1025, 128, False), h3(128, 'tn', 257, 257, False)],
            'bf16x3': [b3('nt', 2049, 128, True, 128), b3('nn', 2049, 7169, False, 256)],
            'bf16x3_load': [b3c(64, 64, 64, 'nt', 513, 64, True), b3c(128, 128, 64, 'nn', 1025, 64, False),
                            b3c(128128, 128, 128, 'tn', 1025, 128, False)]}


TILE_MAP_CASES = _tile_map_cases()
TABLES = {'f32': F32_CASES + K0_CASES + DUAL_CASES + TILE_MAP_CASES['f32'], 'f16x3': H3_CASES + TILE_MAP_CASES['f16x3'],
          'bf16x3': B3_CASES + TILE_MAP_CASES['bf16x3'], 'bf16x3_load': B3C_CASES + TILE_MAP_CASES['bf16x3_load']}
ALL_CASES = [c for t in TABLES.values() for c in t]


def _spread(table, n):
    """n cases per layout spread over the table (different tiles, alignments and slice counts)"""
    out = []
    for form in FORMS:
        hit = [c for c in table if c.form == form and min(c.m, c.n, c.k) >= 2 and c.m * c.n * c.k < 3e7 and is_window(c)]
        out += hit[::max(1, len(hit) // n)][:n]
    return out


IDENTITY_CASES = _spread(F32_CASES, 4) + _spread(B3_CASES, 2) + _spread(B3C_CASES, 3)
NONFINITE_CASES = _spread(F32_CASES, 6) + _spread(B3_CASES, 2) + _spread(B3C_CASES, 6)
SUBNORMAL_CASES = _spread(F32_CASES, 4)


# -- inputs (host) ---------------------------------------------------------------------------------------------------------
def _seed(c, kind):
    return zlib.crc32(repr((c.form, c.m, c.n, c.k, c.place, kind)).encode())


def inputs(c, kind=None):
    """(a, b, bias) as float32 numpy arrays, tight, in the layout's storage order"""
    kind = kind or c.kind
    rng = np.random.default_rng(_seed(c, kind))
    sa, sb = operand_shapes(c)
    if kind == 'integers':
        a, b = rng.integers(-8, 9, sa).astype(F32), rng.integers(-8, 9, sb).astype(F32)
    else:
        a, b = rng.standard_normal(sa, dtype=F32), rng.standard_normal(sb, dtype=F32)
    if kind == 'identity':                                # eye against a full-mantissa asymmetric B, exponents spread +-30
        a = np.eye(sa[0], sa[1], dtype=F32)             # (tn: stored [k, m], the transpose of eye(m, k))
        b = (b * np.exp2(rng.integers(-30, 31, sb)).astype(F32)).astype(F32)
    if kind == 'subnormal':
        a = (a * F32(2.0 ** -100) * F32(2.0 ** -30)).astype(F32)
    bias = rng.standard_normal(c.n, dtype=F32) if c.bias else None
    if kind == 'integers' and bias is not None:
        bias = rng.integers(-8, 9, c.n).astype(F32)
    return a, b, bias


def ref64(form, a, b, bias=None):
    """(float64 product, sum |a||b| (+ |bias|)) of tight numpy operands"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    if form == 'nt':
        b = b.T
    elif form == 'tn':
        a = a.T
    ref, den = a @ b, np.abs(a) @ np.abs(b)
    if bias is not None:
        ref, den = ref + bias.astype(np.float64), den + np.abs(bias.astype(np.float64))
    return ref, den


def poke_nonfinite(c, a, b):
    """one NaN and one Inf in A, one NaN in B -> (a, b, output rows touched, output column touched)"""
    a, b = a.copy(), b.copy()
    r1, r2, col, kk = c.m // 3, c.m - 1, c.n // 2, c.k // 2
    if c.form == 'tn':
        a[kk, r1], a[0, r2] = np.nan, np.inf
    else:
        a[r1, kk], a[r2, 0] = np.nan, np.inf
    if c.form == 'nt':
        b[col, c.k - 1] = np.nan
    else:
        b[c.k - 1, col] = np.nan
    return a, b, sorted({r1, r2}), col


# -- comparators -----------------------------------------------------------------------------------------------------------
def f32_bound(den, k, s):
    """per element; den = sum |a||b| + |bias|"""
    n = k + s + 2
    return n * U / (1.0 - n * U) * den + k * 2.0 ** -149


def cmp_f32(y, ref, den, k, s):
    """worst |y - ref| / bound over ALL elements (inf: a non-finite output, or an error where the bound is zero)"""
    y = np.asarray(y, np.float64)
    if y.shape != ref.shape or not np.isfinite(y).all():
        return float('inf')
    if y.size == 0:
        return 0.0
    err, bound = np.abs(y - ref), f32_bound(den, k, s)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def split_stats(y, ref, den, rms_of_ref=False):
    """(max |y - ref| / sum |a||b|, rms error / rms of sum |a||b| -- of ref for the f16x3 bars)"""
    y = np.asarray(y, np.float64)
    if y.shape != ref.shape or not np.isfinite(y).all():
        return float('inf'), float('inf')
    den = np.maximum(den, 1e-300)
    scale = ref if rms_of_ref else den
    return float((np.abs(y - ref) / den).max()), float(np.sqrt(np.mean((y - ref) ** 2)) / max(np.sqrt(np.mean(scale ** 2)), 1e-300))


def cmp_split(path, kind, y3, y1, ref, den):
    """The project's bars for a split path against the fp32 kernel's result y1 on the same operands:
    (passes, (e3, e1, r3, r1)).  bf16x3 / convert on load: test_gemm_b3_gpu.py; f16x3: test_gemm_h3_gpu.py."""
    h3 = path == 'f16x3'
    e3, r3 = split_stats(y3, ref, den, h3)
    e1, r1 = split_stats(y1, ref, den, h3)
    if h3:
        ok = e3 <= max(2.0 * e1, 5e-7) and r3 <= max(1.5 * r1, 1e-6)
    else:
        ok = e3 <= max(3.0 * e1, 6e-7) and r3 <= max((2.5 if kind == 'range' else 1.25) * r1, 5e-8)
    return bool(ok), (e3, e1, r3, r1)


def bf16_pieces(x):
    """x = p1 + p2 + p3 exactly: three bf16 values (round to nearest even), as float32 arrays"""
    out, rest = [], np.asarray(x, F32).copy()
    for _ in range(3):
        bits = rest.view(np.uint32).astype(np.uint64)
        p = (((bits + 0x7fff + ((bits >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)
        out.append(p)
        rest = (rest - p).astype(F32)
    return out


# -- GPU side --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    return h


def put(x, place):
    """a [rows, cols] float32 tensor -> the same values as a view in the placement's buffer on the GPU"""
    x = torch.as_tensor(x)
    rows, cols = x.shape
    total, ld, off = geom(rows, cols, place)
    flat = torch.from_numpy(poison(total)).to(DEV) if place.startswith('window') else torch.zeros(total, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = torch.as_strided(flat, (rows, cols), (ld, 1), off)
    view.copy_(x)
    assert (view.data_ptr() % 16 == 0) == (off % 4 == 0)
    return view


CANARY = 7.0


def out_view(m, n, window):
    """(output view, its buffer): tight and NaN-filled, or a window of a buffer of canaries"""
    if not window:
        buf = torch.full((m, n), float('nan'), device=DEV)
        return buf, buf
    buf = torch.full(((m + 3) * (n + 9),), CANARY, device=DEV)
    return torch.as_strided(buf, (m, n), (n + 9, 1), n + 9 + 5), buf


def canaries_intact(view, buf):
    if view is buf:
        return True
    b2 = buf.clone()
    torch.as_strided(b2, tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(CANARY)
    return bool((b2 == CANARY).all())


def sum_slabs(slabs, ns, m, n, bias):
    acc = torch.zeros(m, n, device=DEV)
    for s in range(ns):
        acc = acc + slabs[s * m * n:(s + 1) * m * n].view(m, n)
    return acc + bias if bias is not None else acc


def run(hip, c, a, b, bias, place, call=None, plan=None):
    """One product of the case on operands placed as `place`, under the CURRENT mode and hooks.  The launch count of the
    call is checked against `plan` when one is given.  Returns the [m, n] result (a copy)."""
    from gist_amd import _lib
    L = _lib.load()
    call = call or c.call
    av, bv = put(a, place), put(b, place)
    out, buf = out_view(c.m, c.n, place.startswith('window'))
    before = L.gist_launch_count()
    if call == 'slabs':
        need = hip.gemm_plan(c.form, c.m, c.n, c.k, aligned=aligned_of(c, place), call='slabs', deferred=True)
        slabs = torch.full((max(need['scratch_bytes'] // 4, 4),), float('nan'), device=DEV)
        ns = hip.gemm_slabs(c.form, av, bv, bias, out, slabs)
        issued = L.gist_launch_count() - before
        assert ns == need['splits'], (ns, need)
        if ns > 1:
            out.copy_(sum_slabs(slabs, ns, c.m, c.n, bias))
    else:
        getattr(hip, 'gemm_' + c.form)(*((av, bv, bias, out) if c.form == 'nt' else (av, bv, out)))
        issued = L.gist_launch_count() - before
    if plan is not None:
        assert issued == plan['launches'], (issued, plan)
    assert canaries_intact(out, buf), 'written outside the output window'
    return out.clone()


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def gpu_inputs(c, kind=None):
    kind = kind or c.kind
    if kind in DEVICE_KINDS:
        gen = torch.Generator(device=DEV).manual_seed(_seed(c, kind))
        a, b = _operands(c.form, c.m, c.n, c.k, gen, kind)
        return a, b, (torch.randn(c.n, device=DEV, generator=gen) if c.bias else None)
    return tuple(to_dev(x) for x in inputs(c, kind))


def gpu_ref64(c, a, b, bias):
    ref, den = _ref64(c.form, a, b, slice(None))
    if bias is not None:
        ref, den = ref + bias.double(), den + bias.double().abs()
    return ref.cpu().numpy(), den.cpu().numpy()


def report(c, key, ratio):
    print('gemm-kernels ratio\t%s\t%s\t%.4g' % (key, _id(c), ratio))


def check_case(hip, c):
    with configured(hip, c):
        plan = plan_of(hip, c)
        assert plan['path'] == c.path and plan_key(plan) == c.want, (plan, c)
        a, b, bias = gpu_inputs(c)
        tight = tight_twin(c)
        y = run(hip, c, a, b, bias, tight, plan=plan_of(hip, c, place=tight))
        ref, den = gpu_ref64(c, a, b, bias)
        if c.path == 'f32':
            ratio = cmp_f32(y.cpu().numpy(), ref, den, c.k, plan['splits'])
            report(c, inst(hip, c), ratio)
            assert ratio <= 1.0, (c, ratio)
        if is_window(c):
            yw = run(hip, c, a, b, bias, c.place, plan=plan)
            assert torch.equal(yw, y), 'poisoned surroundings changed the result'
        if c.call == 'slabs' and plan['splits'] > 1:      # the slabs summed in slab order = the call that reduces them
            assert torch.equal(run(hip, c, a, b, bias, tight, call='call'), y)
        if plan['tail_splits'] > 1:                       # the same bits whichever slice arrives last
            for _ in range(2):
                assert torch.equal(run(hip, c, a, b, bias, tight), y)
        if plan['tile_n'] == 256 and c.path == 'bf16x3':  # the wide tile = the narrow tile, bit for bit
            hip.tuning('b3_wide', 1)
            try:
                assert plan_of(hip, c)['tile_n'] == 128
                assert torch.equal(run(hip, c, a, b, bias, tight), y)
            finally:
                hip.tuning('b3_wide', 0)
        ai, bi, biasi = gpu_inputs(c, 'integers')         # every partial sum exact: the product bit for bit
        yi = run(hip, c, ai, bi, biasi, c.place)
        exact, _ = gpu_ref64(c, ai, bi, biasi)
        assert torch.equal(yi, torch.from_numpy(exact).float().to(DEV)), 'integer product not exact'
    if c.path != 'f32':                                   # the split bars: against the fp32 kernel on the same operands
        with configured(hip, c, mode='f32'):
            p1 = plan_of(hip, c, place=tight)
            assert p1['path'] == 'f32'
            y1 = run(hip, c, a, b, bias, tight)
        r1 = cmp_f32(y1.cpu().numpy(), ref, den, c.k, p1['splits'])
        assert r1 <= 1.0, (c, r1)
        ok, stats = cmp_split(c.path, c.kind, y.cpu().numpy(), y1.cpu().numpy(), ref, den)
        limit_e = max((2.0 if c.path == 'f16x3' else 3.0) * stats[1], 5e-7 if c.path == 'f16x3' else 6e-7)
        report(c, inst(hip, c), stats[0] / limit_e)
        print('   e3 %.3g e1 %.3g r3 %.3g r1 %.3g' % stats)
        assert ok, (c, stats)


@pytest.mark.parametrize('case', F32_CASES + TILE_MAP_CASES['f32'], ids=_id)
def test_f32_kernel(hip, case):
    check_case(hip, case)


@pytest.mark.parametrize('case', H3_CASES + TILE_MAP_CASES['f16x3'], ids=_id)
def test_f16x3_kernels(hip, case):
    check_case(hip, case)


@pytest.mark.parametrize('case', B3_CASES + TILE_MAP_CASES['bf16x3'], ids=_id)
def test_bf16x3_kernels(hip, case):
    check_case(hip, case)


@pytest.mark.parametrize('case', B3C_CASES + TILE_MAP_CASES['bf16x3_load'], ids=_id)
def test_bf16x3_convert_on_load_kernel(hip, case):
    check_case(hip, case)


@pytest.mark.parametrize('case', K0_CASES, ids=_id)
def test_f32_k_zero_is_the_bias_or_zeros(hip, case):
    """k == 0: the bias, or zeros, from the generic instantiation.  An empty tensor has no address, so the operands are
    poisoned buffers handed to the C entry points directly: with k == 0 nothing of them may be read."""
    from gist_amd import _lib
    L = _lib.load()
    c = case
    bias = to_dev(inputs(c)[2])
    junk = torch.from_numpy(poison(4096)).to(DEV)
    out, buf = out_view(c.m, c.n, True)
    with configured(hip, c):
        plan = plan_of(hip, c)
        assert plan['path'] == 'f32' and plan_key(plan) == c.want and plan['launches'] == 1
        before = L.gist_launch_count()
        ap, bp, op, ldo, st = junk.data_ptr(), junk.data_ptr() + 2048 * 4, out.data_ptr(), out.stride(0), hip._stream()
        if c.form == 'nt':
            rc = L.gist_gemm_nt_f32(ap, 4, bp, 4, None if bias is None else bias.data_ptr(), op, ldo, c.m, c.n, 0, None, 0, st)
        elif c.form == 'nn':
            rc = L.gist_gemm_nn_f32(ap, 4, bp, c.n + 3, op, ldo, c.m, c.n, 0, None, 0, st)
        else:
            rc = L.gist_gemm_tn_f32(ap, c.m + 3, bp, c.n + 3, op, ldo, c.m, c.n, 0, None, 0, st)
        _lib.check(rc, 'gist_gemm_%s_f32' % c.form)
        assert L.gist_launch_count() - before == 1
    want = bias.expand(c.m, c.n) if bias is not None else torch.zeros(c.m, c.n, device=DEV)
    assert torch.equal(out, want) and canaries_intact(out, buf)


@pytest.mark.parametrize('case', IDENTITY_CASES, ids=_id)
def test_identity_reproduces_every_bit(hip, case):
    """eye . B = B: a full-mantissa asymmetric B with exponents spread +-30 comes back bit for bit (b1 + b2 + b3 = b on the
    bf16x3 paths); rows past the identity's diagonal are zero.  Catches a swapped fragment or C/D map and a lost piece."""
    c = case._replace(bias=False, kind='identity')
    a, b, _ = gpu_inputs(c)
    with configured(hip, c):
        assert plan_of(hip, c)['path'] == c.path
        y = run(hip, c, a, b, None, c.place)
    blog = b.t() if c.form == 'nt' else b                 # [k, n]
    want = torch.zeros(c.m, c.n, device=DEV)
    r = min(c.m, c.k)
    want[:r] = blog[:r]
    assert torch.equal(y.view(torch.int32)[:r], want.view(torch.int32)[:r]) and (y[r:] == 0).all()


@pytest.mark.parametrize('case', NONFINITE_CASES, ids=_id)
def test_non_finite_inputs_stay_in_their_row(hip, case):
    """One NaN and one Inf in A, one NaN in B: those output rows and that column are non-finite, every other element has the
    bits of the clean run (no masking by multiplication, no shared scale)."""
    c = case._replace(kind='normal')
    a, b, bias = inputs(c)
    a2, b2, rows, col = poke_nonfinite(c, a, b)
    with configured(hip, c):
        assert plan_of(hip, c)['path'] == c.path
        clean = run(hip, c, to_dev(a), to_dev(b), to_dev(bias), c.place)
        y = run(hip, c, to_dev(a2), to_dev(b2), to_dev(bias), c.place)
    touched = torch.zeros(c.m, c.n, dtype=torch.bool, device=DEV)
    touched[rows] = True
    touched[:, col] = True
    assert torch.isfinite(clean).all()
    assert not torch.isfinite(y[touched]).any()
    assert torch.equal(y[~touched], clean[~touched])


@pytest.mark.parametrize('case', SUBNORMAL_CASES, ids=_id)
def test_f32_subnormal_operands_are_not_flushed(hip, case):
    """A = normal values x 2^-130 (subnormal), B of order 1: fp32 MFMA inputs are not flushed (the build passes no flush
    flag), so the result meets the derived bound through its absolute term k 2^-149 -- and is not zero."""
    c = case._replace(kind='subnormal', bias=False)
    a, b, _ = gpu_inputs(c)
    with configured(hip, c):
        plan = plan_of(hip, c)
        y = run(hip, c, a, b, None, c.place).cpu().numpy()
    ref, den = gpu_ref64(c, a, b, None)
    ratio = cmp_f32(y, ref, den, c.k, plan['splits'])
    report(c, ('subnormal',) + inst(hip, c), ratio)
    assert (y[np.abs(ref) > 2 * f32_bound(den, c.k, plan['splits'])] != 0).all() and np.count_nonzero(y) > 0
    assert ratio <= 1.0, (c, ratio)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('splits', [1, 2])
def test_b3c_tiles_agree_bitwise(hip, form, splits):
    """the three tiles of the convert-on-load kernel form every output element from the same terms in the same order"""
    got = []
    for hook, tm, tn in B3C_TILES:
        c = Case('bf16x3_load', 'bf16x3', (('b3c', 2), ('gemm_tile', hook), ('b3c_splits', splits)), form, 129, 257, 129,
                 'tight/16', form == 'nt', 'call', 'normal', (tm, tn, splits, 1))
        a, b, bias = gpu_inputs(c)                        # (the seed does not depend on the hooks: the same operands)
        with configured(hip, c):
            plan = plan_of(hip, c)
            assert plan['path'] == c.path and plan_key(plan) == c.want, plan
            got.append(run(hip, c, a, b, bias, c.place, plan=plan))
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def _dual_run(hip, c, dy, w, z, place):
    from gist_amd import _lib
    L = _lib.load()
    m, n1, k1 = c.m, c.n, c.k
    dyv, wv, zv = put(dy, place), put(w, place), put(z, place)
    # (dz must be 16-byte aligned with a pitch % 4 == 0 for this entry point: a window of its own)
    dzbuf = torch.full(((m + 3) * (n1 + 12 - n1 % 4),), CANARY, device=DEV)
    dz = torch.as_strided(dzbuf, (m, n1), (n1 + 12 - n1 % 4, 1), n1 + 12 - n1 % 4 + 4)
    dw, dwbuf = out_view(k1, n1, True)
    assert hip.gemm_dual_takes(dyv, wv, zv, dz)
    slabs = torch.full((max(plan_of(hip, c)['scratch_bytes'] // 4, 4),), float('nan'), device=DEV)
    before = L.gist_launch_count()
    ns = hip.gemm_nn_tn_dual(dyv, wv, dz, zv, dw, slabs)
    assert L.gist_launch_count() - before == 1
    assert ns == c.want[2], ns
    assert canaries_intact(dz, dzbuf) and canaries_intact(dw, dwbuf)
    if ns > 1:
        assert (dw == CANARY).all()
        dwr = sum_slabs(slabs, ns, k1, n1, None)
    else:
        dwr = dw.clone()
    return dz.clone(), dwr, (dyv, wv, zv)


@pytest.mark.parametrize('case', DUAL_CASES, ids=_id)
def test_f32_dual_kernel(hip, case):
    """dz = dy . w and dW = dy^T . z in one launch: both against float64 under the fp32 bound, bit-equal to the two separate
    launches, exact on integers, untouched by poisoned surroundings; a NaN and an Inf in dy poison their rows of dz and
    their rows of dW, a NaN in z its column of dW, and nothing else."""
    c = case
    m, n1, k1 = c.m, c.n, c.k
    rng = np.random.default_rng(_seed(c, 'dual'))
    dy, w, z = (rng.standard_normal(s, dtype=F32) for s in ((m, k1), (k1, n1), (m, n1)))
    with configured(hip, c):
        plan = plan_of(hip, c)
        assert plan['path'] == 'f32' and plan_key(plan) == c.want, plan
        dz, dw, (dyv, wv, zv) = _dual_run(hip, c, dy, w, z, tight_twin(c))
        for name, y, (ref, den), k, s in (('dz', dz, ref64('nn', dy, w), k1, 1), ('dW', dw, ref64('tn', dy, z), m, plan['splits'])):
            ratio = cmp_f32(y.cpu().numpy(), ref, den, k, s)
            report(c, inst(hip, c) + (name,), ratio)
            assert ratio <= 1.0, (name, ratio)
        # the two separate launches: the same body, the same bits
        assert torch.equal(_run(hip, 'nn', dyv, wv, None, m, n1), dz)
        slabs = torch.full((max(plan['scratch_bytes'] // 4, 4),), float('nan'), device=DEV)
        sep_w = torch.full((k1, n1), float('nan'), device=DEV)
        ns = hip.gemm_slabs('tn', dyv, zv, None, sep_w, slabs)
        assert ns == plan['splits']
        assert torch.equal(sum_slabs(slabs, ns, k1, n1, None) if ns > 1 else sep_w, dw)
        if is_window(c):
            dz2, dw2, _ = _dual_run(hip, c, dy, w, z, c.place)
            assert torch.equal(dz2, dz) and torch.equal(dw2, dw)
        ints = [rng.integers(-8, 9, s).astype(F32) for s in ((m, k1), (k1, n1), (m, n1))]
        dzi, dwi, _ = _dual_run(hip, c, ints[0], ints[1], ints[2], c.place)
        assert torch.equal(dzi, to_dev(ref64('nn', ints[0], ints[1])[0].astype(F32)))
        assert torch.equal(dwi, to_dev(ref64('tn', ints[0], ints[2])[0].astype(F32)))
        dy2, z2 = dy.copy(), z.copy()
        dy2[m // 3, k1 // 2], dy2[m - 1, 0], z2[m // 2, n1 - 1] = np.nan, np.inf, np.nan
        dzn, dwn, _ = _dual_run(hip, c, dy2, w, z2, c.place)
    bad_z = torch.zeros(m, n1, dtype=torch.bool, device=DEV)
    bad_z[[m // 3, m - 1]] = True
    bad_w = torch.zeros(k1, n1, dtype=torch.bool, device=DEV)
    bad_w[[k1 // 2, 0]] = True
    bad_w[:, n1 - 1] = True
    assert not torch.isfinite(dzn[bad_z]).any() and torch.equal(dzn[~bad_z], dz[~bad_z])
    assert not torch.isfinite(dwn[bad_w]).any() and torch.equal(dwn[~bad_w], dw[~bad_w])
