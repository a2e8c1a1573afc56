"""GPU: every entry point that borrows scratch keeps the two promises of include/gist_hip.h's conventions block -- it
writes nothing outside the bytes it was told about, and its results do not depend on what those bytes held before.

Every case calls the C ABI (gist_amd._lib.load()) with its own pointers and byte counts -- never the wrappers of
gist_amd/hip.py, whose grow-only workspace of at least 1 MiB hides the size.  The scratch and the output each sit in a
tests.scratch_guard.Guarded window.  A case runs at several capacities (CAPACITY_KINDS: what the size query reports, one
byte less, half, nothing with a NULL pointer, and 2 * need + 4 because a launcher may plan more slices when it sees more
room); the library is always told the TRUE capacity.  At every capacity the call runs with the scratch full of 0xFF bytes
(NaN in every float format), of zeros, and of what a larger call of the same entry point left there, and then

  (a) the guard bands of scratch and output are intact;
  (b) the output is bit for bit the same under the three poisons;
  (c) the 0xFF run meets the float64 bound the operation has in its own test file (reference and bound imported from
      there: no tolerance is introduced here);
  and where the capacity makes the launcher refuse, the code is negative and no output or band byte changed.

Buffers that hold indices, offsets or counts (the prepared block structure, the extraction's scratch) are never filled
with 0xFF: a stale read there would be a wild gather.  They get zeros, or the structure of a larger earlier call.

COVERED maps every (export, scratch parameter) this file guards to its test; tests/test_scratch_guard.py checks that the
header's scratch-taking exports are all here, in the step-level file, or exempted with a reason.

What was found (MI355X):
  * every call of every case below is bitwise the same under all three poisons -- none had to be held to (c) alone --
    and no band byte was ever written: no overrun, no stale read;
  * gist_standard_scaler_f32 was wrong on its own, whatever the scratch held: it formed its mean as sum * (1 / count), which
    misses the mean of a CONSTANT column by an ulp for about one row count in five (300 fit rows of -3.5: -3.5000000000000004);
    the variance was then 1e-31 instead of 0 and the column came out as +-1 where sklearn's StandardScaler gives 0.  The
    case with 300 fit rows below failed on it (the three row counts of tests/test_kernels_gpu.py happen to be exact).
    Fixed in prep.hip: the statistics are sum / count, as numpy's;
  * a launcher that is given too little scratch falls back (the gist_gemm_* family, gist_gemm_slabs_f32,
    gist_gemm_nn_tn_dual_f32: fewer slices, down to none) or refuses before any launch.  The refusals of
    gist_ln_affine_bwd_f32, gist_standard_scaler_f32 and gist_spmm_blocks_prepare answer GIST_EINVAL, not the
    GIST_ENOSPACE the header's table of codes names for "workspace too small"; tests/test_graphsage_surface.py pins that
    code for the first, so the cases here hold those three to "a negative code, nothing written" and
    gist_gat_attn_grad_f32 to GIST_ENOSPACE.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.scratch_guard import Guarded, assert_all_intact
from tests.test_gemm_plan_gpu import CASES as PLAN_CASES
from tests.test_gemm_b3_gpu import _operands, _ref64
from tests import test_rowops_kernels_gpu as R
from tests import test_gemm_kernels_gpu as GK
from tests import test_ln_affine_kernels_gpu as LA
from tests import test_ln_all_kernels_gpu as LN
from tests.test_kernels_gpu import _dropout_mask_ref, _sibling_graph, close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
GIST_EINVAL, GIST_ENOSPACE = -1, -3
CAPACITY_KINDS = ('need', 'need-1', 'half', 'null', 'double+4')
FLOAT_POISONS = ('nan', 'zero', 'keep')
INDEX_POISONS = ('zero', 'keep')

# (export, scratch parameter) -> the test below that guards it
COVERED = {
    ('gist_gemm_nt_f32', 'workspace'): 'test_gemm_plan_cases',
    ('gist_gemm_nn_f32', 'workspace'): 'test_gemm_plan_cases',
    ('gist_gemm_tn_f32', 'workspace'): 'test_gemm_plan_cases',
    ('gist_gemm_slabs_f32', 'slabs'): 'test_gemm_slabs',
    ('gist_gemm_nn_dropout_f32', 'workspace'): 'test_gemm_nn_dropout',
    ('gist_gemm_nn_dropout_colsum_f32', 'workspace'): 'test_gemm_nn_dropout',
    ('gist_gemm_nn_dropout_colsum_f32', 'g_col_partials'): 'test_gemm_nn_dropout',
    ('gist_gemm_nn_tn_dual_f32', 'slabs'): 'test_gemm_nn_tn_dual',
    ('gist_colsum_f32', 'partials'): 'test_colsum',
    ('gist_colsum_chunks_f32', 'partials'): 'test_colsum',
    ('gist_ln_affine_bwd_f32', 'workspace'): 'test_ln_affine_bwd',
    ('gist_ln_all_fwd_f32', 'partials'): 'test_ln_all',
    ('gist_ln_all_bwd_f32', 'partials'): 'test_ln_all',
    ('gist_standard_scaler_f32', 'workspace'): 'test_standard_scaler',
    ('gist_gat_attn_grad_f32', 'partials'): 'test_gat_attn_grad',
    ('gist_spmm_blocks_prepare', 'prepared'): 'test_spmm_blocks_prepare',
    ('gist_extract_parts_batch', 'scratch'): 'test_extract_parts_scratch',
    ('ExtractPartsDesc', 'scratch'): 'test_extract_parts_scratch',      # gist_extract_parts_desc_batch
}


def capacities(need):
    """[(kind, bytes)] of CAPACITY_KINDS for a size query's answer, without repeats (need = 0: nothing, and 4 bytes)."""
    out, seen = [], set()
    for kind, cap in zip(CAPACITY_KINDS, (need, need - 1, need // 2, 0, 2 * need + 4)):
        if cap >= 0 and cap not in seen:
            seen.add(cap)
            out.append((kind, cap))
    return out


def gemm_capacities(L, form, m, n, k):
    """The capacity table of a gist_gemm_{nt,nn,tn}_f32 case in the CURRENT mode and hooks (the CPU mutation check reads
    it too): [(kind, bytes, plan for that many bytes)]."""
    from gist_amd import hip
    need = hip.gemm_plan(form, m, n, k)['workspace_bytes']
    return [(kind, cap, hip.gemm_plan(form, m, n, k, scratch_bytes=cap)) for kind, cap in capacities(need)]


def plan_fits(plan, cap):
    """Does everything the plan puts into the workspace lie inside `cap` bytes?"""
    ends = [plan['operand_offset'] + plan['operand_bytes'] if plan['operand_bytes'] else 0,
            plan['scratch_offset'] + plan['scratch_bytes'] if plan['scratch_bytes'] else 0]
    return max(ends) <= cap


@pytest.fixture(scope='module')
def L():
    from gist_amd import _lib, hip
    assert hip.device_count() >= 1
    return _lib.load()


def _st():
    from gist_amd import hip
    return hip._stream()


def bits(t):
    return t.contiguous().view(torch.int32)


class Out(object):
    """An output operand [rows, cols] fp32 (dense) in its own Guarded window, refilled with NaN before every call."""

    def __init__(self, rows, cols, name, dtype=torch.float32):
        self.shape, self.dtype = (rows, cols), dtype
        self.g = Guarded(rows * cols * torch.empty(0, dtype=dtype).element_size(), DEV, name=name)
        self.t = self.g.view(dtype).view(rows, cols) if rows * cols else torch.empty(rows, cols, dtype=dtype, device=DEV)
        self.ptr = self.g.ptr

    def reset(self):
        self.g.poison('nan')
        return self


def under_poisons(scratch, poisons, run, prime, outs, what, extra=None):
    """run() once per poison of `scratch` (a Guarded or None; 'keep' = after prime(), a larger call into the same
    scratch); after every call the bands of scratch and outputs are intact.  -> {poison: [clone of every output]}, all
    bitwise equal; extra() -> further tensors to keep and compare (results that live in the scratch itself)."""
    got = {}
    for kind in poisons:
        if scratch is not None:
            if kind == 'keep':
                scratch.poison('nan' if 'nan' in poisons else 'zero')
                rc = prime()
                torch.cuda.synchronize()
                assert rc == 0, '%s: the larger call before it: code %d' % (what, rc)
                assert_all_intact([scratch] + [o.g for o in outs])
            else:
                scratch.poison(kind)
        for o in outs:
            o.reset()
        rc = run()
        torch.cuda.synchronize()
        assert rc == 0, '%s under %r: code %d' % (what, kind, rc)
        assert_all_intact([scratch] + [o.g for o in outs])
        got[kind] = [o.t.clone() for o in outs] + ([t.clone() for t in extra()] if extra else [])
    first = got[poisons[0]]
    for kind in poisons[1:]:
        assert len(first) == len(got[kind])
        for i, (a, b) in enumerate(zip(first, got[kind])):
            name = outs[i].g.name if i < len(outs) else 'the result kept in the scratch'
            assert a.shape == b.shape and torch.equal(bits(a), bits(b)), \
                '%s: %s differs between the %r and %r scratch' % (what, name, poisons[0], kind)
    return got


def floats_of(guard, count):
    """the first `count` floats of a Guarded whose byte count need not be a multiple of 4"""
    return guard.view()[:4 * count].view(torch.float32)


def spill(guard, big):
    """what a larger call left in its own (larger) buffer, as far as the Guarded reaches: the 'keep' poison of a buffer
    whose size is exact, so the larger call itself cannot run in it"""
    src = big.view(torch.uint8) if big.dtype != torch.uint8 else big
    k = min(src.numel(), guard.nbytes)
    guard.view()[:k].copy_(src.reshape(-1)[:k])


def refused(scratch, run, outs, what, code=None):
    """run() must answer a negative code (`code` if given) and change no byte of the outputs, the scratch or a band."""
    if scratch is not None:
        scratch.poison('zero')
    for o in outs:
        o.reset()
    before = [o.g.view().clone() for o in outs]
    rc = run()
    torch.cuda.synchronize()
    assert rc < 0 and (code is None or rc == code), '%s: code %d' % (what, rc)
    assert_all_intact([scratch] + [o.g for o in outs])
    for b, o in zip(before, outs):
        assert torch.equal(b, o.g.view()), '%s: a refused call wrote %s' % (what, o.g.name)
    assert scratch is None or not scratch.view().any(), '%s: a refused call wrote its scratch' % what


# ========================================================================================================================
# gist_gemm_{nt,nn,tn}_f32: the fourteen cases of tests/test_gemm_plan_gpu.py
# ========================================================================================================================
def _gemm(L, form, a, b, bias, out_ptr, m, n, k, wp, wb):
    bp = bias.data_ptr() if bias is not None else None
    if form == 'nt':
        return L.gist_gemm_nt_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), bp, out_ptr, n, m, n, k, wp, wb, _st())
    fn = L.gist_gemm_nn_f32 if form == 'nn' else L.gist_gemm_tn_f32
    return fn(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out_ptr, n, m, n, k, wp, wb, _st())


def _gemm_buffers(form, m, n, k, a, b):
    """(an empty tensor has no address: a k = 0 call gets real buffers of which it may read nothing)"""
    if k:
        return a, b
    return ((torch.ones(4, m, device=DEV), torch.ones(4, n, device=DEV)) if form == 'tn' else
            (torch.ones(m, 4, device=DEV), torch.ones(n, 4, device=DEV)))


@pytest.mark.parametrize('mode,hooks,form,m,n,k,full,less', PLAN_CASES,
                         ids=['%s-%s-%dx%dx%d' % (c[0], c[2], c[3], c[4], c[5]) for c in PLAN_CASES])
def test_gemm_plan_cases(L, mode, hooks, form, m, n, k, full, less):
    from gist_amd import hip
    prev = hip.gemm_mode()
    try:
        hip.gemm_mode(mode)
        for name, v in hooks.items():
            hip.tuning(name, v)
        gen = torch.Generator(device=DEV).manual_seed(m + 3 * n + 7 * k)
        a, b = _operands(form, m, n, k, gen, 'normal')
        bias = torch.randn(n, device=DEV, generator=gen) * 1e-3 if form == 'nt' else None
        rows = torch.arange(0, m, max(1, m // 192), device=DEV)
        ref, den = _ref64(form, a, b, rows)
        if bias is not None:
            ref = ref + bias.double()
        a_buf, b_buf = _gemm_buffers(form, m, n, k, a, b)
        # the larger call of the 'keep' poison: more rows, columns and k, other magnitudes, planned for the same bytes
        m2, n2, k2 = m + 70, n + 33, k + 130
        a2, b2 = _operands(form, m2, n2, k2, gen, 'normal')
        a2, b2 = a2 * 300.0, b2 * 7.0
        out2 = torch.empty(m2, n2, device=DEV)
        out = Out(m, n, 'output of gist_gemm_%s_f32 %dx%dx%d' % (form, m, n, k))
        y1 = None
        for kind, cap, plan in gemm_capacities(L, form, m, n, k):
            what = 'gist_gemm_%s_f32 %s %dx%dx%d with %s = %d bytes' % (form, mode, m, n, k, kind, cap)
            print('%s: %r' % (what, plan))
            assert plan_fits(plan, cap), (what, plan)
            ws = Guarded(cap, DEV, name='workspace of ' + what) if cap else None
            wp = ws.ptr if ws else None
            got = under_poisons(ws, FLOAT_POISONS if ws else ('nan',),
                                lambda: _gemm(L, form, a_buf, b_buf, bias, out.ptr, m, n, k, wp, cap),
                                lambda: _gemm(L, form, a2, b2, None, out2.data_ptr(), m2, n2, k2, wp, cap), [out], what)
            y = got['nan'][0][rows].double()
            assert torch.isfinite(y).all(), what
            if plan['path'] == 'f32':       # tests/test_kernels_gpu.py: test_gemm_nt
                err = (y - ref).abs().max().item()
                assert err <= (2e-6 * np.sqrt(k) + 1e-6) * max(1.0, ref.abs().max().item()), (what, err)
                continue
            if y1 is None:                  # the split paths: against the fp32 kernel's own error on the same operands
                hip.gemm_mode('f32')
                o1 = torch.full((m, n), float('nan'), device=DEV)
                need1 = hip.gemm_plan(form, m, n, k)['workspace_bytes']
                w1 = torch.empty(max(need1, 16), dtype=torch.uint8, device=DEV)
                assert _gemm(L, form, a_buf, b_buf, bias, o1.data_ptr(), m, n, k, w1.data_ptr() if need1 else None, need1) == 0
                hip.gemm_mode(mode)
                y1 = o1[rows].double().cpu().numpy()
            ok, stats = GK.cmp_split(plan['path'], 'normal', y.cpu().numpy(), y1, ref.cpu().numpy(), den.cpu().numpy())
            assert ok, (what, stats)
    finally:
        for name in hooks:
            hip.tuning(name, 0)
        hip.gemm_mode(prev)


# ========================================================================================================================
# gist_gemm_slabs_f32: the deferred-slab forms, slab bytes from both size queries
# ========================================================================================================================
def _one_layer_plan(n_in, n_out, n_max):
    from gist_amd import _lib
    P = _lib.StepPlan()
    P.n_layers, P.n_max, P.fuse = 1, n_max, 1
    P.layer[0].n_in, P.layer[0].n_out = n_in, n_out
    P.layer[0].ldz, P.layer[0].ldy = 2 * n_in, n_out
    return P


SLAB_CASES = [('nt', 300, 41, 2046), ('nn', 300, 41, 2046), ('tn', 41, 1024, 2046)]


def _slab_needs(L, form, m, n, k):
    """{which query: bytes}: gist_gemm_workspace_bytes, and what the fused step reserves for the same projection (the class
    layer's logits for NT, a weight gradient for TN)."""
    needs = {'gist_gemm_workspace_bytes': int(L.gist_gemm_workspace_bytes(m, n, k))}
    if form == 'nt':
        needs['gist_step_fused_slab_bytes'] = int(L.gist_step_fused_slab_bytes(ctypes.byref(_one_layer_plan(k // 2, n, m)), 1))
    elif form == 'tn':
        needs['gist_step_fused_slab_bytes'] = int(L.gist_step_fused_slab_bytes(ctypes.byref(_one_layer_plan(n // 2, m, k)), 0))
    return needs


def _slabs(L, form, a, b, bias, c_ptr, m, n, k, sp, sb, ns):
    return L.gist_gemm_slabs_f32({'nt': 0, 'nn': 1, 'tn': 2}[form], a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                 bias.data_ptr() if bias is not None else None, c_ptr, n, m, n, k, sp, sb,
                                 ctypes.byref(ns), _st())


@pytest.mark.parametrize('form,m,n,k', SLAB_CASES, ids=['%s-%dx%dx%d' % c for c in SLAB_CASES])
def test_gemm_slabs(L, form, m, n, k):
    from gist_amd import hip
    prev = hip.gemm_mode()
    hip.gemm_mode('f32')
    try:
        gen = torch.Generator(device=DEV).manual_seed(m + n + k)
        a, b = _operands(form, m, n, k, gen, 'normal')
        bias = torch.randn(n, device=DEV, generator=gen) if form == 'nt' else None
        ref, den = GK.ref64(form, a.cpu().numpy(), b.cpu().numpy(), None if bias is None else bias.cpu().numpy())
        m2, k2 = m + 70, k + 130
        a2, b2 = _operands(form, m2, n, k2, gen, 'normal')
        a2 = a2 * 300.0
        c2 = torch.empty(m2, n, device=DEV)
        c = Out(m, n, 'c of gist_gemm_slabs_f32')
        needs = _slab_needs(L, form, m, n, k)
        assert all(v > 0 for v in needs.values()), needs
        seen = set()
        for query, need in needs.items():
            for kind, cap in capacities(need):
                if cap in seen:
                    continue
                seen.add(cap)
                what = 'gist_gemm_slabs_f32 %s %dx%dx%d with %s of %s = %d bytes' % (form, m, n, k, kind, query, cap)
                slabs = Guarded(cap, DEV, name='slabs of ' + what) if cap else None
                sp = slabs.ptr if slabs else None
                ns, ns2, counts = ctypes.c_int32(-1), ctypes.c_int32(-1), []

                def run():
                    rc = _slabs(L, form, a, b, bias, c.ptr, m, n, k, sp, cap, ns)
                    counts.append(ns.value)
                    return rc

                got = under_poisons(slabs, FLOAT_POISONS if slabs else ('nan',), run,
                                    lambda: _slabs(L, form, a2, b2, None, c2.data_ptr(), m2, n, k2, sp, cap, ns2), [c], what,
                                    extra=lambda: [floats_of(slabs, ns.value * m * n)] if ns.value > 1 else [])
                assert len(set(counts)) == 1 and counts[0] >= 1, counts
                n_s = counts[0]
                print('%s: %d slabs' % (what, n_s))
                assert n_s == 1 or n_s * m * n * 4 <= cap, (what, n_s)
                if n_s > 1:      # c is not written; the consumer's sum in slab order, then the bias
                    assert torch.isnan(got['nan'][0]).all(), what + ': c written although the slabs are deferred'
                    y = GK.sum_slabs(got['nan'][1], n_s, m, n, bias)
                else:
                    y = got['nan'][0]
                r = GK.cmp_f32(y.cpu().numpy(), ref, den, k, n_s)
                assert r <= 1.0, (what, r)
    finally:
        hip.gemm_mode(prev)


# ========================================================================================================================
# gist_gemm_nn_dropout_f32 / _colsum_f32: the narrow-k one-kernel form and the two-kernel form
# ========================================================================================================================
NN_DROP_CASES = [('narrow', 300, 1028, 41, 1000), ('narrow', 17, 260, 64, 1000), ('two-kernel', 17, 260, 64, 1001),
                 ('two-kernel', 300, 41, 2046, 1000), ('two-kernel', 130, 1028, 65, 77)]


@pytest.mark.parametrize('colsum', [False, True], ids=['plain', 'colsum'])
@pytest.mark.parametrize('kind_,m,n,k,off', NN_DROP_CASES, ids=['%s-%dx%dx%d' % c[:4] for c in NN_DROP_CASES])
def test_gemm_nn_dropout(L, kind_, m, n, k, off, colsum):
    from gist_amd import hip
    prev = hip.gemm_mode()
    hip.gemm_mode('f32')
    try:
        rs = np.random.RandomState(m + n + k)
        g = (rs.randn(m, k) * 10.0 ** rs.randint(-2, 3, size=(m, 1))).astype(F32)
        w = rs.randn(k, n).astype(F32)
        gt, wt = torch.from_numpy(g).to(DEV), torch.from_numpy(w).to(DEV)
        g2, w2 = torch.randn(m + 70, k + 130, device=DEV) * 300.0, torch.randn(k + 130, n, device=DEV)
        z2 = torch.empty(m + 70, n, device=DEV)
        mask = _dropout_mask_ref(m, n, R.P_DROP, R.SEED, off)
        z = Out(m, n, 'z of gist_gemm_nn_dropout_f32')
        chunks = int(L.gist_row_chunks16(m))
        part = Out(chunks, k, 'g_col_partials (exactly gist_row_chunks16(m) * k floats)') if colsum else None
        outs = [z] + ([part] if colsum else [])
        need = int(L.gist_gemm_workspace_bytes(m, n, k))
        assert (need > 0) == (k == 2046), need
        assert R.nn_drop_inst(m, n, k, n, n, True, True, off)[1] == kind_      # (the mirror of the host dispatch)

        def call(G, W, Z_ptr, mm, kk, wp, cap, offset, part_ptr):
            if colsum:
                return L.gist_gemm_nn_dropout_colsum_f32(G.data_ptr(), G.stride(0), W.data_ptr(), W.stride(0), Z_ptr, n, mm, n, kk,
                                                         R.P_DROP, R.SEED, offset, wp, cap, part_ptr, _st())
            return L.gist_gemm_nn_dropout_f32(G.data_ptr(), G.stride(0), W.data_ptr(), W.stride(0), Z_ptr, n, mm, n, kk,
                                              R.P_DROP, R.SEED, offset, wp, cap, _st())

        part2 = torch.empty(int(L.gist_row_chunks16(m + 70)) * (k + 130), device=DEV)
        for kind, cap in capacities(need):
            what = 'gist_gemm_nn_dropout%s_f32 %s %dx%dx%d with %s = %d bytes' % ('_colsum' if colsum else '', kind_, m, n, k, kind, cap)
            ws = Guarded(cap, DEV, name='workspace of ' + what) if cap else None
            wp = ws.ptr if ws else None
            before = L.gist_launch_count()
            got = under_poisons(ws, FLOAT_POISONS if ws else ('nan',),
                                lambda: call(gt, wt, z.ptr, m, k, wp, cap, off, part.ptr if colsum else None),
                                lambda: call(g2, w2, z2.data_ptr(), m + 70, k + 130, wp, cap, 5, part2.data_ptr()), outs, what)
            if ws is None:
                issued = L.gist_launch_count() - before
                assert (issued == 1) if kind_ == 'narrow' else (issued >= 2), (what, issued)
            r, zeros_ok = R.cmp_nn_drop(g, w, got['nan'][0].cpu().numpy(), mask, R.P_DROP)
            assert r <= 1.0 and zeros_ok, (what, r, zeros_ok)
            if colsum:      # the chunk sums add up to g's column sums (tests/test_rowops_kernels_gpu.py: cmp_colsum)
                p = got['nan'][1].cpu().numpy()
                assert np.isfinite(p).all()
                assert R.cmp_colsum(g, R.chunked_sum_f32(p), chunks) <= 1.0, what
    finally:
        hip.gemm_mode(prev)


# ========================================================================================================================
# gist_gemm_nn_tn_dual_f32
# ========================================================================================================================
DUAL_CASES = [(300, 192, 96), (1140, 512, 256)]


@pytest.mark.parametrize('m,n,k', DUAL_CASES, ids=['%dx%dx%d' % c for c in DUAL_CASES])
def test_gemm_nn_tn_dual(L, m, n, k):
    from gist_amd import hip
    prev = hip.gemm_mode()
    hip.gemm_mode('f32')
    try:
        rng = np.random.default_rng(m + n)
        dy, w, zz = (rng.standard_normal(s, dtype=F32) for s in ((m, k), (k, n), (m, n)))
        dyt, wt, zt = (torch.from_numpy(x).to(DEV) for x in (dy, w, zz))
        dy2, z2 = torch.randn(m + 64, k, device=DEV) * 300.0, torch.randn(m + 64, n, device=DEV)
        dz2, dw2 = torch.empty(m + 64, n, device=DEV), torch.empty(k, n, device=DEV)
        dz, dw = Out(m, n, 'dz of gist_gemm_nn_tn_dual_f32'), Out(k, n, 'dw of gist_gemm_nn_tn_dual_f32')
        assert hip.gemm_dual_takes(dyt, wt, zt, dz.t) and hip.gemm_dual_takes(dy2, wt, z2, dz2)
        need = int(L.gist_gemm_workspace_bytes(k, n, m))
        refs = (GK.ref64('nn', dy, w), GK.ref64('tn', dy, zz))

        def call(DY, Z, DZ_ptr, DW_ptr, mm, sp, cap, ns):
            return L.gist_gemm_nn_tn_dual_f32(DY.data_ptr(), k, wt.data_ptr(), n, DZ_ptr, n, Z.data_ptr(), n, DW_ptr, n, mm, n, k,
                                              sp, cap, ctypes.byref(ns), _st())

        for kind, cap in capacities(need):
            what = 'gist_gemm_nn_tn_dual_f32 %dx%dx%d with %s = %d bytes' % (m, n, k, kind, cap)
            slabs = Guarded(cap, DEV, name='slabs of ' + what) if cap else None
            sp = slabs.ptr if slabs else None
            ns, ns2 = ctypes.c_int32(-1), ctypes.c_int32(-1)
            got = under_poisons(slabs, FLOAT_POISONS if slabs else ('nan',),
                                lambda: call(dyt, zt, dz.ptr, dw.ptr, m, sp, cap, ns),
                                lambda: call(dy2, z2, dz2.data_ptr(), dw2.data_ptr(), m + 64, sp, cap, ns2), [dz, dw], what,
                                extra=lambda: [floats_of(slabs, ns.value * k * n)] if ns.value > 1 else [])
            n_s = ns.value
            print('%s: %d slabs' % (what, n_s))
            assert n_s >= 1 and (n_s == 1 or n_s * k * n * 4 <= cap), (what, n_s)
            dwr = GK.sum_slabs(got['nan'][2], n_s, k, n, None) if n_s > 1 else got['nan'][1]
            assert GK.cmp_f32(got['nan'][0].cpu().numpy(), refs[0][0], refs[0][1], k, 1) <= 1.0, what
            assert GK.cmp_f32(dwr.cpu().numpy(), refs[1][0], refs[1][1], m, n_s) <= 1.0, what
    finally:
        hip.gemm_mode(prev)


# ========================================================================================================================
# column sums: partials of exactly gist_colsum_partials(n) * d floats
# ========================================================================================================================
@pytest.mark.parametrize('d', [1, 41, 602])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 257, 2046])
def test_colsum(L, n, d):
    g = R.colsum_inputs(n, d)
    gt = torch.from_numpy(g).to(DEV)
    g2 = torch.randn(2 * n + 70, d, device=DEV) * 1e6
    chunks = int(L.gist_colsum_partials(n))
    assert chunks == (n + 63) // 64
    out = Out(1, d, 'out of gist_colsum_f32')
    part = Guarded(chunks * d * 4, DEV, name='partials of gist_colsum_f32 n=%d d=%d (gist_colsum_partials(n) * d floats)' % (n, d))
    scratch2 = torch.empty(int(L.gist_colsum_partials(2 * n + 70)) * d, device=DEV)
    out2 = torch.empty(d, device=DEV)

    def prime():
        # a larger batch's partial sums: computed beside the guarded buffer, then its first chunks copied in -- the call
        # itself may not be given more than the interior
        rc = L.gist_colsum_f32(g2.data_ptr(), d, 2 * n + 70, d, scratch2.data_ptr(), out2.data_ptr(), _st())
        spill(part, scratch2)
        return rc

    got = under_poisons(part, FLOAT_POISONS, lambda: L.gist_colsum_f32(gt.data_ptr(), d, n, d, part.ptr, out.ptr, _st()),
                        prime, [out], 'gist_colsum_f32 n=%d d=%d' % (n, d))
    assert R.cmp_colsum(g, got['nan'][0].cpu().numpy()[0], chunks) <= 1.0
    # gist_colsum_chunks_f32 reads exactly chunks * d floats (here: n rows as n chunks) and writes d
    rows = Guarded(n * d * 4, DEV, name='partials read by gist_colsum_chunks_f32')
    rows.view(torch.float32).copy_(gt.reshape(-1))
    out.reset()
    assert L.gist_colsum_chunks_f32(rows.ptr, n, d, out.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert_all_intact([rows, out.g])
    assert torch.equal(bits(rows.view(torch.float32)), bits(gt.reshape(-1)))
    assert R.cmp_colsum(g, out.t.cpu().numpy()[0], n) <= 1.0


# ========================================================================================================================
# gist_ln_affine_bwd_f32: exactly gist_ln_affine_bwd_workspace_floats; one float short must refuse
# ========================================================================================================================
LNA_CASES = [(37, 17, 1, 1), (256, 35, 1, 0), (1028, 16, 0, 1), (602, 1, 1, 1)]


@pytest.mark.parametrize('d,n,relu,lb', LNA_CASES, ids=['d%d-n%d-relu%d-lb%d' % c for c in LNA_CASES])
def test_ln_affine_bwd(L, d, n, relu, lb):
    inputs = LA.bwd_inputs((d, n, True, relu, lb))
    g, y, rstd, gamma, beta = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in inputs)
    n2 = n + 40
    g2, y2 = torch.randn(n2, d, device=DEV) * 1e4, torch.randn(n2, d, device=DEV)
    rstd2, dx2, sums2 = torch.rand(n2, device=DEV) + 0.5, torch.empty(n2, d, device=DEV), torch.empty(3, d, device=DEV)
    need = int(L.gist_ln_affine_bwd_workspace_floats(n, d))
    assert need == 3 * ((n + 15) // 16) * d
    big = torch.empty(int(L.gist_ln_affine_bwd_workspace_floats(n2, d)), device=DEV)
    outs = [Out(n, d, 'dx'), Out(1, d, 'dgamma'), Out(1, d, 'dbeta')] + ([Out(1, d, 'dlin_bias')] if lb else [])

    def call(wp, floats):
        return L.gist_ln_affine_bwd_f32(g.data_ptr(), d, y.data_ptr(), d, rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), relu,
                                        outs[0].ptr, d, outs[1].ptr, outs[2].ptr, outs[3].ptr if lb else None, n, d, wp, floats, _st())

    def prime():
        rc = L.gist_ln_affine_bwd_f32(g2.data_ptr(), d, y2.data_ptr(), d, rstd2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), relu,
                                      dx2.data_ptr(), d, sums2[0].data_ptr(), sums2[1].data_ptr(), sums2[2].data_ptr(), n2, d,
                                      big.data_ptr(), big.numel(), _st())
        spill(ws, big)
        return rc

    for floats in (need, 2 * need + 1):
        ws = Guarded(floats * 4, DEV, name='workspace of gist_ln_affine_bwd_f32 (%d floats, %d asked)' % (floats, need))
        got = under_poisons(ws, FLOAT_POISONS, lambda: call(ws.ptr, floats), prime, outs, 'gist_ln_affine_bwd_f32 d=%d n=%d' % (d, n))
        res = [t.cpu().numpy() for t in got['nan']]
        r = LA.cmp_affine_bwd(inputs, relu, res[0], res[1][0], res[2][0], res[3][0] if lb else None)
        assert max(r) <= 1.0, r
    for floats in (need - 1, need // 2):
        ws = Guarded(floats * 4, DEV, name='short workspace of gist_ln_affine_bwd_f32') if floats else None
        refused(ws, lambda: call(ws.ptr if ws else None, floats), outs, 'gist_ln_affine_bwd_f32 with %d of %d floats' % (floats, need))
    refused(None, lambda: call(None, 0), outs, 'gist_ln_affine_bwd_f32 without a workspace')


# ========================================================================================================================
# gist_ln_all_{fwd,bwd}_f32: exactly gist_ln_all_partials(n) floats
# ========================================================================================================================
def ln_all_sizes(L):
    """1, 7, 4096, 43328, and the first size at which the grid is at its workgroup cap (gist_ln_all_partials stops
    growing: found by query)."""
    top = int(L.gist_ln_all_partials(1 << 30))
    lo, hi = 1, 1 << 30
    while lo < hi:
        mid = (lo + hi) // 2
        if int(L.gist_ln_all_partials(mid)) >= top:
            hi = mid
        else:
            lo = mid + 1
    return [1, 7, 4096, 43328, lo, lo + 4099]


@pytest.mark.parametrize('which', range(6))
def test_ln_all(L, which):
    sizes = ln_all_sizes(L)
    n = sizes[which]
    if which >= 4:
        assert int(L.gist_ln_all_partials(n)) == int(L.gist_ln_all_partials(1 << 30)) == 4096, 'not at the workgroup cap'
        assert int(L.gist_ln_all_partials(sizes[4] - 1)) < 4096
    x = LN.make_input('normal', n)
    xt = torch.from_numpy(x).to(DEV)
    x2 = torch.randn(2 * n + 5000, device=DEV) * 1e5 + 3e4
    y2, s2 = torch.empty_like(x2), torch.empty(2, device=DEV)
    need = int(L.gist_ln_all_partials(n))
    big = torch.empty(int(L.gist_ln_all_partials(x2.numel())), device=DEV)
    part = Guarded(need * 4, DEV, name='partials of gist_ln_all_*_f32 n=%d (%d floats)' % (n, need))
    yhat, stats = Out(1, n, 'yhat'), Out(1, 2, 'stats')

    def prime_fwd():
        rc = L.gist_ln_all_fwd_f32(x2.data_ptr(), y2.data_ptr(), s2.data_ptr(), x2.numel(), LN.LN_EPS, big.data_ptr(), _st())
        spill(part, big)
        return rc

    got = under_poisons(part, FLOAT_POISONS,
                        lambda: L.gist_ln_all_fwd_f32(xt.data_ptr(), yhat.ptr, stats.ptr, n, LN.LN_EPS, part.ptr, _st()),
                        prime_fwd, [yhat, stats], 'gist_ln_all_fwd_f32 n=%d' % n)
    y = got['nan'][0][0].cpu().numpy()
    mean32, rstd32 = (float(v) for v in got['nan'][1][0].cpu().numpy())
    y64, mean, s, sigma = LN.forward_ref(x)
    assert LN._ratio('scratch fwd', np.abs(y - y64), LN.forward_bound(y64, mean, s)) < 1
    assert LN._ratio('scratch stats', abs(mean32 - mean), LN.EPS32 * (0.5 * abs(mean) + 10 * sigma) + 1e-300) < 1
    assert LN._ratio('scratch stats', abs(rstd32 - 1 / s), 6.25 * LN.EPS32 / s) < 1
    rs = np.random.RandomState(n % 997 + 5)
    g = (rs.randn(n) * np.where(rs.rand(n) < 0.1, 50.0, 1.0)).astype(F32)
    gt, yt, st_ = torch.from_numpy(g).to(DEV), got['nan'][0][0].clone(), got['nan'][1][0].clone()
    dx, dx2 = Out(1, n, 'dx'), torch.empty_like(x2)

    def prime_bwd():
        rc = L.gist_ln_all_bwd_f32(x2.data_ptr(), y2.data_ptr(), s2.data_ptr(), dx2.data_ptr(), x2.numel(), big.data_ptr(), _st())
        spill(part, big)
        return rc

    got = under_poisons(part, FLOAT_POISONS,
                        lambda: L.gist_ln_all_bwd_f32(gt.data_ptr(), yt.data_ptr(), st_.data_ptr(), dx.ptr, n, part.ptr, _st()),
                        prime_bwd, [dx], 'gist_ln_all_bwd_f32 n=%d' % n)
    dx64, b_bound, _ = LN.backward_ref(g, y, rstd32)
    assert LN._ratio('scratch bwd', np.abs(got['nan'][0][0].cpu().numpy() - dx64), b_bound + 1e-300) < 1


# ========================================================================================================================
# gist_standard_scaler_f32: exactly gist_standard_scaler_workspace_bytes, with and without fit rows
# ========================================================================================================================
@pytest.mark.parametrize('fit', ['rows', 'all'])
@pytest.mark.parametrize('d', [1, 50, 602])
def test_standard_scaler(L, d, fit):
    from oracle import gist_oracle as O
    n = 700
    rs = np.random.RandomState(n + d)
    x = (rs.randn(n, d) * rs.uniform(0.01, 30, d) + rs.uniform(-50, 50, d)).astype(F32)
    x[:, d // 2] = -3.5
    rows = np.sort(rs.choice(n, 300, replace=False)) if fit == 'rows' else np.arange(n)
    mask = np.zeros(n, bool)
    mask[rows] = True
    want, mean, var = O.standard_scaler(x, mask)
    xt = torch.from_numpy(x).to(DEV)
    fr = torch.from_numpy(rows.astype(np.int32)).to(DEV) if fit == 'rows' else None
    n_fit = len(rows)
    need = int(L.gist_standard_scaler_workspace_bytes(n_fit, d))
    assert need > 0
    X, M, V = Out(n, d, 'x (in place)'), Out(1, d, 'mean', torch.float64), Out(1, d, 'var', torch.float64)

    class InPlace(object):      # x is input and output: "reset" restores the input
        g, t = X.g, X.t

        def reset(self):
            X.t.copy_(xt)

    outs = [InPlace(), M, V]

    def call(wp, nbytes):
        return L.gist_standard_scaler_f32(X.ptr, d, n, d, fr.data_ptr() if fr is not None else None, n_fit, M.ptr, V.ptr, wp, nbytes, _st())

    big_x = torch.randn(2 * n, d, device=DEV) * 1e5
    big_ws = torch.empty(int(L.gist_standard_scaler_workspace_bytes(2 * n, d)), dtype=torch.uint8, device=DEV)
    mv = torch.empty(2, d, dtype=torch.float64, device=DEV)

    def prime():
        rc = L.gist_standard_scaler_f32(big_x.data_ptr(), d, 2 * n, d, None, 2 * n, mv[0].data_ptr(), mv[1].data_ptr(),
                                        big_ws.data_ptr(), big_ws.numel(), _st())
        spill(ws, big_ws)
        return rc

    for nbytes in (need, 2 * need + 4):
        ws = Guarded(nbytes, DEV, name='workspace of gist_standard_scaler_f32 (%d bytes, %d asked)' % (nbytes, need))
        got = under_poisons(ws, FLOAT_POISONS, lambda: call(ws.ptr, nbytes), prime, outs, 'gist_standard_scaler_f32 d=%d %s' % (d, fit))
        xs, m_, v_ = (t.cpu().numpy() for t in got['nan'])
        assert np.allclose(m_[0], mean, rtol=1e-12, atol=1e-12) and np.allclose(v_[0], var, rtol=1e-9, atol=1e-12)
        assert np.abs(xs - want).max() <= 1e-6 * max(1.0, np.abs(want).max())      # tests/test_kernels_gpu.py
        assert np.array_equal(xs[:, d // 2], want[:, d // 2])
    for nbytes in (need - 1, need // 2):
        ws = Guarded(nbytes, DEV, name='short workspace of gist_standard_scaler_f32')
        refused(ws, lambda: call(ws.ptr, nbytes), outs, 'gist_standard_scaler_f32 with %d of %d bytes' % (nbytes, need))
    refused(None, lambda: call(None, 0), outs, 'gist_standard_scaler_f32 without a workspace')


# ========================================================================================================================
# gist_gat_attn_grad_f32: exactly gist_gat_attn_grad_workspace_floats
# ========================================================================================================================
@pytest.mark.parametrize('heads', [1, 4])
@pytest.mark.parametrize('n,f', [(1, 37), (257, 64), (600, 37)])
def test_gat_attn_grad(L, n, f, heads):
    from tests.test_gat_kernels_gpu import _close, ref_attn_grad
    gen = torch.Generator(device=DEV).manual_seed(n + f + heads)
    z = torch.randn(n, heads * f, device=DEV, generator=gen)
    ds_src = torch.randn(n, heads, device=DEV, generator=gen)
    ds_dst = torch.randn(n, heads, device=DEV, generator=gen)
    n2 = 2 * n + 300
    z2, s2, da2 = torch.randn(n2, heads * f, device=DEV) * 1e4, torch.randn(n2, heads, device=DEV), torch.empty(heads, 2 * f, device=DEV)
    need = int(L.gist_gat_attn_grad_workspace_floats(n, heads, f))
    big = torch.empty(int(L.gist_gat_attn_grad_workspace_floats(n2, heads, f)), device=DEV)
    da = Out(heads, 2 * f, 'dA of gist_gat_attn_grad_f32')

    def call(wp, floats):
        return L.gist_gat_attn_grad_f32(z.data_ptr(), heads * f, ds_src.data_ptr(), ds_dst.data_ptr(), n, heads, f, wp, floats,
                                        da.ptr, _st())

    def prime():
        rc = L.gist_gat_attn_grad_f32(z2.data_ptr(), heads * f, s2.data_ptr(), s2.data_ptr(), n2, heads, f, big.data_ptr(),
                                      big.numel(), da2.data_ptr(), _st())
        spill(ws, big)
        return rc

    for floats in (need, 2 * need + 1):
        ws = Guarded(floats * 4, DEV, name='partials of gist_gat_attn_grad_f32 (%d floats, %d asked)' % (floats, need))
        got = under_poisons(ws, FLOAT_POISONS, lambda: call(ws.ptr, floats), prime, [da], 'gist_gat_attn_grad_f32 n=%d' % n)
        _close(got['nan'][0], ref_attn_grad(z, ds_src, ds_dst, heads, f), 'dA', ' (n=%d, %d floats of scratch)' % (n, floats))
    for floats in (need - 1, need // 2):
        ws = Guarded(floats * 4, DEV, name='short partials of gist_gat_attn_grad_f32')
        refused(ws, lambda: call(ws.ptr, floats), [da], 'gist_gat_attn_grad_f32 with %d of %d floats' % (floats, need), GIST_ENOSPACE)
    refused(None, lambda: call(None, 0), [da], 'gist_gat_attn_grad_f32 without a workspace', GIST_ENOSPACE)


# ========================================================================================================================
# gist_spmm_blocks_prepare + the prepared aggregation that reads it: exactly gist_spmm_blocks_bytes per orientation
# ========================================================================================================================
def _csr(src, dst, n):
    from oracle import gist_oracle as O
    rowptr, col = O.csr_from_edges(src, dst, n)
    return rowptr, col


@pytest.mark.parametrize('pairs', [False, True], ids=['no pairs', 'pairs'])
@pytest.mark.parametrize('d', [1536, 602])
@pytest.mark.parametrize('orientation', ['forward', 'reversed'])
def test_spmm_blocks_prepare(L, d, pairs, orientation):
    """Index-holding scratch: zeros, or the structure of a batch with more blocks -- never 0xFF.  Both orientations a
    step prepares: the in-edge CSR (y = norm . A x) and the reversed one in the backward form (y += A^T (norm . x))."""
    from oracle import gist_oracle as O
    rs = np.random.RandomState(7 + d)
    n, cuts, src, dst = _sibling_graph(rs, n_parts=6, part=102, siblings=((1, 4), (2, 3)) if pairs else (), cross_per_row=45)
    nb = len(cuts) - 1
    rowptr, col = _csr(src, dst, n)
    norm = O.in_degree_norm(rowptr)
    x = rs.randint(-4, 5, (n, d)).astype(F32) if d % 4 == 0 else rs.randn(n, d).astype(F32)
    back = orientation == 'reversed'
    y0 = rs.randint(-4, 5, (n, d)).astype(F32)      # what the backward form accumulates onto
    if back:
        rowptr, col = O.transpose_csr(rowptr, col)
        ref = y0.copy()
        O.spmm_sum(rowptr, col, x, src_scale=norm, out=ref, accumulate=True)
        ref = ref.astype(np.float64)
    else:
        ref = O.spmm_sum(rowptr, col, x, out_scale=norm).astype(np.float64)
    i32 = lambda a_: torch.from_numpy(np.asarray(a_).astype(np.int32)).to(DEV)
    rp, cl, rb, nt = i32(rowptr), i32(col), i32(cuts), torch.from_numpy(norm.astype(F32)).to(DEV)
    # the larger earlier batch: more blocks, sibling parts among them
    n2, cuts2, src2, dst2 = _sibling_graph(np.random.RandomState(3), n_parts=11, part=110, siblings=((0, 5), (2, 9)), cross_per_row=45)
    rowptr2, col2 = _csr(src2, dst2, n2)
    rp2, cl2, rb2 = i32(rowptr2), i32(col2), i32(cuts2)
    big = torch.empty(int(L.gist_spmm_blocks_bytes(len(cuts2) - 1)), dtype=torch.uint8, device=DEV)
    xt = torch.zeros(max(n, n2), d, device=DEV)[:n]      # (rows a stale index of the larger structure could still name)
    xt.copy_(torch.from_numpy(x))
    need = int(L.gist_spmm_blocks_bytes(nb))
    y = Out(n, d, 'y of gist_spmm_csr_prepared_f32')
    if back:      # (accumulated onto: every call starts from y0, not from NaN)
        y0t = torch.from_numpy(y0).to(DEV)
        y.reset = lambda: y.t.copy_(y0t)

    def run():
        rc = L.gist_spmm_blocks_prepare(rp.data_ptr(), cl.data_ptr(), n, rb.data_ptr(), nb, prep.ptr, prep.nbytes, _st())
        if rc:
            return rc
        return L.gist_spmm_csr_prepared_f32(rp.data_ptr(), cl.data_ptr(), xt.data_ptr(), d, y.ptr, d, n, d,
                                            None if back else nt.data_ptr(), nt.data_ptr() if back else None, int(back),
                                            rb.data_ptr(), nb, prep.ptr, _st())

    def prime():
        rc = L.gist_spmm_blocks_prepare(rp2.data_ptr(), cl2.data_ptr(), n2, rb2.data_ptr(), len(cuts2) - 1, big.data_ptr(),
                                        big.numel(), _st())
        spill(prep, big)
        return rc

    for nbytes in (need, 2 * need + 16):
        prep = Guarded(nbytes, DEV, name='prepared block structure (%d bytes, gist_spmm_blocks_bytes(%d) = %d)' % (nbytes, nb, need))
        got = under_poisons(prep, INDEX_POISONS, run, prime, [y], 'gist_spmm_blocks_prepare + prepared aggregation d=%d' % d)
        out = got['zero'][0].cpu().numpy().astype(np.float64)
        assert np.isfinite(out).all()
        close(out, ref)      # tests/test_kernels_gpu.py: TOL = 1e-4 of the largest result
    for nbytes in (need - 16, need // 2 // 16 * 16):
        prep = Guarded(nbytes, DEV, name='short prepared block structure')
        refused(prep, lambda: L.gist_spmm_blocks_prepare(rp.data_ptr(), cl.data_ptr(), n, rb.data_ptr(), nb, prep.ptr, prep.nbytes, _st()),
                [y], 'gist_spmm_blocks_prepare with %d of %d bytes' % (nbytes, need))


# ========================================================================================================================
# gist_extract_parts_batch / _desc_batch: exactly gist_extract_parts_scratch_bytes(n_max), zeroed once, bands only
# ========================================================================================================================
class _At(object):
    """what tests/test_extract_kernels_gpu.PartsLaunch asks of its scratch: an address"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def test_extract_parts_scratch(L):
    """n = 2100, 17, 1, 600, 2100 back to back on ONE scratch of exactly the bytes the query reports for the largest:
    zeroed once as the contract says, guarded, never poisoned; every batch equals its host reference."""
    from gist_amd import hip
    from tests import test_extract_kernels_gpu as X
    n_max = X.ref_struct('big', 0).n + 5
    need = int(L.gist_extract_parts_scratch_bytes(n_max))
    scratch = Guarded(need, DEV, name='scratch of gist_extract_parts_desc_batch (gist_extract_parts_scratch_bytes(%d) = %d)' % (n_max, need))
    scratch.poison('zero')
    runs = [X.PartsLaunch(epoch, j, 24, 'int', X.width_geom(24, k), _At(scratch.ptr), n_max=n_max,
                          drop_offset=X.OFFSETS[k % 3] if k % 2 else None, with_ah=False)
            for k, (epoch, j) in enumerate(X.SEQUENCE)]
    for r in runs:
        r.launch(hip)
        torch.cuda.synchronize()
        scratch.assert_intact()
    words = scratch.view(torch.int64) if need % 8 == 0 else None
    assert words is None or [int(v) for v in words[1:4].cpu()] == [0, 0, 0], 'error word or tickets set'
    for r in runs:
        r.check()
    # the argument-list form on the same scratch
    r = X.PartsLaunch('small17', 0, 24, 'int', X.width_geom(24, 0), _At(scratch.ptr), n_max=n_max, with_ah=False)
    x = r.desc
    rc = L.gist_extract_parts_batch(x.g_rowptr, x.g_col, x.g_t_rowptr, x.g_t_col, x.ids, x.n, x.n_max, x.node_part, x.part_slot,
                                    x.batch, x.rowptr, x.col, x.t_rowptr, x.t_col, x.col_capacity, x.norm, x.feat, x.ld_feat,
                                    x.n_feat, x.z0, x.ldz0, x.labels_all, x.labels, None, 0, 0.0, 0, 0, 0, scratch.ptr, _st())
    torch.cuda.synchronize()
    assert rc == 0, L.gist_last_error()
    scratch.assert_intact()
    r.check()
