"""GPU: every launching export of include/gist_hip.h keeps the promise INTEGRATION.md makes of all of them --
"Asynchronous on the given stream; no allocation, no host sync inside" -- when the stream is NOT the null stream.

One harness (protocol), one table of cases (CASES, STEP_CASES, MODULE_CASES).  A case gives make(variant) -> its inputs
(built on the CPU) and call(inputs, context) -> its outputs.  The variants A and B have the same shapes, strides, dtypes
and sizes, so both take the same kernel path; float data are other random values, index data (ids, part tables, index
pools, fit rows, graphs) are other VALID index sets of the same length -- B's graph is A's transposed: as many rows, as
many edges.  No index buffer is ever filled with NaN bytes or 0xFF (the rule of tests/test_scratch_bounds_kernels_gpu.py):
a launch that runs too early reads A, computes a wrong answer and cannot leave its buffers.

  1. warm-up: the call with A on the default stream, twice, each followed by a synchronise (the first loads the code
     objects and grows hip.workspace, the second is the one whose host time is measured; every input, scratch and output
     now holds what A left);
  2. on a torch.cuda.Stream() S that was first probed to run beside the null stream (side_stream): a delay kernel, an event
     `delay_done`, B copied into the live input buffers (in-place state and the outputs' initial contents included), the
     call inside `with torch.cuda.stream(S)`, returned_early = not delay_done.query() read as soon as the call returns,
     the outputs cloned on S, S.synchronize();
  3. the expected result: B restored and the same call on the default stream;
  and then
  (a) every output of 2 equals 3 bit for bit;
  (b) every output of 3 differs from 1 (the case can tell A from B);
  (c) returned_early: the host was back while S was still held by the delay, so the call did not wait for the device and
      every launch was issued before its inputs existed -- one that is not ordered on S saw A.

The delay is torch.cuda._sleep, its cycle count calibrated once with a pair of events: the larger of 20 ms and ten times
the host time of the case's warm-up call; had it ended when the call returned, the case is repeated with twice the delay,
three times at the most, and then FAILS as inconclusive (never skipped).  No tolerance: bitwise equality with the same
call on the default stream.

test_wrong_stream_is_caught is the positive control: gist_colsum_f32 through the same protocol, but handed stream 0
while B is made ready on S -- its result must DIFFER from step 3's, which shows that on this runtime and queue
configuration a launch on the wrong stream really overtakes S and is seen.  It reads valid A data and provokes nothing.

The steps (gist_sage_step, gist_gat_step / _phase, gist_graphsage_step / _phase, gist_baseline_gcn_step) run through
their engines on datasets.toy cut into parts of 64 and 65 rows (four batches of 129), with dropout where the family has it
and the next batch's extraction riding on the optimiser launch (prefetch); A and B are other batches of the same length
and other parameter arenas and Adam moments, restored on S behind the delay; the batch is described before the delay
starts.  Compared: loss, logits, gradients, parameters, both moments and the batch buffers' rowptr / col; the gist_timer
fills as many slots on S as on the default stream, each elapsed time finite and >= 0.

The module path (MODULE_CASES): one training step of each family's module loop (modules.py on the custom autograd ops of
gist_amd/ops.py and autograd.py, gist_amd.nn.CrossEntropyLoss, loss.backward() where autograd puts it, gist_amd.optim.Adam)
on S.  The wrappers with a readback in their own source (MODULE_READBACKS) cut the cluster out of the graph: that happens
before any delay starts, as the batch of a step is taken from its iterator before it; the training step itself has none,
so it is held to (a), (b) AND (c).

COVERED maps every one of the header's 81 stream-taking exports to the test that reaches it (EXEMPT: the one without a
device-visible result); tests/test_stream_order_coverage.py holds both against the header.

What was found (MI355X, GPU_MAX_HW_QUEUES = 4):
  * every output of every case is bit for bit the default stream's, and every case returned while its delay still held
    the stream: no launch and no second stage of a reduction leaves the given stream, and no entry point or hip.py
    wrapper waits for the device.  Nothing in the library had to change;
  * the two hipMemsetAsync calls (gemm_h3.hip: the column-maxima words of an operand that is not k-contiguous, f16x3 NN
    and TN forms; step.hip: the amax words of the f16x3 step's kept weights) only zero words that the next kernels merge
    into with atomicMax, so a memset that ran too early would give the right maxima all the same.  load() therefore
    leaves STALE_AMAX (1e30) in hip.workspace and in the step's h3_workspace behind the delay: the cases
    gemm-f16x3-tn, gemm-f16x3-nn and sage_step-f16x3-kept reach the memsets and pass only if they are ordered on S;
  * not every side stream can show a misorder: on a pool stream that shares the null stream's hardware queue the
    positive control found the null-stream launch waiting behind the delay.  side_stream() probes for that;
  * no output had to be excused from bitwise equality: none is unrepeatable on the default stream;
  * delays: 20 ms (the floor) for all 59 cases, no case had to repeat; the host time of a warm-up call was 0.01 - 0.18 ms
    for the kernel-level cases and the steps, 1.2 - 1.9 ms for a module step (ten times that is below the floor);
    torch.cuda._sleep holds the stream for 1 ms per 2.39 million cycles;
  * the positive control sees the misorder: the null-stream launch overtakes S and its result differs;
  * one-off checks in scratch builds (not committed): with the stream of gist_colsum_f32's colsum_stage2_kernel launch
    and of gist_adam_f32's launch replaced by 0, the cases colsum, adam and module-sage fail at (a) in every word of the
    output concerned; with the stream of both hipMemsetAsync calls replaced by 0, gemm-f16x3-tn, gemm-f16x3-nn and
    sage_step-f16x3-kept fail at (a); everything else passes in both.
"""
import contextlib
import ctypes
import random
import time
import types
import zlib

import numpy as np
import pytest
import torch

from tests import test_scratch_bounds_kernels_gpu as KERNELS
from tests import test_spmm_kernels_gpu as SP
from tests import test_extract_kernels_gpu as X
from tests import test_class_layer_kernels_gpu as CL
from tests import test_gat_kernels_gpu as GATK

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F32 = np.float32
P_DROP, SEED = 0.2, 1234
MIN_DELAY_MS, HOST_FACTOR, MAX_REPEATS = 20.0, 10.0, 3
LR, WD = 0.01, 5e-4
# the bits of 1e30f: what load() leaves in every float scratch the library zeroes for itself (hipMemsetAsync of the amax
# words in gemm_h3.hip and step.hip, merged into with atomicMax).  A memset that ran too early is overwritten by it, the
# maxima stay at 1e30, the split scales and the output bits change; one ordered on the stream wipes it.  Finite, and only
# ever put into float scratch (tests/test_scratch_bounds_*_gpu.py fill the same buffers with NaN bytes).
STALE_AMAX = 0x7149F2CA


def stale(buf):
    """fill a uint8 scratch tensor with STALE_AMAX words, on the current stream"""
    buf[:buf.numel() // 4 * 4].view(torch.int32).fill_(STALE_AMAX)

# the wrappers of the module path that read a value back from the device in their own source (file: what) -- the only
# admissible reason not to assert (c) there
MODULE_READBACKS = {
    'gist_amd/ops.py:304': 'nnz = int(srp[-1].item()) in the induced-subgraph op behind Graph.subgraph: the size of the next allocation',
    'gist_amd/graph.py:85': 'int(self.rowptr[-1].item()) in Graph.number_of_edges, once per structure and only if unknown',
}


# ========================================================================================================================
# the harness
# ========================================================================================================================
_CYCLES_PER_MS = []


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, measured once with a pair of events"""
    if not _CYCLES_PER_MS:
        torch.cuda._sleep(1000000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20000000
        a.record()
        torch.cuda._sleep(n)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.5, 'torch.cuda._sleep(%d) held the stream for %.3f ms only: it is no delay on this runtime' % (n, ms)
        _CYCLES_PER_MS.append(n / ms)
        print('torch.cuda._sleep: %.0f cycles per ms' % _CYCLES_PER_MS[0])
    return _CYCLES_PER_MS[0]


def side_stream():
    """A torch.cuda.Stream() that the null stream really runs beside.  The runtime spreads its streams over a few hardware
    queues (GPU_MAX_HW_QUEUES) and a queue runs in order: on a stream that shares the null stream's queue a launch
    wrongly issued to stream 0 would wait behind the delay like a correct one, and every check of this file would pass
    whatever the library did (seen on the MI355X: the positive control found no misorder on such a stream).  So a
    candidate is probed first: a 5 ms
    delay on it, then an event on the null stream, which must complete while the delay still holds the candidate."""
    for _ in range(16):
        S = torch.cuda.Stream()
        held, free = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(S):
            torch.cuda._sleep(int(5 * cycles_per_ms()))
            held.record(S)
        free.record(torch.cuda.default_stream())
        t0 = time.perf_counter()
        while not free.query() and not held.query() and time.perf_counter() - t0 < 0.1:
            pass
        beside = free.query() and not held.query()
        S.synchronize()
        torch.cuda.synchronize()
        if beside and S.cuda_stream != 0:
            return S
    raise AssertionError('inconclusive: none of 16 pool streams runs beside the null stream on this runtime')


def bits(t):
    t = t.contiguous()
    if t.dtype in (torch.float32, torch.int32):
        return t.view(torch.int32)
    return t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


def _keep(outs):
    """clones of the device outputs, on the current stream (host outputs are read after the synchronise)"""
    return [o.clone() if o.is_cuda else None for o in outs]


def _finish(outs, kept):
    return [o.clone() if k is None else k for o, k in zip(outs, kept)]


def protocol(what, load, call, prepare=None, after=None, expect_equal=True, assert_early=True):
    """The three steps of the module docstring.  prepare(v): host-side state of variant v (before any delay starts);
    load(v): the device copies that put v into the live buffers, on the current stream; call() -> [output tensors];
    after(which) -> extra host figures of a run, taken after its synchronise.  -> (delay in ms, repeats) it needed."""
    prepare = prepare or (lambda v: None)
    delay_ms, repeats = None, 0
    while True:
        # 1. warm-up with A on the default stream: twice, the first call loads the code objects and grows the workspaces,
        #    the second is the one whose host time sizes the delay
        prepare('A')
        load('A')
        call()
        torch.cuda.synchronize()
        prepare('A')
        load('A')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = call()
        host_ms = (time.perf_counter() - t0) * 1e3
        first = _keep(outs)
        torch.cuda.synchronize()
        first = _finish(outs, first)
        extra1 = after('warm-up') if after else None
        if delay_ms is None:
            delay_ms = max(MIN_DELAY_MS, HOST_FACTOR * host_ms)
        # 2. B behind a delay on a side stream
        prepare('B')
        S = side_stream()
        with torch.cuda.stream(S):
            torch.cuda._sleep(int(delay_ms * cycles_per_ms()))
            delay_done = torch.cuda.Event()
            delay_done.record(S)
            load('B')
            outs = call()
            returned_early = not delay_done.query()
            side = _keep(outs)
        S.synchronize()
        side = _finish(outs, side)
        extra2 = after('side stream') if after else None
        torch.cuda.synchronize()
        if returned_early or not assert_early or repeats == MAX_REPEATS:
            break
        repeats += 1
        delay_ms *= 2
    # 3. the expected result: B on the default stream
    prepare('B')
    load('B')
    outs = call()
    want = _keep(outs)
    torch.cuda.synchronize()
    want = _finish(outs, want)
    extra3 = after('default stream') if after else None
    print('%s: delay %.0f ms, warm-up call %.2f ms on the host, %d repeats, returned early: %s'
          % (what, delay_ms, host_ms, repeats, returned_early))
    assert len(side) == len(want) == len(first) and len(want) >= 1
    for i, (s, w, f) in enumerate(zip(side, want, first)):
        assert s.shape == w.shape == f.shape and s.dtype == w.dtype, (what, i)
        assert not torch.equal(bits(w), bits(f)), '%s: output %d is the same for A and B: the case cannot tell them apart' % (what, i)
        same = torch.equal(bits(s), bits(w))
        if expect_equal:
            assert same, ('%s: output %d on the side stream differs from the default stream\'s in %d of %d words (%s A\'s)'
                          % (what, i, int((bits(s) != bits(w)).sum()), bits(w).numel(),
                             'it is' if torch.equal(bits(s), bits(f)) else 'nor is it'))
    if after:
        assert extra2 == extra3, '%s: %r on the side stream, %r on the default stream' % (what, extra2, extra3)
    if assert_early:
        assert returned_early, ('%s: inconclusive -- the call returned after a delay of %.0f ms had ended (%d repeats): it '
                                'waits for the device, or the host is that slow' % (what, delay_ms, repeats))
    if not expect_equal:
        return [torch.equal(bits(s), bits(w)) for s, w in zip(side, want)]
    return delay_ms, repeats


# ========================================================================================================================
# the table of kernel-level cases
# ========================================================================================================================
CASES = []


class Case(object):
    def __init__(self, name, exports, make, call, ctx=None, mode=None, tune=None, pinned=()):
        self.name, self.exports, self.make, self.call, self.ctx = name, tuple(exports), make, call, ctx
        self.mode, self.tune, self.pinned = mode, dict(tune or {}), tuple(pinned)

    @contextlib.contextmanager
    def settings(self):
        """the process-wide GEMM mode and tuning hooks of the case, put back afterwards"""
        from gist_amd import hip
        prev_mode, prev = hip.gemm_mode(), {k: hip.tuning(k) for k in self.tune}
        try:
            if self.mode is not None:
                hip.gemm_mode(self.mode)
            for k, v in self.tune.items():
                hip.tuning(k, v)
            yield
        finally:
            for k, v in prev.items():
                hip.tuning(k, v)
            hip.gemm_mode(prev_mode)


def case(name, exports, ctx=None, mode=None, tune=None, pinned=()):
    """@case(...) on a function make_and_call() -> (make, call)"""
    def deco(fn):
        make, call = fn()
        CASES.append(Case(name, exports, make, call, ctx, mode, tune, pinned))
        return fn
    return deco


def rs_of(name, v):
    return np.random.RandomState(zlib.crc32(name.encode()) % (1 << 30) + {'A': 0, 'B': 1}[v])


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def rnd(rs, *shape):
    return T(rs.randn(*shape).astype(F32))


def pos(rs, *shape):
    return T((rs.rand(*shape) + 0.5).astype(F32))


def i32(a):
    return T(np.asarray(a).astype(np.int32))


def zeros(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def L_():
    from gist_amd import _lib
    return _lib.load()


def st():
    from gist_amd import hip
    return hip._stream()


def ck(rc, name):
    from gist_amd import _lib
    _lib.check(rc, name)


# -- projections -----------------------------------------------------------------------------------------------------------
def _gemm_operands(rs, form, m, n, k):
    if form == 'nt':
        return dict(a=rnd(rs, m, k), b=rnd(rs, n, k), bias=rnd(rs, n), c=rnd(rs, m, n))
    if form == 'nn':
        return dict(a=rnd(rs, m, k), b=rnd(rs, k, n), c=rnd(rs, m, n))
    return dict(a=rnd(rs, k, m), b=rnd(rs, k, n), c=rnd(rs, m, n))


def _gemm_case(mode, hooks, form, m, n, k, launches):
    name = 'gemm-%s-%s-%dx%dx%d' % (mode, form, m, n, k)

    def ctx():
        from gist_amd import hip
        plan = hip.gemm_plan(form, m, n, k)
        assert plan['launches'] > 1 and (launches is None or plan['launches'] == launches), plan
        return plan

    def call(t, plan):
        from gist_amd import hip
        if form == 'nt':
            hip.gemm_nt(t['a'], t['b'], t['bias'], t['c'])
        else:
            (hip.gemm_nn if form == 'nn' else hip.gemm_tn)(t['a'], t['b'], t['c'])
        return [t['c']]

    CASES.append(Case(name, ['gist_gemm_%s_f32' % form], lambda v: _gemm_operands(rs_of(name, v), form, m, n, k), call,
                      ctx, mode, hooks))


# the cases of tests/test_gemm_plan_gpu.py that take more than one launch (split-K + reduce; the f16x3 / bf16x3 paths with
# their pre-passes) at up to 300 x 256 outputs, and the NN / TN forms on the split-K shapes of the slab cases
for (_mode, _hooks, _form, _m, _n, _k, _full, _less) in KERNELS.PLAN_CASES:
    if _full[4] > 1 and _m * _n <= 300 * 256:
        _gemm_case(_mode, _hooks, _form, _m, _n, _k, _full[4])
for (_form, _m, _n, _k) in KERNELS.SLAB_CASES[1:]:
    _gemm_case('f32', {}, _form, _m, _n, _k, None)
# gemm_h3.hip zeroes its column-maxima words (hipMemsetAsync) for an operand that is not k-contiguous: B of the NN form, A
# and B of the TN form (the f16x3 TN case above); the H3 path is the f16x3 mode's, bf16x3 has no such words
_gemm_case('f16x3', {'h3_min_tiles': 1, 'h3_min_gflop': 0.001}, 'nn', 200, 200, 96, None)


def _slab_floats(m, n, k):
    return max(int(L_().gist_gemm_workspace_bytes(m, n, k)) // 4, 4)


@case('gemm_slabs', ['gist_gemm_slabs_f32'], mode='f32')
def _():
    form, m, n, k = KERNELS.SLAB_CASES[0]

    def make(v):
        rs = rs_of('gemm_slabs', v)
        return dict(_gemm_operands(rs, form, m, n, k), slabs=rnd(rs, _slab_floats(m, n, k)))

    def call(t, c):
        from gist_amd import hip
        ns = hip.gemm_slabs(form, t['a'], t['b'], t['bias'], t['c'], t['slabs'])
        assert ns > 1, 'the case is meant to defer its slabs'
        return [t['slabs'][:ns * m * n]]
    return make, call


def _nn_drop_case(kind_, m, n, k, off):
    name = 'gemm_nn_dropout-%s-%dx%dx%d' % (kind_, m, n, k)

    def make(v):
        rs = rs_of(name, v)
        chunks = int(L_().gist_row_chunks16(m))
        return dict(g=rnd(rs, m, k), w=rnd(rs, k, n), z=rnd(rs, m, n), z2=rnd(rs, m, n), part=rnd(rs, chunks * k))

    def call(t, c):
        from gist_amd import hip
        hip.gemm_nn_dropout_(t['g'], t['w'], t['z'], P_DROP, SEED, off)
        hip.gemm_nn_dropout_colsum_(t['g'], t['w'], t['z2'], P_DROP, SEED, off, t['part'])      # (the offset's parity picks the form)
        return [t['z'], t['z2'], t['part']]

    CASES.append(Case(name, ['gist_gemm_nn_dropout_f32', 'gist_gemm_nn_dropout_colsum_f32'], make, call, None, 'f32'))


_nn_drop_case(*KERNELS.NN_DROP_CASES[1])      # narrow: one kernel
_nn_drop_case(*KERNELS.NN_DROP_CASES[3])      # two kernels, split-K workspace


@case('gemm_nn_tn_dual', ['gist_gemm_nn_tn_dual_f32'], mode='f32')
def _():
    m, n, k = KERNELS.DUAL_CASES[0]

    def make(v):
        rs = rs_of('dual', v)
        return dict(dy=rnd(rs, m, k), w=rnd(rs, k, n), z=rnd(rs, m, n), dz=rnd(rs, m, n), dw=rnd(rs, k, n),
                    slabs=rnd(rs, _slab_floats(k, n, m)))

    def call(t, c):
        from gist_amd import hip
        assert hip.gemm_dual_takes(t['dy'], t['w'], t['z'], t['dz'])
        ns = hip.gemm_nn_tn_dual(t['dy'], t['w'], t['dz'], t['z'], t['dw'], t['slabs'])
        return [t['dz'], t['slabs'][:ns * k * n] if ns > 1 else t['dw']]
    return make, call


@case('b3_split', ['gist_b3_split_f32'])
def _():
    def make(v):
        return dict(src=rnd(rs_of('b3', v), 128, 128))

    def call(t, c):
        from gist_amd import hip
        return list(hip.b3_split(t['src'], p=P_DROP, seed=SEED, offset=10, col_partials=True))
    return make, call


# -- row kernels -----------------------------------------------------------------------------------------------------------
@case('colsum', ['gist_colsum_f32', 'gist_colsum_chunks_f32'])
def _():
    n, d = 257, 41          # five 64-row chunks: both stages of gist_colsum_f32

    def make(v):
        rs = rs_of('colsum', v)
        return dict(g=rnd(rs, n, d), part=rnd(rs, int(L_().gist_colsum_partials(n)) * d), out=rnd(rs, d), out2=rnd(rs, d))

    def call(t, c):
        from gist_amd import hip
        hip.colsum(t['g'], t['out'], t['part'])
        hip.colsum_chunks(t['g'].view(-1), n, d, t['out2'])
        return [t['out'], t['part'], t['out2']]
    return make, call


@case('ln_relu', ['gist_ln_relu_fwd_f32', 'gist_ln_relu_fwd_drop_f32', 'gist_ln_relu_fwd_slabs_f32', 'gist_ln_relu_bwd_f32',
                  'gist_ln_relu_bwd_colsum_f32'])
def _():
    n, d, ns = 130, 260, 3

    def make(v):
        rs = rs_of('ln_relu', v)
        chunks = int(L_().gist_row_chunks16(n))
        t = dict(slabs=rnd(rs, ns * n * d), bias=rnd(rs, d), g=rnd(rs, n, d), part=rnd(rs, chunks * d))
        for k in ('y1', 'y2', 'y3', 'o1', 'o2', 'o2b', 'o3', 'o3b', 'dy1', 'dy2'):
            t[k] = rnd(rs, n, d)
        for k in ('r1', 'r2', 'r3'):
            t[k] = pos(rs, n)
        return t

    def call(t, c):
        from gist_amd import hip
        hip.ln_relu_fwd(t['y1'], t['o1'], t['r1'], True, True)
        hip.ln_relu_fwd_drop(t['y2'], t['o2'], t['o2b'], t['r2'], True, True, P_DROP, SEED, 7, d + 4)
        hip.ln_relu_fwd_slabs(t['y3'], t['slabs'], ns, t['bias'], t['o3'], t['o3b'], t['r3'], True, True, P_DROP, SEED, 9, d)
        hip.ln_relu_bwd(t['g'], t['y1'], t['r1'], t['dy1'], True, True)
        hip.ln_relu_bwd_colsum(t['g'], t['y2'], t['r2'], t['dy2'], True, True, t['part'])
        return [t[k] for k in ('y1', 'o1', 'r1', 'y2', 'o2', 'o2b', 'r2', 'y3', 'o3', 'o3b', 'r3', 'dy1', 'dy2', 'part')]
    return make, call


@case('class_layer', ['gist_class_layer_f32', 'gist_class_dw_slabs_f32', 'gist_ln_relu_bwd_colsum_class_dw_f32'])
def _():
    n, c, k = CL.OPT_SHAPE

    def make(v):
        rs = rs_of('class', v)
        z, w, b, lab = CL.make_inputs(n, c, k, seed={'A': 0, 'B': 1}[v])
        chunks = int(L_().gist_row_chunks16(n))
        slab = max(int(L_().gist_class_dw_slab_bytes(n, c, k)) // 4, 4)
        return dict(z=T(z), w=T(w), b=T(b), lab=T(lab), logits=rnd(rs, n, c), dl=rnd(rs, n, CL.round4(c)), nll=rnd(rs, n),
                    dz=rnd(rs, n, k), part=rnd(rs, chunks * c), slabs=rnd(rs, slab), slabs2=rnd(rs, slab),
                    g=rnd(rs, n, k), yhat=rnd(rs, n, k), rstd=pos(rs, n), dy=rnd(rs, n, k), cpart=rnd(rs, chunks * k))

    def call(t, c_):
        from gist_amd import hip
        assert hip.class_layer_takes(t['z'], t['w'], c)
        hip.class_layer(t['z'], t['w'], t['b'], t['lab'], n, t['logits'], t['dl'], t['nll'], t['dz'], P_DROP, SEED, 6, t['part'])
        ns = hip.class_dw_slabs(t['dl'][:, :c], t['z'], t['slabs'])
        ns2 = hip.ln_relu_bwd_colsum_class_dw(t['g'], t['yhat'], t['rstd'], t['dy'], True, True, t['cpart'], t['dl'][:, :c],
                                              t['z'], t['slabs2'])
        assert ns >= 1 and ns2 == ns
        return [t['logits'], t['dl'], t['nll'], t['dz'], t['part'], t['slabs'][:ns * c * k], t['slabs2'][:ns * c * k], t['dy'],
                t['cpart']]
    return make, call


@case('softmax_xent', ['gist_softmax_xent_f32', 'gist_softmax_xent_slabs_f32', 'gist_argmax_correct_i32'])
def _():
    n, c, ns = 300, 41, 3

    def make(v):
        rs = rs_of('xent', v)
        t = dict(logits=rnd(rs, n, c), lab=i32(rs.randint(0, c, n)), slabs=rnd(rs, ns * n * c), bias=rnd(rs, c),
                 logits2=rnd(rs, n, c), correct=i32([{'A': 5, 'B': 1000}[v]]))
        for k in ('nll', 'nll2'):
            t[k] = rnd(rs, n)
        for k in ('loss', 'loss2'):
            t[k] = rnd(rs, 1)
        for k in ('dl', 'dl2'):
            t[k] = rnd(rs, n, c)
        return t

    def call(t, c_):
        from gist_amd import hip
        hip.softmax_xent(t['logits'], t['lab'], None, n, t['nll'], t['loss'], t['dl'])
        hip.softmax_xent_slabs(t['logits2'], t['slabs'], ns, t['bias'], t['lab'], None, n, t['nll2'], t['loss2'], t['dl2'])
        hip.argmax_correct(t['logits2'], t['lab'], None, t['correct'])
        return [t[k] for k in ('nll', 'loss', 'dl', 'logits2', 'nll2', 'loss2', 'dl2', 'correct')]
    return make, call


def _adam_state(rs, n):
    return dict(p=rnd(rs, n), g=rnd(rs, n), m=T((rs.randn(n) * 0.1).astype(F32)), v=T((rs.rand(n) * 0.01).astype(F32)))


ADAM_N, ADAM_SEGS = 5037, [(1000, 1777, 3), (3000, 4100, 5)]      # tests/test_extract_kernels_gpu.py: ADAM_SEGS


def _segments(t):
    from gist_amd import _lib
    arr = (_lib.GradSegment * len(ADAM_SEGS))()
    for i, (b, e, ns) in enumerate(ADAM_SEGS):
        src = t['src%d' % i]
        arr[i].begin, arr[i].end, arr[i].src, arr[i].stride, arr[i].n_src = b, e, src.data_ptr(), src.shape[1], ns
    return arr


def _adam_make(name, extra=None):
    def make(v):
        rs = rs_of(name, v)
        t = _adam_state(rs, ADAM_N)
        for i, (b, e, ns) in enumerate(ADAM_SEGS):
            t['src%d' % i] = rnd(rs, ns, e - b + 3)
        t['nll'], t['loss'] = T(np.abs(rs.randn(777)).astype(F32)), rnd(rs, 1)
        if extra:
            t.update(extra(rs, v))
        return t
    return make


@case('adam', ['gist_adam_f32', 'gist_adam_segments_f32', 'gist_grad_segments_finish_f32'])
def _():
    def extra(rs, v):
        t = {k + '2': x for k, x in _adam_state(rs, ADAM_N).items()}
        t['g3'] = rnd(rs, ADAM_N)
        return t

    def call(t, c):
        from gist_amd import hip
        hip.adam_(t['p'], t['g'], t['m'], t['v'], 3, LR, weight_decay=WD)
        hip.adam_segments_(t['p2'], t['g2'], t['m2'], t['v2'], 3, LR,
                           [(b, e, t['src%d' % i], t['src%d' % i].shape[1], ns) for i, (b, e, ns) in enumerate(ADAM_SEGS)],
                           row_loss=t['nll'], n_loss_rows=777, loss_count=774, loss=t['loss'], weight_decay=WD)
        ck(L_().gist_grad_segments_finish_f32(t['g3'].data_ptr(), ADAM_N, _segments(t), len(ADAM_SEGS), st()),
           'gist_grad_segments_finish_f32')
        return [t[k] for k in ('p', 'm', 'v', 'p2', 'g2', 'm2', 'v2', 'loss', 'g3')]
    return _adam_make('adam', extra), call


@case('ln_all', ['gist_ln_all_fwd_f32', 'gist_ln_all_bwd_f32'])
def _():
    n = 43328          # tests/test_scratch_bounds_kernels_gpu.py ln_all_sizes: more than one workgroup

    def make(v):
        rs = rs_of('ln_all', v)
        return dict(x=rnd(rs, n), yhat=rnd(rs, n), stats=rnd(rs, 2), g=rnd(rs, n), dx=rnd(rs, n))

    def call(t, c):
        from gist_amd import hip
        hip.ln_all_fwd(t['x'], t['yhat'], t['stats'])
        hip.ln_all_bwd(t['g'], t['yhat'], t['stats'], t['dx'])
        return [t['yhat'], t['stats'], t['dx']]
    return make, call


@case('ln_affine', ['gist_ln_affine_fwd_f32', 'gist_ln_affine_fwd_drop_f32', 'gist_ln_affine_infer_f32', 'gist_ln_affine_bwd_f32'])
def _():
    d, n, relu, _lb = KERNELS.LNA_CASES[1]

    def make(v):
        rs = rs_of('ln_affine', v)
        t = dict(x=rnd(rs, n, d), lb=rnd(rs, d), gamma=pos(rs, d), beta=rnd(rs, d), g=rnd(rs, n, d),
                 ws=rnd(rs, max(int(L_().gist_ln_affine_bwd_workspace_floats(n, d)), 1)))
        for k in ('yhat', 'out', 'yhat2', 'out2', 'out2b', 'out3', 'dx'):
            t[k] = rnd(rs, n, d)
        for k in ('rstd', 'rstd2'):
            t[k] = pos(rs, n)
        for k in ('dgamma', 'dbeta', 'dlb'):
            t[k] = rnd(rs, d)
        return t

    def call(t, c):
        from gist_amd import hip
        hip.ln_affine_fwd(t['x'], t['lb'], t['gamma'], t['beta'], t['yhat'], t['out'], t['rstd'], relu)
        hip.ln_affine_fwd_drop(t['x'], t['lb'], t['gamma'], t['beta'], t['yhat2'], t['out2'], t['out2b'], t['rstd2'], relu,
                               P_DROP, SEED, 11, d + 2)
        hip.ln_affine_infer(t['x'], t['lb'], t['gamma'], t['beta'], t['out3'], relu)
        hip.ln_affine_bwd(t['g'], t['yhat'], t['rstd'], t['gamma'], t['beta'], relu, t['dx'], t['dgamma'], t['dbeta'], t['dlb'],
                          ws=t['ws'])
        return [t[k] for k in ('yhat', 'out', 'rstd', 'yhat2', 'out2', 'out2b', 'rstd2', 'out3', 'dx', 'dgamma', 'dbeta', 'dlb')]
    return make, call


@case('gcn_tail', ['gist_gcn_tail_fwd_f32', 'gist_gcn_tail_infer_f32', 'gist_gcn_tail_bwd_f32'])
def _():
    n, d = 130, 66

    def make(v):
        rs = rs_of('gcn_tail', v)
        t = dict(x=rnd(rs, n, d), b=rnd(rs, d), stats=rnd(rs, 2), stats2=rnd(rs, 2), g=rnd(rs, n, d), dbias=rnd(rs, d),
                 ws=rnd(rs, max(int(L_().gist_gcn_tail_bwd_workspace_floats(n, d)), 2)),
                 ws_f=rnd(rs, int(L_().gist_ln_all_partials(n * d))), ws_i=rnd(rs, int(L_().gist_ln_all_partials(n * d))))
        for k in ('yhat', 'out', 'out2', 'dx'):
            t[k] = rnd(rs, n, d)
        return t

    def call(t, c):
        from gist_amd import hip
        hip.gcn_tail_fwd(t['x'], t['b'], t['yhat'], t['out'], t['stats'], True, True, P_DROP, SEED, 5, ws=t['ws_f'])
        hip.gcn_tail_infer(t['x'], t['b'], t['out2'], True, True, stats=t['stats2'], ws=t['ws_i'])
        hip.gcn_tail_bwd(t['g'], t['x'], t['b'], t['yhat'], t['stats'], t['dx'], t['dbias'], True, True, P_DROP, SEED, 5,
                         ws=t['ws'])
        return [t[k] for k in ('yhat', 'out', 'stats', 'out2', 'stats2', 'dx', 'dbias')]
    return make, call


@case('dropout', ['gist_dropout_f32'])
def _():
    def make(v):
        return dict(z=rnd(rs_of('dropout', v), 130, 66))

    def call(t, c):
        from gist_amd import hip
        hip.dropout_(t['z'], P_DROP, SEED, 3)
        return [t['z']]
    return make, call


@case('standard_scaler', ['gist_standard_scaler_f32'])
def _():
    n, d, n_fit = 700, 50, 300          # tests/test_scratch_bounds_kernels_gpu.py: test_standard_scaler (five launches)

    def make(v):
        rs = rs_of('scaler', v)
        x = (rs.randn(n, d) * rs.uniform(0.01, 30, d) + rs.uniform(-50, 50, d)).astype(F32)
        return dict(x=T(x), rows=i32(np.sort(rs.choice(n, n_fit, replace=False))))

    def call(t, c):
        from gist_amd import hip
        mean, var = hip.standard_scale_(t['x'], t['rows'])
        return [t['x'], mean, var]
    return make, call


# -- aggregation -----------------------------------------------------------------------------------------------------------
def _sp_graph(gname, v):
    """A: the named graph of tests/test_spmm_kernels_gpu.py; B: its transpose -- as many rows, as many edges"""
    n, rowptr, col, trp, tcl, cuts = SP.graph(gname)
    a, b = ((rowptr, col), (trp, tcl)) if v == 'A' else ((trp, tcl), (rowptr, col))
    return dict(rp=i32(a[0]), cl=i32(a[1]), trp=i32(b[0]), tcl=i32(b[1]))


def _sp_ctx(gname):
    def ctx():
        cuts = SP.graph(gname)[5]
        return None if cuts is None else i32(cuts).to(DEV)
    return ctx


SP_BY_ID = {c['id']: c for c in SP.CASES}
# (case of tests/test_spmm_kernels_gpu.py, form, mode, exports reached)
SPMM_PICKS = [
    ('v4_l16_d64', 'fwd', 0, ['gist_spmm_csr_f32']), ('rs_v1_d33', 'bwd', 0, ['gist_spmm_csr_f32']),
    ('v4_l16_d64', 'fwd', 1, ['gist_spmm_csr_drop_f32']), ('lds_d260', 'bwd', 2, ['gist_spmm_csr_drop_f32']),
    ('lds_d260', 'fwd', 0, ['gist_spmm_csr_blocked_f32']), ('mf_unprep_forced_d256', 'fwd', 0, ['gist_spmm_csr_blocked_f32']),
    ('mf_single_block', 'fwd', 0, ['gist_spmm_blocks_prepare', 'gist_spmm_csr_prepared_f32']),
    ('d32_d130_rt4', 'bwd', 0, ['gist_spmm_blocks_prepare', 'gist_spmm_csr_prepared_f32']),
    ('mf_single_block', 'fwd', 1, ['gist_spmm_blocks_prepare', 'gist_spmm_csr_drop_prepared_f32']),
    ('d32_mode2_rt2', 'bwd', 2, ['gist_spmm_blocks_prepare', 'gist_spmm_csr_drop_prepared_f32']),
]


def _spmm_case(cid, form, mode, exports):
    c = SP_BY_ID[cid]
    assert mode in c['modes'], (cid, mode)
    n, d = SP.graph(c['graph'])[0], c['d']
    name = 'spmm-%s-%s-mode%d' % (cid, form, mode)
    rb_given = SP.has_blocks(c)

    def make(v):
        rs = rs_of(name, v)
        return dict(_sp_graph(c['graph'], v), xb=rnd(rs, n + 2, max(c['ldx'], 1)), yb=rnd(rs, n + 2, max(c['ldy'], 1)),
                    osc=pos(rs, n), ssc=pos(rs, n))

    def call(t, cuts):
        from gist_amd import hip
        b = types.SimpleNamespace(x=t['xb'][:n, c['ox']:c['ox'] + d], y=t['yb'][1:n + 1, c['oy']:c['oy'] + d])
        rb = cuts if rb_given else None
        prep = hip.spmm_prepare(t['rp'], t['cl'], rb) if c['entry'] == 'prepared' else None
        SP.call(c, form, mode, t['rp'], t['cl'], rb, prep, b, t['osc'], t['ssc'] if form == 'bwd' else None, form == 'bwd')
        return [t['yb']]      # (the structure itself may have bytes no call defines: it is judged by what reads it)

    CASES.append(Case(name, exports, make, call, _sp_ctx(c['graph']), None, c['tune']))


for _pick in SPMM_PICKS:
    _spmm_case(*_pick)


@case('spmm_lnbwd', ['gist_spmm_csr_drop_lnbwd_f32'], ctx=_sp_ctx(SP.LNB[1]['graph']), tune=SP.LNB[1]['tune'])
def _():
    c = SP.LNB[1]
    n, d = SP.graph(c['graph'])[0], c['d']
    nbk = len(SP.graph(c['graph'])[5]) - 1

    def make(v):
        rs = rs_of('lnbwd', v)
        units = int(L_().gist_spmm_lnb_units(nbk))
        return dict(_sp_graph(c['graph'], v), xb=rnd(rs, n + 2, c['ldx']), yb=rnd(rs, n + 2, c['ldy']), ssc=pos(rs, n),
                    yhat=rnd(rs, n, d), rstd=pos(rs, n), dy=rnd(rs, n + 1, d + 4), parts=rnd(rs, units, d))

    def call(t, cuts):
        from gist_amd import hip
        x, y = t['xb'][:n, c['ox']:c['ox'] + d], t['yb'][1:n + 1, c['oy']:c['oy'] + d]
        hip.spmm_drop_lnbwd(t['rp'], t['cl'], x, y, SP.P, SP.SEED, SP.Y_OFF, SP.X_OFF, SP.MASK_LD(c), t['yhat'], t['dy'][:n, :d],
                            t['parts'], src_scale=t['ssc'], row_blocks=cuts, rstd=t['rstd'])
        return [t['dy'], t['parts']]
    return make, call


@case('spmm_units_chains', ['gist_spmm_block_units_f32', 'gist_spmm_block_chains_f32'])
def _():
    # tests/test_spmm_kernels_gpu.py: test_spmm_units_and_chains_against_float64 at its narrowest width
    d = 132
    sizes = np.array([100, 128, 1, 57, 128, 90, 33])
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(bounds[-1])
    chains = {0: [0, 1, 3], 1: [1], 2: [2, 4, 0, 5, 6], 3: [], 4: [4, 0], 5: [5, 3, 1, 2], 6: [6, 6]}
    pairs_, cptr = [], [0]
    for r in sorted(chains):
        pairs_ += [(r, cb) for cb in chains[r]]
        cptr.append(len(pairs_))

    def make(v):
        rs = rs_of('units', v)
        stride = int(L_().gist_spmm_block_image_bytes()) // 2
        imgs, units, _ = SP._images(rs, sizes, bounds, pairs_, stride, False, d, None)
        t = dict(U=i32(np.array(units)), I=T(np.stack(imgs)).to(torch.bfloat16).contiguous(), xb=rnd(rs, n + 2, d + 8),
                 yb=rnd(rs, n + 2, d + 8), yb2=rnd(rs, n + 2, d + 8), osc=pos(rs, n), cptr=i32(cptr))
        for j in range(5):      # the units at position j of their chains (picked here: indexing on the device would copy
            sel = [cptr[r] + j for r in range(len(chains)) if cptr[r] + j < cptr[r + 1]]      # the index list from the host)
            t['U%d' % j], t['I%d' % j] = t['U'][sel].contiguous(), t['I'][sel].contiguous()
        return t

    def call(t, c):
        from gist_amd import hip
        x = t['xb'][:n, 4:4 + d]
        hip.spmm_block_chains(t['cptr'], t['U'], t['I'], x, t['yb'][1:n + 1, 4:4 + d], out_scale=t['osc'], accumulate=True)
        for j in range(5):      # one launch per position in the chains: units of a launch have disjoint output rows
            hip.spmm_block_units(t['U%d' % j], t['I%d' % j], x, t['yb2'][1:n + 1, 4:4 + d], out_scale=t['osc'], accumulate=True)
        return [t['yb'], t['yb2']]
    return make, call


@case('degree_norms', ['gist_in_degree_norm_f32', 'gist_gcn_degree_scales_f32'])
def _():
    n = SP.graph('small')[0]

    def make(v):
        g = _sp_graph('small', v)
        return dict(rp=g['rp'], trp=g['trp'], norm=zeros(n), nd=zeros(n), ns=zeros(n))

    def call(t, c):
        from gist_amd import hip
        hip.in_degree_norm(t['rp'], t['norm'])
        hip.gcn_degree_scales(t['rp'], t['trp'], t['nd'], t['ns'])
        return [t['norm'], t['nd'], t['ns']]
    return make, call


# -- graph attention -------------------------------------------------------------------------------------------------------
def _gat_case(cat):
    f, heads = GATK.DISPATCH_CASES[0]
    n = SP.graph('small')[0]
    w = heads * f if cat else f
    name = 'gat_layer_%s' % ('cat' if cat else 'mean')
    sfx = '_cat' if cat else ''

    def make(v):
        rs = rs_of(name, v)
        t = dict(_sp_graph('small', v), z=rnd(rs, n, heads * f), a=T((rs.randn(heads, 2 * f) * (2.0 / f ** 0.5)).astype(F32)),
                 d_out=rnd(rs, n, w), out=rnd(rs, n, w), g=rnd(rs, n, w), dz=rnd(rs, n, heads * f), da=rnd(rs, heads, 2 * f))
        for k in ('s_src', 's_dst', 'm', 'l', 'ds_dst', 'dd', 'ds_src'):
            t[k] = rnd(rs, n, heads)
        return t

    def call(t, c):
        from gist_amd import hip
        hip.gat_scores(t['z'], t['a'], t['s_src'], t['s_dst'])
        hip.gat_aggregate(t['rp'], t['cl'], t['z'], t['a'], t['s_src'], t['s_dst'], True, t['out'], t['m'], t['l'], cat=cat)
        hip.gat_backward_dst(t['rp'], t['cl'], t['z'], t['a'], t['out'], t['d_out'], t['s_src'], t['s_dst'], t['m'], t['l'], True,
                             t['g'], t['ds_dst'], t['dd'], cat=cat)
        hip.gat_backward_src(t['trp'], t['tcl'], t['z'], t['a'], t['g'], t['s_src'], t['s_dst'], t['m'], t['l'], t['dd'],
                             t['ds_dst'], t['dz'], t['ds_src'], cat=cat)
        hip.gat_attn_grad(t['z'], t['ds_src'], t['ds_dst'], t['da'])
        return [t[k] for k in ('s_src', 's_dst', 'out', 'm', 'l', 'g', 'ds_dst', 'dd', 'dz', 'ds_src', 'da')]

    CASES.append(Case(name, ['gist_gat_scores_f32', 'gist_gat_aggregate%s_f32' % sfx, 'gist_gat_backward_dst%s_f32' % sfx,
                             'gist_gat_backward_src%s_f32' % sfx, 'gist_gat_attn_grad_f32'], make, call))


_gat_case(False)
_gat_case(True)


@case('gat_blocks', ['gist_gat_row_stats_f32', 'gist_gat_aggregate_blocks_f32'], ctx=_sp_ctx('parts_small'))
def _():
    f, heads = 36, 2
    n = SP.graph('parts_small')[0]

    def make(v):
        rs = rs_of('gat_blocks', v)
        t = dict(_sp_graph('parts_small', v), z=rnd(rs, n, heads * f), a=rnd(rs, heads, 2 * f), out=rnd(rs, n, f),
                 out_cat=rnd(rs, n, heads * f))
        for k in ('s_src', 's_dst', 'm', 'l'):
            t[k] = rnd(rs, n, heads)
        return t

    def call(t, cuts):
        from gist_amd import hip
        hip.gat_row_stats(t['rp'], t['cl'], t['s_src'], t['s_dst'], t['m'], t['l'])
        hip.gat_aggregate_blocks(t['rp'], t['cl'], cuts, t['z'], t['a'], t['s_src'], t['s_dst'], t['m'], t['l'], True, t['out'])
        hip.gat_aggregate_blocks(t['rp'], t['cl'], cuts, t['z'], t['a'], t['s_src'], t['s_dst'], t['m'], t['l'], False,
                                 t['out_cat'], cat=True)
        return [t['m'], t['l'], t['out'], t['out_cat']]
    return make, call


# -- extraction ------------------------------------------------------------------------------------------------------------
# the 'spec' graph of tests/test_extract_kernels_gpu.py (parts of 60, 120, 90, 352, 130, 80 rows): A is the batch of parts
# (1, 2), B of parts (4, 5) -- 210 rows each
EX_GRAPH, EX_PARTS, EX_N, EX_D = 'spec', {'A': (1, 2), 'B': (4, 5)}, 210, 24


def _ex_batch(v):
    """(ids, part_slot table with the batch as number 0) of variant v"""
    G = X.build_graph(EX_GRAPH)
    slot = np.full((len(G.parts) + 1, 2), -1, np.int32)
    row = 0
    for p in EX_PARTS[v]:
        slot[p] = (0, row)
        row += len(G.parts[p])
    ids = np.concatenate([G.parts[p] for p in EX_PARTS[v]])
    assert len(ids) == EX_N
    return ids, slot


def _ex_ctx():
    G = X.build_graph(EX_GRAPH)
    feat, intra = X.features(EX_GRAPH, EX_D, 'int')
    g = types.SimpleNamespace(rowptr=i32(G.rowptr).to(DEV), col=i32(G.col).to(DEV), t_rowptr=i32(G.t_rowptr).to(DEV),
                              t_col=i32(G.t_col).to(DEV))
    return types.SimpleNamespace(g=g, G=G, labels=i32(G.labels).to(DEV), node_part=i32(G.node_part).to(DEV),
                                 feat=T(feat.astype(F32)).to(DEV), intra=T(intra.astype(F32)).to(DEV),
                                 scratch=X.new_scratch(EX_N + 5))


def _ex_outputs(rs, cap, names=('', )):
    t = {}
    for s in names:
        t.update({'rowptr' + s: i32(np.zeros(EX_N + 1)), 'col' + s: i32(np.zeros(cap)), 't_rowptr' + s: i32(np.zeros(EX_N + 1)),
                  't_col' + s: i32(np.zeros(cap)), 'norm' + s: rnd(rs, EX_N), 'lab' + s: i32(np.zeros(EX_N)),
                  'z' + s: rnd(rs, EX_N + 5, 2 * EX_D), 'x0' + s: rnd(rs, EX_N + 5, EX_D)})
    return t


def _ex_keys(s):
    return ['rowptr' + s, 'col' + s, 't_rowptr' + s, 't_col' + s, 'norm' + s, 'lab' + s, 'z' + s]


def _ex_cap():
    return int(len(X.build_graph(EX_GRAPH).col))


@case('induced', ['gist_induced_mark', 'gist_induced_unmark', 'gist_induced_rowptr', 'gist_induced_fill', 'gist_fill_i32'],
      ctx=_ex_ctx)
def _():
    def make(v):
        ids, _ = _ex_batch(v)
        N = X.build_graph(EX_GRAPH).n
        return dict(ids=i32(ids), remap=i32(np.full(N, -1)), srp=i32(np.zeros(EX_N + 1)), scol=i32(np.zeros(_ex_cap())),
                    filled=i32(np.zeros(64)), fill_value={'A': 7, 'B': -3}[v])

    def call(t, c):
        from gist_amd import hip
        hip.fill_i32_(t['filled'], t['fill_value'])
        hip.induced_mark(t['ids'], t['remap'])
        marked = t['remap'].clone()
        hip.induced_rowptr(c.g.rowptr, c.g.col, t['ids'], t['remap'], t['srp'])
        hip.induced_fill(c.g.rowptr, c.g.col, t['ids'], t['remap'], t['srp'], t['scol'])
        hip.induced_mark(t['ids'][:EX_N // 2], t['remap'], unmark=True)
        return [t['filled'], marked, t['srp'], t['scol'], t['remap']]
    return make, call


@case('extract_batch', ['gist_extract_batch', 'gist_extract_batch_drop'], ctx=_ex_ctx)
def _():
    def make(v):
        N = X.build_graph(EX_GRAPH).n
        return dict(_ex_outputs(rs_of('extract_batch', v), _ex_cap(), ('', '_d')), ids=i32(_ex_batch(v)[0]), remap=i32(np.full(N, -1)))

    def call(t, c):
        from gist_amd import hip
        hip.extract_batch(c.g, t['ids'], t['remap'], t['rowptr'], t['col'], t['t_rowptr'], t['t_col'], t['norm'], c.feat,
                          t['z'][:EX_N, :EX_D], c.labels, t['lab'])
        hip.extract_batch_drop(c.g, t['ids'], t['remap'], t['rowptr_d'], t['col_d'], t['t_rowptr_d'], t['t_col_d'], t['norm_d'],
                               c.feat, t['z_d'][:EX_N, :EX_D], c.labels, t['lab_d'], t['x0_d'][:EX_N], P_DROP, SEED, 1000,
                               2 * EX_D)
        return [t[k] for k in _ex_keys('') + _ex_keys('_d') + ['x0_d']]
    return make, call


def _parts_desc(t, c, s, drop, ah):
    """struct gist_extract_parts_desc of the case's buffers with suffix s"""
    from gist_amd import _lib
    x = _lib.ExtractPartsDesc()
    x.g_rowptr, x.g_col, x.g_t_rowptr, x.g_t_col = (u.data_ptr() for u in (c.g.rowptr, c.g.col, c.g.t_rowptr, c.g.t_col))
    x.ids, x.n, x.n_max = t['ids'].data_ptr(), EX_N, EX_N + 5
    x.node_part, x.part_slot, x.batch = c.node_part.data_ptr(), t['slot'].data_ptr(), 0
    x.rowptr, x.col, x.t_rowptr, x.t_col = (t[k + s].data_ptr() for k in ('rowptr', 'col', 't_rowptr', 't_col'))
    x.col_capacity, x.norm = t['col' + s].numel(), t['norm' + s].data_ptr()
    x.feat, x.ld_feat, x.n_feat = c.feat.data_ptr(), c.feat.stride(0), EX_D
    x.z0, x.ldz0 = t['z' + s].data_ptr(), 2 * EX_D
    x.labels_all, x.labels = c.labels.data_ptr(), t['lab' + s].data_ptr()
    if drop:
        x.x0, x.ldx0 = t['x0' + s].data_ptr(), EX_D
        x.p, x.seed, x.offset, x.mask_ld = P_DROP, SEED, 77, 2 * EX_D
    x.scratch = c.scratch.data_ptr()
    if ah:
        x.feat_intra, x.ld_intra = c.intra.data_ptr(), c.intra.stride(0)
        x.ah = t['z' + s].data_ptr() + 4 * EX_D
    return x


def _parts_make(name, names, extra=None):
    def make(v):
        rs = rs_of(name, v)
        ids, slot = _ex_batch(v)
        t = dict(_ex_outputs(rs, _ex_cap(), names), ids=i32(ids), slot=i32(slot))
        if extra:
            t.update(extra(v))
        return t
    return make


@case('extract_parts', ['gist_extract_parts_batch', 'gist_extract_parts_desc_batch'], ctx=_ex_ctx)
def _():
    def call(t, c):
        L = L_()
        x = _parts_desc(t, c, '', True, False)
        ck(L.gist_extract_parts_batch(x.g_rowptr, x.g_col, x.g_t_rowptr, x.g_t_col, x.ids, x.n, x.n_max, x.node_part, x.part_slot,
                                      x.batch, x.rowptr, x.col, x.t_rowptr, x.t_col, x.col_capacity, x.norm, x.feat, x.ld_feat,
                                      x.n_feat, x.z0, x.ldz0, x.labels_all, x.labels, x.x0, x.ldx0, x.p, x.seed, x.offset,
                                      x.mask_ld, x.scratch, st()), 'gist_extract_parts_batch')
        y = _parts_desc(t, c, '_d', False, True)
        ck(L.gist_extract_parts_desc_batch(ctypes.byref(y), st()), 'gist_extract_parts_desc_batch')
        return [t[k] for k in _ex_keys('') + ['x0'] + _ex_keys('_d')]
    return _parts_make('extract_parts', ('', '_d')), call


@case('adam_segments_extract', ['gist_adam_segments_extract_f32'], ctx=_ex_ctx)
def _():
    adam = _adam_make('adam_extract')

    def call(t, c):
        x = _parts_desc(t, c, '', True, True)
        ck(L_().gist_adam_segments_extract_f32(t['p'].data_ptr(), t['g'].data_ptr(), t['m'].data_ptr(), t['v'].data_ptr(), ADAM_N,
                                               LR, 0.9, 0.999, 1e-8, WD, 3, _segments(t), len(ADAM_SEGS), t['nll'].data_ptr(),
                                               777, 774, t['loss'].data_ptr(), ctypes.byref(x), st()),
           'gist_adam_segments_extract_f32')
        return [t[k] for k in ['p', 'g', 'm', 'v', 'loss', 'x0'] + _ex_keys('')]
    return _parts_make('adam_extract', ('',), adam), call


# -- gathers, block moves, host traffic ---------------------------------------------------------------------------------------
@case('gathers', ['gist_gather_rows_f32', 'gist_gather_i32', 'gist_block_gather_f32', 'gist_block_scatter_f32',
                  'gist_mean_rows_f32'])
def _():
    N, d, n = 500, 63, 257

    def make(v):
        rs = rs_of('gathers', v)
        return dict(src=rnd(rs, N, d + 1), isrc=i32(rs.randint(0, 1000, N)), ids=i32(rs.randint(0, N, n)), dst=rnd(rs, n, d + 5),
                    idst=i32(np.zeros(n)), rows=i32(rs.permutation(N)[:40]), cols=i32(rs.permutation(d)[:17]),
                    blk=rnd(rs, 40, 17), scat=rnd(rs, N, d + 1), mean=rnd(rs, 257))

    def call(t, c):
        from gist_amd import hip
        hip.gather_rows(t['src'][:, :d], t['ids'], t['dst'][:, :d])
        hip.gather_i32(t['isrc'], t['ids'], t['idst'])
        hip.block_gather(t['src'], t['rows'], t['cols'], t['blk'])
        hip.block_scatter(t['blk'], t['rows'], t['cols'], t['scat'])
        hip.mean_rows(t['src'].view(-1), 300, 7, 257, t['mean'])
        return [t['dst'], t['idst'], t['blk'], t['scat'], t['mean']]
    return make, call


@case('host_traffic', ['gist_copy_i32', 'gist_publish_i64'], pinned=('staged', 'mark'))
def _():
    n = 1000

    def make(v):
        rs = rs_of('host', v)
        return dict(staged=i32(rs.randint(0, 1 << 20, n)), dst=i32(np.zeros(n)), word=T(rs.randint(1, 1 << 40, 1).astype(np.int64)),
                    mark=T(np.zeros(2, np.int64)))

    def call(t, c):
        from gist_amd import hip
        assert t['staged'].is_pinned() and t['mark'].is_pinned()
        hip.copy_i32_raw(t['staged'].data_ptr(), t['dst'].data_ptr(), n)      # from a pinned host buffer
        hip.publish_i64_raw(t['word'].data_ptr(), 41, t['mark'].data_ptr())   # into one: read after the synchronise
        return [t['dst'], t['mark']]
    return make, call


ARENA_MOVES = [('gather', 0, 0, 40, 16, 20, 16, 0, 20), ('scatter', 1200, 400, 8, 32, 10, 8, 36, 46),
               ('mean', 1300, 1100, 50, 50, 3, 50, -1, -1)]


def _arena_table():
    from gist_amd import hip
    return hip.ArenaMoves(ARENA_MOVES, 1500, 1200, 54, DEV)


@case('arena_moves', ['gist_arena_moves_f32'], ctx=_arena_table)
def _():
    def make(v):
        rs = rs_of('arena_moves', v)
        idx = np.concatenate([rs.permutation(30)[:20], rs.permutation(40)[:16], rs.permutation(20)[:10], rs.permutation(32)[:8]])
        return dict(idx=i32(idx), src=rnd(rs, 1500), dst=rnd(rs, 1200))

    def call(t, table):
        from gist_amd import hip
        hip.arena_moves(table, t['idx'], t['src'], t['dst'])
        return [t['dst']]
    return make, call


# ========================================================================================================================
# running a kernel-level case
# ========================================================================================================================
def build_variants(c, device):
    """{variant: {name: tensor or host value}} of a case; tensors on `device`"""
    out = {}
    for v in ('A', 'B'):
        out[v] = {k: (x.to(device) if torch.is_tensor(x) else x) for k, x in c.make(v).items()}
    return out


def run_case(c, call=None, **kw):
    src = build_variants(c, DEV)
    live = {}
    for k, x in src['A'].items():
        if not torch.is_tensor(x):
            live[k] = x
        elif k in c.pinned:
            live[k] = torch.empty(x.shape, dtype=x.dtype, pin_memory=True)
        else:
            live[k] = torch.empty_like(x)
    with c.settings():
        context = c.ctx() if c.ctx else None
        torch.cuda.synchronize()

        def prepare(v):
            for k, x in src[v].items():
                if not torch.is_tensor(x):
                    live[k] = x

        def load(v):
            from gist_amd import hip
            for k, x in src[v].items():
                if torch.is_tensor(x):
                    live[k].copy_(x, non_blocking=True)
            stale(hip.workspace(1, DEV))

        return protocol(c.name, load, lambda: (call or c.call)(live, context), prepare, **kw)


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_stream_order(c):
    run_case(c)


def test_wrong_stream_is_caught():
    """The positive control: gist_colsum_f32 of the 'colsum' case handed stream 0 while B is made ready on S."""
    c = [x for x in CASES if x.name == 'colsum'][0]
    n, d = 257, 41

    def on_null_stream(t, context):
        ck(L_().gist_colsum_f32(t['g'].data_ptr(), d, n, d, t['part'].data_ptr(), t['out'].data_ptr(), 0), 'gist_colsum_f32')
        return [t['out']]

    same = run_case(c, on_null_stream, expect_equal=False)
    assert same == [False], 'a launch on the null stream was NOT seen to overtake the side stream: the checks of this file prove nothing here'


# ========================================================================================================================
# the one-call steps through their engines
# ========================================================================================================================
STEP_PARTS = [64, 65] * 4           # four batches of 129 rows: one past a multiple of 128
_STEP_DS = {}


def _step_data(n_feats):
    if n_feats not in _STEP_DS:
        from gist_amd import datasets
        ds = datasets.toy(seed=3, n=2400, n_blocks=24, n_feats=n_feats, n_classes=5, train_frac=1.0)
        order = np.concatenate([np.asarray(p, np.int64) for p in ds.par_li])
        cuts = np.concatenate([[0], np.cumsum(STEP_PARTS)])
        _STEP_DS[n_feats] = (ds, [order[cuts[i]:cuts[i + 1]].copy() for i in range(len(STEP_PARTS))])
    return _STEP_DS[n_feats]


def _step_iterator(ds, parts):
    from gist_amd.sampler import EngineClusterIter
    random.seed(0)
    nid = np.arange(ds.g.number_of_nodes(), dtype=np.int64)
    it = EngineClusterIter('toy', ds.g, len(parts), 2, nid, par_li=[p.copy() for p in parts], device=DEV)
    assert 129 <= it.n_max <= 130
    return it


def _build_sage(kept=False):
    from gist_amd import hip
    from gist_amd.engine import SageEngine, dims_for
    from tests.test_scratch_bounds_steps_gpu import _kept_width
    ds, parts = _step_data(30)
    it = _step_iterator(ds, parts)
    dims = dims_for(30, _kept_width(hip, it.n_max) if kept else 128, 5, 2)
    eng = SageEngine(dims, True, P_DROP, it.n_max, DEV, seed=11)
    gen = torch.Generator().manual_seed(1)
    for k, (i, o) in enumerate(dims):
        s_ = 1.0 / np.sqrt(2 * i)
        eng.arena.W[k].copy_((torch.rand(o, 2 * i, generator=gen) - 0.5) * 2 * s_)
        eng.arena.b[k].copy_((torch.rand(o, generator=gen) - 0.5) * 2 * s_)
    it.bind(eng)
    assert (eng.plan.h3_workspace is not None) == kept, 'the step is not on the path the case is named after'
    return eng, it, None


def _build_sage_kept():
    return _build_sage(True)


def _build_gat():
    from gist_amd.arena import gat_dims
    from gist_amd.gat_engine import GATEngine
    from gist_amd.ist import gat_params
    from gist_amd.modules import GAT
    ds, parts = _step_data(32)
    it = _step_iterator(ds, parts)
    torch.manual_seed(0)
    model = GAT(2, 32, 16, ds.num_classes, 2, merge='mean')
    eng = GATEngine(gat_dims(32, 16, ds.num_classes, 2, 2, merge='mean'), it.n_max, DEV)
    eng.arena.load(gat_params(model))
    it.bind(eng)
    return eng, it, model


def _build_graphsage():
    import torch.nn.functional as F
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.modules import GraphSAGE
    ds, parts = _step_data(32)
    it = _step_iterator(ds, parts)
    torch.manual_seed(0)
    model = GraphSAGE(32, 64, ds.num_classes, 2, F.relu, P_DROP, False).to(DEV)
    eng = GraphSAGEEngine(graphsage_dims(32, 64, ds.num_classes, 2), P_DROP, it.n_max, DEV, seed=7)
    eng.bind(model)
    it.bind(eng)
    return eng, it, model


def _build_baseline_gcn():
    import torch.nn.functional as F
    from gist_amd.arena import baseline_gcn_dims
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    from gist_amd.modules import BaselineGCN
    ds, parts = _step_data(32)
    it = _step_iterator(ds, parts)
    torch.manual_seed(0)
    model = BaselineGCN(32, 32, ds.num_classes, 2, F.relu, P_DROP, True).to(DEV)
    eng = BaselineGCNEngine(baseline_gcn_dims(32, 32, ds.num_classes, 2), True, P_DROP, it.n_max, DEV, seed=7)
    eng.bind(model)
    it.bind(eng)
    return eng, it, model


def _whole(eng, b):
    return eng.train_step(b, LR, WD)


def _phases(method):
    def run(eng, b):
        from gist_amd import _lib
        for phase in (_lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER):
            loss = getattr(eng, method)(b, LR, WD, True, phase=phase)
        return loss
    return run


# the hooks under which a step this small keeps its split operands (tests/test_scratch_bounds_steps_gpu.py: SAGE_HOOKS)
KEPT = ('bf16x3', {'h3_min_tiles': 1, 'h3_min_gflop': 0.001})
KEPT_F16 = ('f16x3', {'h3_min_tiles': 1, 'h3_min_gflop': 0.001})
F32_MODE = ('f32', {})
# (name, builder, how one iteration is called, exports reached, (GEMM mode, tuning hooks))
STEP_CASES = [
    ('sage_step', _build_sage, _whole, ['gist_sage_step'], F32_MODE),
    ('sage_step-phases', _build_sage, _phases('_native_step'), ['gist_sage_step'], F32_MODE),
    ('sage_step-bf16x3-kept', _build_sage_kept, _whole, ['gist_sage_step'], KEPT),
    ('sage_step-f16x3-kept', _build_sage_kept, _whole, ['gist_sage_step'], KEPT_F16),      # step.hip's hipMemsetAsync of the amax words
    ('gat_step', _build_gat, _whole, ['gist_gat_step'], F32_MODE),
    ('gat_step-phases', _build_gat, _phases('_step'), ['gist_gat_step_phase'], F32_MODE),
    ('graphsage_step', _build_graphsage, _whole, ['gist_graphsage_step'], F32_MODE),
    ('graphsage_step-phases', _build_graphsage, _phases('_native_step'), ['gist_graphsage_step_phase'], F32_MODE),
    ('baseline_gcn_step', _build_baseline_gcn, _whole, ['gist_baseline_gcn_step'], F32_MODE),
]
STEP_BATCH = {'A': 0, 'B': 2}      # batches of the epoch; with prefetch their optimiser launches extract batches 1 and 3


def _describe(it, j):
    """the lazy Batch of batch j of the current epoch: what EngineClusterIter.__next__ yields (nothing is launched)"""
    ids, n, row_blocks, parts, next_info = it.describe(j)
    b = it.batcher.lazy(ids)
    b.row_blocks, b.parts, b.next_info = row_blocks, parts, next_info
    b.siblings = it.has_siblings(j)
    return b


@pytest.mark.parametrize('name,build,run,exports,mode', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_stream_order(name, build, run, exports, mode):
    from gist_amd import hip
    L = L_()
    prev = hip.gemm_mode()
    try:
        hip.gemm_mode(mode[0])
        for knob, value in mode[1].items():
            hip.tuning(knob, value)
        eng, it, keep = build()
        eng.prefetch = True
        iter(it)                              # uploads the epoch's tables (a copy kernel on the default stream)
        eng.enable_timer(512)
        A = eng.arena
        gen = torch.Generator(device=DEV).manual_seed(5)
        state = {}
        for v, jitter in (('A', 0.0), ('B', 0.05)):
            state[v] = dict(params=A.params + jitter * torch.randn(A.params.shape, device=DEV, generator=gen),
                            grads=torch.randn(A.params.shape, device=DEV, generator=gen),
                            exp_avg=0.01 * torch.randn(A.params.shape, device=DEV, generator=gen),
                            exp_avg_sq=1e-4 * torch.rand(A.params.shape, device=DEV, generator=gen))
        torch.cuda.synchronize()
        cur = {}

        def prepare(v):
            A.step = {'A': 3, 'B': 8}[v]
            if hasattr(eng, 'drop_calls'):
                eng.drop_calls = {'A': 1000, 'B': 50000}[v]
            it.batcher.prefetched = None       # the step extracts its own batch AND the next one
            cur['b'] = _describe(it, STEP_BATCH[v])
            L.gist_timer_reset(eng._timer)

        def load(v):
            for k, x in state[v].items():
                getattr(A, k).copy_(x, non_blocking=True)
            if getattr(eng, '_h3_ws', None) is not None:
                stale(eng._h3_ws)

        def call():
            b = cur['b']
            run(eng, b)
            bt = it.batcher
            return [eng.loss, eng.logits(b.n), A.grads, A.params, A.exp_avg, A.exp_avg_sq, bt.rowptr[:b.n + 1], bt.col]

        def after(which):
            times = eng.read_timer()
            print('%s, %s: %d timer slots' % (name, which, len(times)))
            assert len(times) > 0, (name, which, 'the timer recorded nothing')
            assert all(np.isfinite(ms) and ms >= 0.0 for ms, _, _, _, _ in times), (name, which, times)
            return [(kind, m, n, k) for _, kind, m, n, k in times]

        protocol(name, load, call, prepare, after)
        assert it.batcher.prefetched is not None, 'the next batch was not extracted beside the optimiser'
        eng.check_extract()
        eng.disable_timer()
    finally:
        for knob in mode[1]:
            hip.tuning(knob, 0)
        hip.gemm_mode(prev)


# ========================================================================================================================
# the module path: one training step of each family's module loop
# ========================================================================================================================
def _model_sage():
    import torch.nn.functional as F
    from gist_amd.modules import GCN
    return GCN(32, 64, 5, 2, F.relu, P_DROP, use_layernorm=True, use_aggregation=True)


def _model_gat():
    from gist_amd.modules import GAT
    return GAT(2, 32, 16, 5, 2, merge='mean')


def _model_graphsage():
    import torch.nn.functional as F
    from gist_amd.modules import GraphSAGE
    return GraphSAGE(32, 64, 5, 2, F.relu, P_DROP, False)


def _model_baseline_gcn():
    import torch.nn.functional as F
    from gist_amd.modules import BaselineGCN
    return BaselineGCN(32, 32, 5, 2, F.relu, P_DROP, True)


MODULE_CASES = [('module-sage', _model_sage), ('module-gat', _model_gat), ('module-graphsage', _model_graphsage),
                ('module-baseline_gcn', _model_baseline_gcn)]


@pytest.mark.parametrize('name,new_model', MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_module_stream_order(name, new_model):
    """pred = model(cluster), CrossEntropyLoss, zero_grad, loss.backward(), optimizer.step() of an UNBOUND model on a
    cluster of 129 rows: the custom autograd ops, one launch each, with torch's own kernels between them.  The cluster is
    cut out before any delay starts (Graph.subgraph reads a size back: MODULE_READBACKS); A and B are other features,
    labels, parameters and Adam moments, and other dropout offsets / seeds."""
    from gist_amd import autograd, hip
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    prev = hip.gemm_mode()
    hip.gemm_mode('f32')
    try:
        ds, parts = _step_data(32)
        ids = np.concatenate([parts[0], parts[1]])
        g = ds.g.to(DEV)
        cluster = g.subgraph(ids)
        assert type(cluster).__name__ == 'Graph' and cluster.number_of_nodes() == 129
        torch.manual_seed(0)
        model = new_model().to(DEV)
        model.train()
        params = list(model.parameters())
        opt = Adam(params, lr=LR, weight_decay=WD)
        opt.state = [(torch.zeros_like(p.data), torch.zeros_like(p.data)) for p in params]
        loss_f = CrossEntropyLoss()
        feat, lab = cluster.ndata['feat'], cluster.ndata['label']
        gen = torch.Generator(device=DEV).manual_seed(9)
        rn = lambda t, scale: scale * torch.randn(t.shape, device=DEV, generator=gen)
        state = {}
        for v, jitter in (('A', 0.0), ('B', 0.05)):
            state[v] = dict(feat=feat + jitter * 10 * rn(feat, 1.0),
                            lab=torch.randint(0, 5, lab.shape, device=DEV, generator=gen).to(lab.dtype),
                            p=[p.data + rn(p, jitter) for p in params], m=[rn(p, 0.01) for p in params],
                            v=[rn(p, 0.01).square() for p in params])
        torch.cuda.synchronize()

        def prepare(v):
            opt.step_count = {'A': 3, 'B': 8}[v]
            autograd._drop_counter[0] = {'A': 1000, 'B': 50000}[v]
            torch.manual_seed({'A': 1, 'B': 2}[v])

        def load(v):
            feat.copy_(state[v]['feat'], non_blocking=True)
            lab.copy_(state[v]['lab'], non_blocking=True)
            for p, (m_, v_), sp, sm, sv in zip(params, opt.state, state[v]['p'], state[v]['m'], state[v]['v']):
                p.data.copy_(sp, non_blocking=True)
                m_.copy_(sm, non_blocking=True)
                v_.copy_(sv, non_blocking=True)

        def call():
            pred = model(cluster)
            loss = loss_f(pred, lab)
            opt.zero_grad()
            loss.backward()
            grads = [p.grad.clone() for p in params]
            opt.step()
            return ([pred.detach(), loss.detach()] + grads + [p.data for p in params] + [m_ for m_, _ in opt.state] +
                    [v_ for _, v_ in opt.state])

        protocol(name, load, call, prepare)
    finally:
        hip.gemm_mode(prev)


# ========================================================================================================================
# the coverage table
# ========================================================================================================================
COVERED = {}
for _c in CASES:
    for _e in _c.exports:
        COVERED.setdefault(_e, 'test_stream_order')
for _name, _build, _run, _exports, _mode in STEP_CASES:
    for _e in _exports:
        COVERED.setdefault(_e, 'test_step_stream_order')
# exports with no device-visible result to compare
EXEMPT = {
    'gist_empty_launches': 'launches kernels that read and write nothing (a launch-overhead probe): no result a stream order could change',
}
