"""The op-by-op twin of gist_sage_step: the SAME sequence, one C-ABI call per kernel, behind SageEngine.forward,
loss_and_backward and adam_step.  It is what the native step is compared with bit for bit, and it is the masked-loss
path, the evaluation path and what train_step runs under hip.profile_begin().  Cut like csrc/step.hip: one record of
the step (Step, filled by decide), then one function per phase.

Two launches of the native step are NOT followed here, on purpose: gist_ln_relu_bwd_colsum_class_dw_f32 (the class
layer's dW riding on the last hidden layer's LayerNorm backward) and gist_spmm_csr_drop_lnbwd_f32 (the reverse
aggregation carrying the next LayerNorm backward).  The twin issues their separate kernels, which give the same bits;
following them would change the sequence it issues.
"""
import ctypes

import torch

from . import _lib, hip


class Step(object):
    """One op-by-op step: created by forward (decide), read by loss_and_backward, consumed by optimise.  A fresh record
    is the "nothing forwarded yet" state, and every forward starts a fresh one: what a loss_and_backward deferred is
    dropped by a forward issued before the optimise that was to sum it (only train_step defers, and it does not).
    Decisions, taken before anything is launched:
      offs        dropout counter base of every layer ([]: no dropout in this step); blocked: the batch has row blocks
      fold        per layer: its dropout is folded into the producers of its [h | ah]
      slabs       the fused slabs are in play: split-K projections may stay slabs for their reader
      one_launch  a lazy batch takes the one-launch extraction, which also forms layer 0's ah
    Launch OUTCOMES cannot be decided up front; the phase that learns them stores them:
      prep_fwd, prep_bwd  the batch's prepared block structures, or None (forward)
      cls_fused   project_class left the class layer to loss()'s one launch; logit_slabs: or its logits as so many slabs
      segments    gradient pieces optimise() still has to sum (segment()); loss_rows: rows of row_loss it reduces"""
    __slots__ = ('offs', 'fold', 'slabs', 'one_launch', 'blocked',
                 'prep_fwd', 'prep_bwd', 'cls_fused', 'logit_slabs', 'segments', 'loss_rows')

    def __init__(self):
        self.offs, self.fold, self.segments = [], [], []
        self.slabs = self.one_launch = self.blocked = self.cls_fused = False
        self.prep_fwd = self.prep_bwd = None
        self.logit_slabs, self.loss_rows = 1, 0


def fused_buffers(eng):
    """Slabs / chunk sums of the op-by-op path, sized like the native step's (the split counts of
    the deferred projections must agree: gist_step_fused_slab_bytes)."""
    if eng._fused is not None:
        return eng._fused
    L = _lib.load()
    P = _lib.StepPlan()
    P.n_layers, P.n_max = eng.L1, eng.n_max
    for k, (i, o) in enumerate(eng.dims):
        P.layer[k].n_in, P.layer[k].n_out = i, o
    chunks = int(L.gist_row_chunks16(eng.n_max))
    nbs = [int(L.gist_step_fused_slab_bytes(ctypes.byref(P), which)) for which in range(eng.L1 + 2)]
    slabs = [torch.empty(nb, dtype=torch.uint8, device=eng.device) if nb > 0 else None for nb in nbs]
    eng._fused = {'dw': slabs[:eng.L1], 'logits': slabs[eng.L1], 'y': slabs[eng.L1 + 1],      # y: a hidden projection
                  'partials': [torch.zeros(max(chunks * o, 4), dtype=torch.float32, device=eng.device)
                               for (i, o) in eng.dims]}
    return eng._fused


def decide(eng, b, training, _step):
    """The forward decisions of a step, before anything is launched.  Advances the engine's dropout counter: layer k
    uses drop_calls + sum_{j<k} round_up(n * 2 * n_in_j, 2), as gist_sage_step does."""
    st, n = Step(), b.n
    st.blocked = b.row_blocks is not None and b.row_blocks.numel() > 1
    st.fold = [False] * eng.L1
    if training and eng.p_drop > 0.0:
        for k, (i, o) in enumerate(eng.dims):
            st.offs.append(eng.drop_calls)
            eng.drop_calls += n * 2 * i + ((n * 2 * i) & 1)
            st.fold[k] = (eng.fuse and eng.H[k] is not None and (k > 0 or (_step and not b.ready)) and
                          hip.spmm_drop_takes(1, i, eng.H[k][:n, :i], eng.Z[k][:n, i:], st.blocked))
    st.slabs = eng.fuse and training and _step
    if not b.ready:
        if b.batcher is None:
            raise RuntimeError('gist_amd: lazy batch without a batcher')
        # the native step's extraction sums layer 0's aggregation in its own order, so the twin runs the same launch
        st.one_launch = bool(b.batcher.feat_intra is not None and b.parts is not None and eng.fuse and
                             eng.plan is not None and eng.plan.feat_intra and
                             _lib.load().gist_extract_parts_supported(eng.n_max))
    return st


def extract(eng, st, b):
    """A lazy batch's extraction, with layer 0's dropout folded into the feature gather when st.fold[0]."""
    n, bt, i0 = b.n, b.batcher, eng.dims[0][0]
    dr = (eng.H[0][:n, :i0], eng.p_drop, eng.seed, st.offs[0], 2 * i0) if st.fold[0] else None
    if st.one_launch:       # (gist_extract_parts_desc.feat_intra: Z[0]'s right half comes with it)
        bt.prefetched = None
        hip.extract_parts(bt.g, b.ids, eng.n_max, b.parts[0], b.parts[1], b.parts[2], bt.rowptr[:n + 1], bt.col,
                          bt.t_rowptr[:n + 1], bt.t_col, bt.norm, bt.feat, eng.z0_left(n), bt.labels, bt.lab,
                          eng._extraction_scratch(), drop=dr, feat_intra=bt.feat_intra, ah=eng.Z[0][:n, i0:])
    else:
        bt.extract(b.ids, eng.z0_left(n), drop=dr)
    b.ready = True
    b.z0_dropped = dr is not None


def aggregate(eng, st, b, k):
    """Z_k's right half = A^ . (left half), and layer k's dropout over [h | ah] where no producer carries it."""
    n, i = b.n, eng.dims[k][0]
    z = eng.Z[k][:n]
    if k == 0 and (st.one_launch or b.ah_owner is eng):     # ah (and its mask when folded) came with the extraction
        if st.offs and not st.fold[0]:
            hip.dropout_(z, eng.p_drop, eng.seed, st.offs[0])
            b.ah_owner = None
    elif st.fold[k]:      # source = the undropped input, store = dropout(ah)
        hip.spmm_drop(b.rowptr, b.col, eng.H[k][:n, :i], z[:, i:], 1, eng.p_drop, eng.seed, st.offs[k] + i, 0, 2 * i,
                      out_scale=b.norm, row_blocks=b.row_blocks if st.blocked else None, prepared=st.prep_fwd)
    else:
        hip.spmm(b.rowptr, b.col, z[:, :i], z[:, i:], out_scale=b.norm, row_blocks=b.row_blocks, prepared=st.prep_fwd)
        if st.offs:
            hip.dropout_(z, eng.p_drop, eng.seed, st.offs[k])


def project_hidden(eng, st, b, k):
    """Y_k = Z_k . W_k^T + b_k, then LayerNorm + ReLU into the left half of Z_{k+1} -- with layer k + 1's dropout where
    it is folded there (the undropped rows go to H[k + 1])."""
    n, A = b.n, eng.arena
    i, o = eng.dims[k]
    i_next = eng.dims[k + 1][0]
    z, y, out = eng.Z[k][:n], eng.Y[k][:n], eng.Z[k + 1][:n, :i_next]
    rstd = eng.rstd[k][:n] if eng.use_layernorm else None
    fold = st.fold[k + 1]
    drop = ((eng.H[k + 1][:n, :i_next], eng.p_drop, eng.seed, st.offs[k + 1], 2 * i_next) if fold else
            (None, 0.0, eng.seed, 0, o))        # (out2, p, seed, offset, mask_ld) of the LayerNorm epilogue
    ys = fused_buffers(eng)['y'] if st.slabs else None
    if ys is not None and not hip.gemm_splits_own_operands(n, o, 2 * i):
        # the projection's k slices stay slabs; the LayerNorm sums them as it reads (gist_sage_step)
        ns = hip.gemm_slabs('nt', z, A.W[k], A.b[k], y, ys)
        if ns > 1:
            hip.ln_relu_fwd_slabs(y, ys, ns, A.b[k], out, drop[0], rstd, eng.use_layernorm, True, *drop[1:])
            return
    else:
        hip.gemm_nt(z, A.W[k], A.b[k], y)
    if fold:
        hip.ln_relu_fwd_drop(y, out, drop[0], rstd, eng.use_layernorm, True, *drop[1:])
    else:
        hip.ln_relu_fwd(y, out, rstd, eng.use_layernorm, True)


def project_class(eng, st, b):
    """The class layer's logits -- or nothing yet, when gist_sage_step's one launch for projection, CE, dZ and bias
    chunks takes them (st.cls_fused: loss() issues it), or split-K slabs for the loss kernel to sum (st.logit_slabs)."""
    n, A, k = b.n, eng.arena, eng.L1 - 1
    i, o = eng.dims[k]
    z = eng.Z[k][:n]
    if st.slabs:
        fb = fused_buffers(eng)
        if (fb['dw'][k] is not None and eng.ldc <= 64 and (not st.offs or st.offs[k] % 2 == 0) and
                int(hip.tuning('class_fused')) != 1 and hip.class_layer_takes(z, A.W[k], o) and
                fb['dw'][k].numel() >= _lib.load().gist_class_dw_slab_bytes(n, o, 2 * i)):
            st.cls_fused = True
            return
        if fb['logits'] is not None:
            st.logit_slabs = hip.gemm_slabs('nt', z, A.W[k], A.b[k], eng.Y[k][:n, :o], fb['logits'])
            return
    hip.gemm_nt(z, A.W[k], A.b[k], eng.Y[k][:n, :o])


def project_class_first(eng, b):
    """Inference, narrowing class layer (H -> C): [h | A^h] W^T = h W1^T + A^(h W2^T), so aggregate the C-wide
    projection, not the H-wide activations (full-graph evaluation: one D=4096 pass over 115 M edges becomes a D=41
    pass).  Same value up to fp32 summation order; training keeps the reference order: dropout acts on [h | A^h]."""
    n, A, k = b.n, eng.arena, eng.L1 - 1
    i, o = eng.dims[k]
    h, W = eng.Z[k][:n, :i], A.W[k]
    p_buf = eng.dlogits[:n, :o]                      # free in inference
    hip.gemm_nt(h, W[:, i:], None, p_buf)
    hip.gemm_nt(h, W[:, :i], A.b[k], eng.Y[k][:n, :o])
    hip.spmm(b.rowptr, b.col, p_buf, eng.Y[k][:n, :o], out_scale=b.norm, accumulate=True)


def forward(eng, b, training, _step=False):
    """SageEngine.forward: GCN.forward (modules.py:310-314) on the batch whose features already sit in
    Z[0][:, :F] (a lazy batch is extracted first).  Returns the logits view [n, C].
    _step: called by train_step -- the class layer's logits may stay split-K slabs for the loss
    kernel and a lazy batch's feature gather carries layer 0's dropout, like gist_sage_step."""
    st = eng._twin = decide(eng, b, training, _step)
    if not b.ready:
        extract(eng, st, b)
    # block structure of the batch, once for all its aggregations, where a kernel reads it (as gist_sage_step does)
    if st.blocked and any(hip.spmm_prepared_useful(eng.Z[k][:b.n, :i], eng.Z[k][:b.n, i:])
                          for k, (i, o) in enumerate(eng.dims)):
        st.prep_fwd = hip.spmm_prepare(b.rowptr, b.col, b.row_blocks)
        if training:
            st.prep_bwd = hip.spmm_prepare(b.t_rowptr, b.t_col, b.row_blocks)
    last = eng.L1 - 1
    for k in range(last):
        aggregate(eng, st, b, k)
        project_hidden(eng, st, b, k)
    if not training and eng.dims[last][1] < eng.dims[last][0]:
        project_class_first(eng, b)
    else:
        aggregate(eng, st, b, last)
        project_class(eng, st, b)
    return eng.logits(b.n)


# -- loss and backward ------------------------------------------------------------------------------------------------
def dz(eng, k, n):
    """dZ_k [n, 2 * in_k] = [dh | d(ah)] in the shared scratch; layer k - 1 reads the left half as its d_out."""
    i = eng.dims[k][0]
    return eng.dZ[:n * 2 * i].view(n, 2 * i)


def segment(eng, grad, src, ns):
    """adam_segments_'s (begin, end, source, stride, count): gradient `grad` = the sum of the `ns` pieces in `src`."""
    g = (grad.data_ptr() - eng.arena.grads.data_ptr()) // 4
    return (g, g + grad.numel(), src, grad.numel(), ns)


def reverse_aggregate(eng, st, b, k, masked):
    """dh_k += A^T . (norm . d(ah)_k); masked: layer k's dropout mask is applied to both halves here."""
    i = eng.dims[k][0]
    d = dz(eng, k, b.n)
    if masked:
        hip.spmm_drop(b.t_rowptr, b.t_col, d[:, i:], d[:, :i], 2, eng.p_drop, eng.seed, st.offs[k], st.offs[k] + i,
                      2 * i, src_scale=b.norm, accumulate=True, row_blocks=b.row_blocks, prepared=st.prep_bwd)
    else:
        hip.spmm(b.t_rowptr, b.t_col, d[:, i:], d[:, :i], src_scale=b.norm, accumulate=True, row_blocks=b.row_blocks,
                 prepared=st.prep_bwd)


def loss(eng, st, b, mask, count, fb):
    """CE and d_logits.  Deferred (fb), the rows' losses stay in row_loss for optimise(); with st.cls_fused the launch
    also forms the logits, the class layer's dZ and its bias chunk sums."""
    n, A, k = b.n, eng.arena, eng.L1 - 1
    if fb and st.cls_fused:
        hip.class_layer(eng.Z[k][:n], A.W[k], A.b[k], b.labels, n, eng.Y[k][:n, :eng.dims[k][1]], eng.dlogits[:n],
                        eng.row_loss[:n], dz(eng, k, n) if k > 0 else None, eng.p_drop if st.offs else 0.0, eng.seed,
                        st.offs[k] if st.offs else 0, fb['partials'][k])
    elif fb:
        hip.softmax_xent_slabs(eng.logits(n), fb['logits'], st.logit_slabs, A.b[-1], b.labels, None, n,
                               eng.row_loss[:n], None, eng.dlogits[:n])
    elif st.logit_slabs > 1:
        raise RuntimeError('gist_amd: masked loss after a slab forward')
    else:
        hip.softmax_xent(eng.logits(n), b.labels, mask, n if count is None else count, eng.row_loss[:n], eng.loss,
                         eng.dlogits[:n])


def backward_input(eng, st, b, k, dy, fb):
    """dZ_k = dY_k . W_k under layer k's dropout mask, unless the reverse aggregation applies it.  Returns (masked: the
    reverse aggregation must apply the mask, dual: dW_k came with the same launch)."""
    n, A, last = b.n, eng.arena, k == eng.L1 - 1
    i = eng.dims[k][0]
    z, d = eng.Z[k][:n], dz(eng, k, n)
    drop = bool(st.offs)
    masked = eng.fuse and drop and not last and hip.spmm_drop_takes(2, i, d[:, i:], d[:, :i], st.blocked)
    p = eng.p_drop if (drop and not masked) else 0.0
    off = st.offs[k] if drop else 0
    # gist_sage_step: dZ_k and dW_k of a narrow hidden layer in one launch (gist_gemm_nn_tn_dual_f32)
    if fb and not last and p == 0.0 and hip.gemm_dual_takes(dy, A.W[k], z, d):
        ns = hip.gemm_nn_tn_dual(dy, A.W[k], d, z, A.dW[k], fb['dw'][k])
        if ns > 1:
            st.segments.append(segment(eng, A.dW[k], fb['dw'][k], ns))
        return masked, True
    if fb and last:      # (db_k's chunk sums ride along; a hidden layer's came with its LayerNorm backward)
        hip.gemm_nn_dropout_colsum_(dy, A.W[k], d, p, eng.seed, off, fb['partials'][k])
    else:
        hip.gemm_nn_dropout_(dy, A.W[k], d, p, eng.seed, off)
    return masked, False


def backward_layer(eng, st, b, k, fb):
    """Layer k's backward: dY_k, dZ_k, dW_k, db_k and the reverse aggregation.  fb: the fused buffers when the
    gradients' last sums are deferred to optimise(), else None."""
    n, A, last = b.n, eng.arena, k == eng.L1 - 1
    z = eng.Z[k][:n]
    if last:
        dy = eng.dlogits[:n, :eng.dims[k][1]]
    else:       # d_out arrives in the left half of dZ_{k+1}; dY overwrites yhat; deferred, db_k's chunk sums ride along
        d_out, dy = dz(eng, k + 1, n)[:, :eng.dims[k + 1][0]], eng.Y[k][:n]
        rstd = eng.rstd[k][:n] if eng.use_layernorm else None
        if fb:
            hip.ln_relu_bwd_colsum(d_out, dy, rstd, dy, eng.use_layernorm, True, fb['partials'][k])
        else:
            hip.ln_relu_bwd(d_out, dy, rstd, dy, eng.use_layernorm, True)
    masked = dual = False
    if last and fb and st.cls_fused:     # (dZ and the bias chunk sums came with the loss)
        st.segments.append(segment(eng, A.dW[k], fb['dw'][k], hip.class_dw_slabs(dy, z, fb['dw'][k])))
    else:
        if k > 0:
            masked, dual = backward_input(eng, st, b, k, dy, fb)
        if not dual and fb and fb['dw'][k] is not None:
            ns = hip.gemm_slabs('tn', dy, z, None, A.dW[k], fb['dw'][k])
            if ns > 1:
                st.segments.append(segment(eng, A.dW[k], fb['dw'][k], ns))
        elif not dual:
            hip.gemm_tn(dy, z, A.dW[k])
        if fb and last and k == 0:       # (no launch left db's chunk sums)
            raise RuntimeError('gist_amd: one-layer models take the native step')
    if fb:
        st.segments.append(segment(eng, A.db[k], fb['partials'][k], int(_lib.load().gist_row_chunks16(n))))
    else:
        hip.colsum(dy, A.db[k], eng.partials)
    if k > 0:
        reverse_aggregate(eng, st, b, k, masked)


def loss_and_backward(eng, b, mask=None, count=None, _step=False):
    """SageEngine.loss_and_backward: CE (mean over masked rows) + full backward into the gradient arena.  With the
    fused sequence inside train_step (_step, eng.fuse, no mask) the bias gradients and split weight
    gradients are left in chunks / slabs for adam_step, like gist_sage_step does; called on its
    own, the gradient arena is complete on return."""
    st = eng._twin
    fb = fused_buffers(eng) if (eng.fuse and mask is None and _step) else None
    st.segments, st.loss_rows = [], (b.n if fb else 0)
    loss(eng, st, b, mask, count, fb)
    for k in range(eng.L1 - 1, -1, -1):
        backward_layer(eng, st, b, k, fb)
    return eng.loss


def optimise(eng, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
    """SageEngine.adam_step: Adam over the arena, in the launch that also sums what loss_and_backward deferred."""
    A, st = eng.arena, eng._twin
    A.step += 1
    if st.segments or st.loss_rows:
        n = st.loss_rows
        hip.adam_segments_(A.params, A.grads, A.exp_avg, A.exp_avg_sq, A.step, lr, st.segments,
                           row_loss=eng.row_loss[:n] if n else None, n_loss_rows=n, loss_count=n,
                           loss=eng.loss if n else None, beta1=betas[0], beta2=betas[1], eps=eps,
                           weight_decay=weight_decay)
        st.segments, st.loss_rows = [], 0
        return
    hip.adam_(A.params, A.grads, A.exp_avg, A.exp_avg_sq, A.step, lr, betas[0], betas[1], eps, weight_decay)
