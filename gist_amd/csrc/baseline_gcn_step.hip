// Native step driver of the BaselineGCN family: one C-ABI call issues a whole training iteration of
// gist_amd.modules.BaselineGCN (cluster_gcn/modules.py:316-349, the plain GCN of GraphConv layers): batch extraction ->
// the two degree scales -> per layer the normalised aggregation and the projection in GraphConv's order, bias + ReLU +
// whole-tensor LayerNorm + the next layer's dropout -> CE -> per layer the tail's backward, the weight gradient and the
// input gradient in the reverse order -> Adam over the flat arena, with the next batch's extraction in the optimiser's
// grid, on one stream.  No kernel of its own: it calls the entry points the op-level API exposes, so an op-by-op caller
// that issues the same sequence gets the same bits (tests/test_baseline_gcn_step_gpu.py).  What it removes is everything
// between the launches: the eight torch launches of the degree scales, the custom-op dispatches, autograd nodes and the
// per-tensor optimiser launches.
#include "step_host.h"

using namespace gist;

namespace {
constexpr float kLnEps = 1e-5f;      // F.layer_norm's default, modules.py:348

// layer count and shapes only: what the size helpers and the step both need before they look at a pointer
bool shapes_ok(const gist_baseline_gcn_step_plan *p) {
    if (!plan_sizes_ok(p)) return false;
    for (int k = 0; k < p->n_layers; ++k) {
        const gist_baseline_gcn_layer_desc &l = p->layer[k];
        if (l.n_in < 1 || l.n_out < 1 || l.n_in >= (1LL << 22) || l.n_out >= (1LL << 22)) return false;
        if (k > 0 && l.n_in != p->layer[k - 1].n_out) return false;
    }
    return true;
}

// GraphConv's order (dgl_compat/nn/pytorch.py: `if self._in_feats > self._out_feats`)
bool multiplies_first(const gist_baseline_gcn_layer_desc &l) { return l.n_in > l.n_out; }

// the three projections of layer k on a batch of n rows: the same (m, n, k) in either order
void layer_gemms(const gist_baseline_gcn_layer_desc &l, int64_t n, GemmShape (&g)[3]) {
    g[0] = GemmShape{n, l.n_out, l.n_in};      // Y = T . W   or  T = X . W
    g[1] = GemmShape{l.n_in, l.n_out, n};      // dW = T^T . dY  or  X^T . dT
    g[2] = GemmShape{n, l.n_in, l.n_out};      // dT = dY . W^T  or  dX = dT . W^T
}

// floats of tail_ws a batch of n rows asks for: the forward's statistics partials and the backward's scratch
int64_t tail_ws_need(const gist_baseline_gcn_step_plan *p, int64_t n) {
    int64_t need = 0;
    for (int k = 0; k + 1 < p->n_layers; ++k) {
        const int64_t f = gist_ln_all_partials(n * p->layer[k].n_out);
        const int64_t b = gist_gcn_tail_bwd_workspace_floats(n, p->layer[k].n_out);
        need = f > need ? f : need;
        need = b > need ? b : need;
    }
    return need;
}
}  // namespace

// Bytes of gist_baseline_gcn_step_plan.workspace (step_host.h, step_workspace_bytes).  Host function.
extern "C" int64_t gist_baseline_gcn_step_workspace_bytes(const gist_baseline_gcn_step_plan *p) {
    return shapes_ok(p) ? step_workspace_bytes(p, layer_gemms) : 0;
}

// Floats of gist_baseline_gcn_step_plan.tail_ws (both of its sizes grow with the row count: n_max is the largest).
extern "C" int64_t gist_baseline_gcn_step_tail_ws_floats(const gist_baseline_gcn_step_plan *p) {
    return shapes_ok(p) ? tail_ws_need(p, p->n_max) : 0;
}

namespace {
// One call's decisions, made once by validate() before any device work and read by the phase functions.
struct Call {
    const gist_baseline_gcn_step_plan *p;
    const int32_t *ids;
    int64_t n;
    int flags;
    bool train;
    bool by_parts;                     // the one-launch extraction (part tables) instead of gist_extract_batch
    bool norm;                         // the hidden layers' whole-tensor LayerNorm
    float p_drop;                      // this call's dropout probability (0 without GIST_STEP_TRAIN)
    uint64_t offs[GIST_MAX_LAYERS];    // hidden layer k's base in the dropout counter space
    float *yhat[GIST_MAX_LAYERS];      // hidden layer k's yhat: its own buffer, X_{k+1} itself at p = 0, NULL without norm
    Ws ws[GIST_MAX_LAYERS][3];         // split-K scratch of layer k's three projections (layer_gemms order)
    gist_stream_t s;
    hipStream_t st;
};

// Every check and every workspace decision of an iteration, all of it before any device work.
int validate(const char *who, const gist_baseline_gcn_step_plan *p, const int32_t *ids, int64_t n, uint64_t drop_offset,
             int64_t adam_step, int flags, gist_stream_t s, Call &c) {
    GIST_TRY(check_plan(who, p, shapes_ok(p), n));
    GIST_TRY(check_flags(who, flags, false, nullptr));
    const bool train = (flags & GIST_STEP_TRAIN) != 0;
    GIST_REQUIRE(p->p_drop >= 0.f && p->p_drop < 1.f, "%s: p_drop must be in [0,1)", who);
    const int L = p->n_layers;
    c.p = p; c.ids = ids; c.n = n; c.flags = flags; c.train = train; c.s = s; c.st = as_stream(s);
    c.p_drop = train ? p->p_drop : 0.f;
    c.norm = p->use_layernorm != 0;
    GIST_TRY(check_batch_buffers(who, p, p->nd && p->ns && p->logits));
    for (int k = 0; k < L; ++k) {
        const gist_baseline_gcn_layer_desc &l = p->layer[k];
        const bool hidden = k + 1 < L;
        GIST_REQUIRE(l.W && l.b && l.X && l.T && l.Y, "%s: null buffer in layer %d", who, k);
        GIST_REQUIRE(!(hidden && c.norm) || (l.stats && (c.p_drop == 0.f || l.yhat)),
                     "%s: null LayerNorm buffer in layer %d", who, k);
        if (train) GIST_REQUIRE(l.dW && l.db, "%s: null gradient view in layer %d", who, k);
        // at p = 0 the tail's result IS yhat: stored once, in the next layer's input
        c.yhat[k] = !(hidden && c.norm) ? nullptr : (c.p_drop > 0.f ? l.yhat : p->layer[k + 1].X);
    }
    GIST_REQUIRE(p->loss_mask == nullptr || (p->loss_count > 0 && p->loss_count <= n),
                 "%s: loss_mask given but loss_count is not in 1 .. n", who);
    GIST_REQUIRE(p->row_blocks == nullptr || p->n_row_blocks > 0, "%s: row_blocks given but n_row_blocks <= 0", who);
    // the backward buffers: every model but one aggregate-first layer alone writes at least one of them
    const bool bwd_bufs = L > 1 || multiplies_first(p->layer[0]);
    if (train) GIST_REQUIRE(p->partials && (!bwd_bufs || (p->bwd[0] && p->bwd[1])), "%s: null backward scratch", who);
    if (train) GIST_TRY(check_arena(who, p, adam_step));
    GIST_REQUIRE(p->tail_ws_floats >= 0 && (p->tail_ws || p->tail_ws_floats == 0) && aligned8(p->tail_ws),
                 "%s: bad tail_ws", who);
    c.by_parts = extracts_by_parts(p);
    const int64_t F = p->layer[0].n_in;
    if (flags & GIST_STEP_EXTRACT) GIST_TRY(check_extract(who, p, ids, c.by_parts, p->ld_feat >= F && p->norm, ""));
    if (flags & GIST_STEP_EXTRACT_NEXT) GIST_TRY(check_extract_next(who, p, p->ld_feat >= F && p->norm));
    // the dropout counter space of this step: the hidden layers' results, as autograd.gcn_tail numbers them
    uint64_t off = drop_offset;
    for (int k = 0; k < L; ++k) {
        c.offs[k] = off;
        if (k + 1 < L) off += round_up2((uint64_t)n * p->layer[k].n_out);
    }
    for (int k = 0; k < L; ++k) {
        GemmShape g[3];
        layer_gemms(p->layer[k], n, g);
        GIST_TRY(pick_workspaces(who, p, k, g, true, train, c.ws[k]));
    }
    // the forward's partials only under the norm; the backward's chunk sums always
    int64_t need = 0;
    for (int k = 0; k + 1 < L; ++k) {
        const int64_t f = c.norm ? gist_ln_all_partials(n * p->layer[k].n_out) : 0;
        const int64_t b = train ? gist_gcn_tail_bwd_workspace_floats(n, p->layer[k].n_out) : 0;
        need = f > need ? f : need;
        need = b > need ? b : need;
    }
    return enough(who, "tail_ws", p->tail_ws ? p->tail_ws_floats : 0, need, "floats");
}

// y = out_scale . A . (src_scale . x) over the batch's graph (or its transpose), dense [n, d] both, on the blocked entry
// when the plan carries row blocks
int aggregate(const Call &c, const int32_t *rowptr, const int32_t *col, const float *x, float *y, int64_t d,
              const float *out_scale, const float *src_scale) {
    const gist_baseline_gcn_step_plan *p = c.p;
    Scope sc(p->timer, 0, c.n, c.n, d, c.st);
    if (p->row_blocks != nullptr)
        return gist_spmm_csr_blocked_f32(rowptr, col, x, d, y, d, c.n, d, out_scale, src_scale, 0, p->row_blocks,
                                         p->n_row_blocks, c.s);
    return gist_spmm_csr_f32(rowptr, col, x, d, y, d, c.n, d, out_scale, src_scale, 0, c.s);
}

// ---- forward (modules.py:343-348 per layer), then the mean CE over the batch rows and its gradient ----
int forward(const Call &c) {
    const gist_baseline_gcn_step_plan *p = c.p;
    const int64_t n = c.n;
    const int L = p->n_layers;
    GIST_TRY(gist_gcn_degree_scales_f32(p->rowptr, p->t_rowptr, n, p->nd, p->ns, c.s));
    for (int k = 0; k < L; ++k) {
        const gist_baseline_gcn_layer_desc &l = p->layer[k];
        const int64_t in = l.n_in, out = l.n_out;
        if (multiplies_first(l)) {
            {
                Scope sc(p->timer, 1, n, out, in, c.st);
                GIST_TRY(gist_gemm_nn_f32(l.X, in, l.W, out, l.T, out, n, out, in, c.ws[k][0].p, c.ws[k][0].bytes, c.s));
            }
            GIST_TRY(aggregate(c, p->rowptr, p->col, l.T, l.Y, out, p->nd, p->ns));
        } else {
            GIST_TRY(aggregate(c, p->rowptr, p->col, l.X, l.T, in, p->nd, p->ns));
            Scope sc(p->timer, 1, n, out, in, c.st);
            GIST_TRY(gist_gemm_nn_f32(l.T, in, l.W, out, l.Y, out, n, out, in, c.ws[k][0].p, c.ws[k][0].bytes, c.s));
        }
        if (k + 1 == L) {
            GIST_TRY(gist_gcn_tail_fwd_f32(l.Y, l.b, nullptr, p->logits, nullptr, n, out, 0, 0, kLnEps, 0.f, p->seed, 0,
                                           nullptr, c.s));
            break;
        }
        float *x_next = p->layer[k + 1].X;
        // yhat == x_next (the norm at p = 0): one store serves both, `out` stays NULL
        GIST_TRY(gist_gcn_tail_fwd_f32(l.Y, l.b, c.yhat[k], c.yhat[k] == x_next ? nullptr : x_next, l.stats, n, out, 1,
                                       c.norm ? 1 : 0, kLnEps, c.p_drop, p->seed, c.offs[k], c.norm ? p->tail_ws : nullptr,
                                       c.s));
    }
    const int64_t C = p->layer[L - 1].n_out;
    return gist_softmax_xent_f32(p->logits, C, p->labels, p->loss_mask, p->loss_mask ? p->loss_count : n, p->row_loss,
                                 p->loss, p->dlogits, C, n, C, c.s);
}

// ---- backward, layer by layer from the last.  dY of the output layer is dlogits; a hidden layer's is written by its
// tail's backward into one ping-pong buffer while the other holds dX_{k+1}, its d_out: bwd[a] = dY, bwd[1 - a] = dT,
// then dX over the dead dY ----
int backward(const Call &c) {
    const gist_baseline_gcn_step_plan *p = c.p;
    const int64_t n = c.n;
    const int L = p->n_layers;
    int a = 0;                          // bwd[a]: where this layer's dY lies (hidden layers) and its dX goes
    const float *dY = p->dlogits;
    for (int k = L - 1; k >= 0; --k) {
        const gist_baseline_gcn_layer_desc &l = p->layer[k];
        const int64_t in = l.n_in, out = l.n_out;
        if (k == L - 1) GIST_TRY(gist_colsum_f32(dY, out, n, out, p->partials, l.db, c.s));
        float *dT = p->bwd[1 - a], *dX = p->bwd[a];
        if (multiplies_first(l)) {
            // dT = A^^T dY (also for layer 0: dW needs it), dW = X^T dT, dX = dT W^T
            GIST_TRY(aggregate(c, p->t_rowptr, p->t_col, dY, dT, out, p->ns, p->nd));
            {
                Scope sc(p->timer, 1, in, out, n, c.st);
                GIST_TRY(gist_gemm_tn_f32(l.X, in, dT, out, l.dW, out, in, out, n, c.ws[k][1].p, c.ws[k][1].bytes, c.s));
            }
            if (k == 0) break;      // (layer 0's input is the features: no gradient)
            Scope sc(p->timer, 1, n, in, out, c.st);
            GIST_TRY(gist_gemm_nt_f32(dT, out, l.W, out, nullptr, dX, in, n, in, out, c.ws[k][2].p, c.ws[k][2].bytes,
                                      c.s));
        } else {
            // dW = T^T dY, dT = dY W^T, dX = A^^T dT
            {
                Scope sc(p->timer, 1, in, out, n, c.st);
                GIST_TRY(gist_gemm_tn_f32(l.T, in, dY, out, l.dW, out, in, out, n, c.ws[k][1].p, c.ws[k][1].bytes, c.s));
            }
            if (k == 0) break;
            {
                Scope sc(p->timer, 1, n, in, out, c.st);
                GIST_TRY(gist_gemm_nt_f32(dY, out, l.W, out, nullptr, dT, in, n, in, out, c.ws[k][2].p,
                                          c.ws[k][2].bytes, c.s));
            }
            GIST_TRY(aggregate(c, p->t_rowptr, p->t_col, dT, dX, in, p->ns, p->nd));
        }
        // the tail of layer k - 1: d_out = dX (= the gradient of X_k), dx = dY_{k-1} over the dead dT
        const gist_baseline_gcn_layer_desc &lo = p->layer[k - 1];
        GIST_TRY(gist_gcn_tail_bwd_f32(dX, lo.Y, lo.b, c.yhat[k - 1], lo.stats, dT, lo.db, n, lo.n_out, 1, c.norm ? 1 : 0,
                                       c.p_drop, p->seed, c.offs[k - 1], p->tail_ws, p->tail_ws_floats, c.s));
        dY = dT;
        a = 1 - a;
    }
    return GIST_OK;
}

// the features into X_0
int extract(const Call &c) {
    const int64_t F = c.p->layer[0].n_in;
    return gist::extract(c.p, c.by_parts, c.flags, c.ids, c.n, F, c.p->layer[0].X, F, c.s);
}

// the optimiser launch; with GIST_STEP_EXTRACT_NEXT the next batch's features go to X_0 as well
int optimise(const Call &c, const AdamHyper &a) {
    const int64_t F = c.p->layer[0].n_in;
    return gist::optimise(c.p, c.flags, F, c.p->layer[0].X, F, a, c.s);
}
}  // namespace

extern "C" int gist_baseline_gcn_step(const gist_baseline_gcn_step_plan *p, const int32_t *ids, int64_t n,
                                      uint64_t drop_offset, float lr, float beta1, float beta2, float eps,
                                      float weight_decay, int64_t adam_step, int flags, gist_stream_t s) {
    Call c;
    GIST_TRY(validate("gist_baseline_gcn_step", p, ids, n, drop_offset, adam_step, flags, s, c));
    ActiveTimer active(p->timer);
    GIST_TRY(extract(c));
    GIST_TRY(forward(c));
    if (!c.train) return GIST_OK;
    GIST_TRY(backward(c));
    return optimise(c, AdamHyper{lr, beta1, beta2, eps, weight_decay, adam_step});
}
