// Native step driver of the GraphSAGE family: one C-ABI call issues a whole training iteration of
// gist_amd.modules.GraphSAGE (cluster_gcn/modules.py:100-189): batch extraction -> per layer aggregation, dropout on
// [h | ah], gemm_nt, bias + LayerNorm with affine + ReLU -> CE -> per layer gemm_tn, gemm_nn under the mask, reverse
// aggregation, the tail's backward -> Adam over the flat arena, with the next batch's extraction in the optimiser's grid,
// on one stream.  No kernel of its own: it calls the entry points the op-level API exposes, so an op-by-op caller that
// issues the same sequence gets the same bits (tests/test_graphsage_step_gpu.py).  What it removes is everything between
// the launches: torch.cat, nn.Dropout's own pass, the transposed-weight copy, two custom-op dispatches per tail,
// autograd nodes and the per-tensor optimiser launches.
#include "step_host.h"

using namespace gist;

namespace {
constexpr float kLnEps = 1e-5f;      // nn.LayerNorm's default, modules.py:120

// layer count and shapes only: what the size helpers and the step both need before they look at a pointer
bool shapes_ok(const gist_graphsage_step_plan *p) {
    if (!plan_sizes_ok(p)) return false;
    for (int k = 0; k < p->n_layers; ++k) {
        const gist_graphsage_layer_desc &l = p->layer[k];
        if (l.n_in < 1 || l.n_out < 1 || l.n_in >= (1LL << 22) || l.n_out >= (1LL << 22)) return false;
        if (k > 0 && l.n_in != p->layer[k - 1].n_out) return false;
    }
    return true;
}

// the three projections of layer k on a batch of n rows
void layer_gemms(const gist_graphsage_layer_desc &l, int64_t n, GemmShape (&g)[3]) {
    g[0] = GemmShape{n, l.n_out, 2 * l.n_in};      // Y = Z . W^T
    g[1] = GemmShape{l.n_out, 2 * l.n_in, n};      // dW = dY^T . Z
    g[2] = GemmShape{n, 2 * l.n_in, l.n_out};      // dZ = dY . W
}

// Is layer k's dropout folded into its producers (the tail of layer k - 1, the aggregation of layer k)?
bool layer_folds(const gist_graphsage_step_plan *p, int k) {
    if (k < 1 || k >= p->n_layers || !(p->p_drop > 0.f)) return false;
    const gist_graphsage_layer_desc &l = p->layer[k];
    return l.H != nullptr && l.Z != nullptr &&
           gist_spmm_drop_takes(1, l.n_in, l.n_in, 2 * l.n_in, l.H, l.Z + l.n_in, p->row_blocks != nullptr) == 1;
}
}  // namespace

// Bytes of gist_graphsage_step_plan.workspace (step_host.h, step_workspace_bytes).  Host function.
extern "C" int64_t gist_graphsage_step_workspace_bytes(const gist_graphsage_step_plan *p) {
    return shapes_ok(p) ? step_workspace_bytes(p, layer_gemms) : 0;
}

// Floats of gist_graphsage_step_plan.ln_workspace: the widest hidden layer's gist_ln_affine_bwd_workspace_floats at
// n_max rows (0 for a model that is its output layer alone).
extern "C" int64_t gist_graphsage_step_ln_workspace_floats(const gist_graphsage_step_plan *p) {
    if (!shapes_ok(p)) return 0;
    int64_t need = 0;
    for (int k = 0; k + 1 < p->n_layers; ++k) {
        const int64_t b = gist_ln_affine_bwd_workspace_floats(p->n_max, p->layer[k].n_out);
        need = b > need ? b : need;
    }
    return need;
}

extern "C" int gist_graphsage_step_folds(const gist_graphsage_step_plan *p, int32_t k) {
    if (!shapes_ok(p) || k < 0 || k >= p->n_layers) return -1;
    return layer_folds(p, k) ? 1 : 0;
}

namespace {
// What one call runs.  gist_graphsage_step runs all of them (the forward alone without GIST_STEP_TRAIN);
// gist_graphsage_step_phase exactly one.  The extraction belongs to the forward.
enum { RUN_FORWARD = 1, RUN_BACKWARD = 2, RUN_OPTIMIZER = 4 };

// One call's decisions, made once by validate() before any device work and read by the phase functions.
struct Call {
    const gist_graphsage_step_plan *p;
    const int32_t *ids;
    int64_t n;
    int flags;
    bool train;
    bool by_parts;                     // the one-launch extraction (part tables) instead of gist_extract_batch
    bool layer0_aggregates;            // not under use_pp while training (modules.py:133)
    int64_t n_feat;                    // columns of the resident features the extraction gathers into Z_0
    float p_drop;                      // this call's dropout probability (0 without GIST_STEP_TRAIN)
    bool folds[GIST_MAX_LAYERS + 1];   // layer k's dropout is folded into its producers ([n_layers]: false)
    uint64_t offs[GIST_MAX_LAYERS];    // layer k's base in the dropout counter space
    Ws ws[GIST_MAX_LAYERS][3];         // split-K scratch of layer k's three projections (layer_gemms order)
    gist_stream_t s;
    hipStream_t st;
};

// Every check and every workspace decision of the parts `run` of an iteration, all of it before any device work.  `who`
// names the entry point in the messages; phase_call: the flags are gist_graphsage_step_phase's (one phase bit,
// GIST_STEP_TRAIN).  Each part checks what it reads: the forward the batch and loss buffers, the layers' W b Z Y (gamma
// beta yhat rstd), the EXTRACT inputs; the backward the gradient views and its scratch; the optimiser the arena and the
// EXTRACT_NEXT inputs.
int validate(const char *who, const gist_graphsage_step_plan *p, const int32_t *ids, int64_t n, uint64_t drop_offset,
             int64_t adam_step, int flags, int run, bool phase_call, gist_stream_t s, Call &c) {
    GIST_TRY(check_plan(who, p, shapes_ok(p), n));
    GIST_TRY(check_flags(who, flags, phase_call, phase_call ? "gist_graphsage_step" : "gist_graphsage_step_phase"));
    const bool train = (flags & GIST_STEP_TRAIN) != 0;
    const bool fwd = (run & RUN_FORWARD) != 0, bwd = (run & RUN_BACKWARD) != 0, opt = (run & RUN_OPTIMIZER) != 0;
    GIST_REQUIRE(p->p_drop >= 0.f && p->p_drop < 1.f, "%s: p_drop must be in [0,1)", who);
    const int L = p->n_layers;
    if (fwd || bwd) GIST_TRY(check_batch_buffers(who, p, p->norm != nullptr));
    for (int k = 0; (fwd || bwd) && k < L; ++k) {
        const gist_graphsage_layer_desc &l = p->layer[k];
        const bool hidden = k + 1 < L;
        GIST_REQUIRE(l.W && l.b && l.Z && l.Y, "%s: null buffer in layer %d", who, k);
        GIST_REQUIRE(!hidden || (l.gamma && l.beta && l.yhat && l.rstd), "%s: null LayerNorm buffer in layer %d", who, k);
        if (bwd) {
            GIST_REQUIRE(l.dW && l.db, "%s: null gradient view in layer %d", who, k);
            GIST_REQUIRE(!hidden || (l.dgamma && l.dbeta), "%s: null LayerNorm gradient view in layer %d", who, k);
        }
    }
    if (fwd)
        GIST_REQUIRE(p->loss_mask == nullptr || (p->loss_count > 0 && p->loss_count <= n),
                     "%s: loss_mask given but loss_count is not in 1 .. n", who);
    if (fwd || bwd)
        GIST_REQUIRE(p->row_blocks == nullptr || p->n_row_blocks > 0, "%s: row_blocks given but n_row_blocks <= 0", who);
    if (bwd) GIST_REQUIRE(p->partials && (L == 1 || p->dZ), "%s: null backward scratch", who);
    if (opt) GIST_TRY(check_arena(who, p, adam_step));
    if (bwd)
        GIST_REQUIRE(p->ln_workspace_floats >= 0 && (p->ln_workspace || p->ln_workspace_floats == 0),
                     "%s: bad ln_workspace", who);
    c.p = p; c.ids = ids; c.n = n; c.flags = flags; c.train = train; c.s = s; c.st = as_stream(s);
    c.p_drop = train ? p->p_drop : 0.f;
    c.layer0_aggregates = !(p->use_pp && train);
    const int64_t F = p->layer[0].n_in;
    c.n_feat = c.layer0_aggregates ? F : 2 * F;
    c.by_parts = extracts_by_parts(p);
    if (fwd && (flags & GIST_STEP_EXTRACT))
        GIST_TRY(check_extract(who, p, ids, c.by_parts, p->ld_feat >= c.n_feat,
                               " (with use_pp the features are 2 * n_in wide)"));
    // (the extraction in the optimiser's grid writes every batch buffer the next forward reads)
    if (opt && (flags & GIST_STEP_EXTRACT_NEXT))
        GIST_TRY(check_extract_next(who, p, p->ld_feat >= c.n_feat && p->layer[0].Z && p->norm && p->rowptr && p->col &&
                                                p->t_rowptr && p->t_col && p->labels));
    // the dropout counter space of this step and which layers fold their mask into their producers: from the plan
    // alone, so the forward and the backward phase of an iteration decide alike
    uint64_t off = drop_offset;
    for (int k = 0; k < L; ++k) {
        c.offs[k] = off;
        off += round_up2((uint64_t)n * 2 * p->layer[k].n_in);
        c.folds[k] = train && layer_folds(p, k);
    }
    c.folds[L] = false;
    for (int k = 0; k < L; ++k) {
        GemmShape g[3];
        layer_gemms(p->layer[k], n, g);
        GIST_TRY(pick_workspaces(who, p, k, g, fwd, bwd, c.ws[k]));
        if (bwd && k + 1 < L)
            GIST_TRY(enough(who, "ln_workspace", p->ln_workspace_floats,
                            gist_ln_affine_bwd_workspace_floats(n, p->layer[k].n_out), "floats"));
    }
    return GIST_OK;
}

// y (+)= out_scale . A . (src_scale . x) over the batch's graph (or its transpose), on the blocked entry when the plan
// carries row blocks
int aggregate(const Call &c, const int32_t *rowptr, const int32_t *col, const float *x, int64_t ldx, float *y,
              int64_t ldy, int64_t d, const float *out_scale, const float *src_scale, int accumulate) {
    const gist_graphsage_step_plan *p = c.p;
    Scope sc(p->timer, 0, c.n, c.n, d, c.st);
    if (p->row_blocks != nullptr)
        return gist_spmm_csr_blocked_f32(rowptr, col, x, ldx, y, ldy, c.n, d, out_scale, src_scale, accumulate,
                                         p->row_blocks, p->n_row_blocks, c.s);
    return gist_spmm_csr_f32(rowptr, col, x, ldx, y, ldy, c.n, d, out_scale, src_scale, accumulate, c.s);
}

// ---- forward (modules.py:133-147 per layer, :185-189), then the mean CE over the batch rows and its gradient ----
int forward(const Call &c) {
    const gist_graphsage_step_plan *p = c.p;
    const int64_t n = c.n;
    const int L = p->n_layers;
    for (int k = 0; k < L; ++k) {
        const gist_graphsage_layer_desc &l = p->layer[k];
        const int64_t in = l.n_in, ldz = 2 * in;
        if (c.folds[k]) {
            // the tail below wrote dropout(h) into Z_k's left half and h into H_k: ah from h, stored under its mask
            Scope sc(p->timer, 0, n, n, in, c.st);
            GIST_TRY(gist_spmm_csr_drop_f32(p->rowptr, p->col, l.H, in, l.Z + in, ldz, n, in, p->norm, nullptr, 0,
                                            p->row_blocks, p->n_row_blocks, 1, c.p_drop, p->seed, c.offs[k] + (uint64_t)in,
                                            0, ldz, c.s));
        } else {
            if (k > 0 || c.layer0_aggregates)
                GIST_TRY(aggregate(c, p->rowptr, p->col, l.Z, ldz, l.Z + in, ldz, in, p->norm, nullptr, 0));
            if (c.p_drop > 0.f) GIST_TRY(gist_dropout_f32(l.Z, ldz, n, ldz, c.p_drop, p->seed, c.offs[k], c.s));
        }
        const bool hidden = k + 1 < L;
        {
            Scope sc(p->timer, 1, n, l.n_out, ldz, c.st);
            GIST_TRY(gist_gemm_nt_f32(l.Z, ldz, l.W, ldz, hidden ? nullptr : l.b, l.Y, l.n_out, n, l.n_out, ldz,
                                      c.ws[k][0].p, c.ws[k][0].bytes, c.s));
        }
        if (!hidden) break;
        const gist_graphsage_layer_desc &nx = p->layer[k + 1];
        if (c.folds[k + 1])
            GIST_TRY(gist_ln_affine_fwd_drop_f32(l.Y, l.n_out, l.b, l.gamma, l.beta, l.yhat, l.n_out, nx.Z, 2 * nx.n_in,
                                                 nx.H, nx.n_in, l.rstd, n, l.n_out, 1, kLnEps, c.p_drop, p->seed,
                                                 c.offs[k + 1], 2 * nx.n_in, c.s));
        else
            GIST_TRY(gist_ln_affine_fwd_f32(l.Y, l.n_out, l.b, l.gamma, l.beta, l.yhat, l.n_out, nx.Z, 2 * nx.n_in,
                                            l.rstd, n, l.n_out, 1, kLnEps, c.s));
    }
    const gist_graphsage_layer_desc &last = p->layer[L - 1];
    return gist_softmax_xent_f32(last.Y, last.n_out, p->labels, p->loss_mask, p->loss_mask ? p->loss_count : n,
                                 p->row_loss, p->loss, p->dlogits, last.n_out, n, last.n_out, c.s);
}

// ---- backward, layer by layer from the last; dY of a hidden layer overwrites its Y ----
int backward(const Call &c) {
    const gist_graphsage_step_plan *p = c.p;
    const int64_t n = c.n;
    const int L = p->n_layers;
    for (int k = L - 1; k >= 0; --k) {
        const gist_graphsage_layer_desc &l = p->layer[k];
        const int64_t in = l.n_in, ldz = 2 * in;
        const float *dY = k == L - 1 ? p->dlogits : l.Y;
        {
            Scope sc(p->timer, 1, l.n_out, ldz, n, c.st);
            GIST_TRY(gist_gemm_tn_f32(dY, l.n_out, l.Z, ldz, l.dW, ldz, l.n_out, ldz, n, c.ws[k][1].p, c.ws[k][1].bytes,
                                      c.s));
        }
        if (k == L - 1) GIST_TRY(gist_colsum_f32(dY, l.n_out, n, l.n_out, p->partials, l.db, c.s));
        if (k == 0) break;      // (layer 0's input is the features: no gradient)
        {
            Scope sc(p->timer, 1, n, ldz, l.n_out, c.st);
            GIST_TRY(gist_gemm_nn_dropout_f32(dY, l.n_out, l.W, ldz, p->dZ, ldz, n, ldz, l.n_out, c.p_drop, p->seed,
                                              c.offs[k], c.ws[k][2].p, c.ws[k][2].bytes, c.s));
        }
        // d h += A^T (norm . d ah): the gradient of the aggregation, into the left half
        GIST_TRY(aggregate(c, p->t_rowptr, p->t_col, p->dZ + in, ldz, p->dZ, ldz, in, nullptr, p->norm, 1));
        const gist_graphsage_layer_desc &lo = p->layer[k - 1];
        GIST_TRY(gist_ln_affine_bwd_f32(p->dZ, ldz, lo.yhat, lo.n_out, lo.rstd, lo.gamma, lo.beta, 1, lo.Y, lo.n_out,
                                        lo.dgamma, lo.dbeta, lo.db, n, lo.n_out, p->ln_workspace,
                                        p->ln_workspace_floats, c.s));
    }
    return GIST_OK;
}

// the features into Z_0's left half, or (use_pp while training) [X | A^X] into all of it
int extract(const Call &c) {
    return gist::extract(c.p, c.by_parts, c.flags, c.ids, c.n, c.n_feat, c.p->layer[0].Z, 2 * c.p->layer[0].n_in, c.s);
}

// the optimiser launch; with GIST_STEP_EXTRACT_NEXT the next batch's features go to Z_0 as well
int optimise(const Call &c, const AdamHyper &a) {
    return gist::optimise(c.p, c.flags, c.n_feat, c.p->layer[0].Z, 2 * c.p->layer[0].n_in, a, c.s);
}
}  // namespace

extern "C" int gist_graphsage_step(const gist_graphsage_step_plan *p, const int32_t *ids, int64_t n,
                                   uint64_t drop_offset, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int64_t adam_step, int flags, gist_stream_t s) {
    const int run = (flags & GIST_STEP_TRAIN) ? RUN_FORWARD | RUN_BACKWARD | RUN_OPTIMIZER : RUN_FORWARD;
    Call c;
    GIST_TRY(validate("gist_graphsage_step", p, ids, n, drop_offset, adam_step, flags, run, false, s, c));
    ActiveTimer active(p->timer);
    GIST_TRY(extract(c));
    GIST_TRY(forward(c));
    if (!(run & RUN_BACKWARD)) return GIST_OK;
    GIST_TRY(backward(c));
    return optimise(c, AdamHyper{lr, beta1, beta2, eps, weight_decay, adam_step});
}

// One third of gist_graphsage_step's iteration: the functions above, one phase per call (include/gist_hip.h).  No state
// is kept between the calls: the plan's buffers are the state, and the phase order is the caller's contract.  The
// forward and the backward phase of an iteration get the same drop_offset (the backward's gist_gemm_nn_dropout_f32
// re-derives the masks); the optimiser phase reads none.
extern "C" int gist_graphsage_step_phase(const gist_graphsage_step_plan *p, const int32_t *ids, int64_t n,
                                         uint64_t drop_offset, float lr, float beta1, float beta2, float eps,
                                         float weight_decay, int64_t adam_step, int flags, gist_stream_t s) {
    const int run = (flags & GIST_STEP_PHASE_FORWARD)    ? RUN_FORWARD
                    : (flags & GIST_STEP_PHASE_BACKWARD) ? RUN_BACKWARD
                                                         : RUN_OPTIMIZER;
    Call c;
    GIST_TRY(validate("gist_graphsage_step_phase", p, ids, n, drop_offset, adam_step, flags, run, true, s, c));
    ActiveTimer active(p->timer);
    if (run == RUN_FORWARD) {
        GIST_TRY(extract(c));
        return forward(c);
    }
    return run == RUN_BACKWARD ? backward(c) : optimise(c, AdamHyper{lr, beta1, beta2, eps, weight_decay, adam_step});
}
