// Native step driver of the GAT family: one C-ABI call issues a whole training iteration of gist_amd.modules.GAT
// (batch extraction -> per layer gemm_nt, scores, aggregate -> CE -> per layer backward_dst, backward_src, attn_grad,
// gemm_tn, gemm_nn -> Adam over the flat arena, with the next batch's extraction in the optimiser's grid) on one stream.
// No kernel of its own: it calls the entry points the op-level API exposes (gist_gat_*, gist_gemm_*, gist_softmax_xent_f32,
// gist_adam_*), in the order and with the leading dimensions, workspaces and edge order of the module path
// (gist_amd/ops.py gat_layer_fwd / gat_layer_bwd), so the two are bit-identical.  What it removes is everything between
// the launches: allocations, the head stacking and its gradient split, autograd nodes, per-tensor optimiser launches.
#include "step_host.h"

using namespace gist;

namespace {
// Does layer k concatenate its heads?  The next layer's input width says so: n_out_k = the head mean, heads_k * n_out_k
// (heads_k > 1) = the concatenation.  The last layer has one head, where the two coincide: the mean.
bool layer_cats(const gist_gat_step_plan *p, int k) {
    return k + 1 < p->n_layers && p->layer[k].heads > 1 && p->layer[k + 1].n_in != p->layer[k].n_out;
}
// columns of layer k's output, of its gradient and of G
int64_t out_width(const gist_gat_step_plan *p, int k) {
    return layer_cats(p, k) ? p->layer[k].heads * p->layer[k].n_out : p->layer[k].n_out;
}

// layer count and shapes only: what the size helpers and the step both need before they look at a pointer
bool shapes_ok(const gist_gat_step_plan *p) {
    if (p == nullptr || p->n_layers < 1 || p->n_layers > GIST_MAX_LAYERS || p->n_max <= 0 || p->n_max >= (1LL << 31))
        return false;
    for (int k = 0; k < p->n_layers; ++k) {
        const gist_gat_layer_desc &l = p->layer[k];
        if (l.n_in < 1 || l.n_out < 1 || l.heads < 1 || l.heads * l.n_out >= (1LL << 22) || l.n_in >= (1LL << 22))
            return false;
        if (k > 0 && l.n_in != p->layer[k - 1].n_out && l.n_in != p->layer[k - 1].heads * p->layer[k - 1].n_out)
            return false;
    }
    return true;
}

// the three projections of layer k on a batch of n rows as (m, n, k) of gist_gemm_{nt,tn,nn}_f32
struct GemmShape { int64_t m, n, k; };
void layer_gemms(const gist_gat_layer_desc &l, int64_t n, GemmShape (&g)[3]) {
    const int64_t hf = l.heads * l.n_out;
    g[0] = GemmShape{n, hf, l.n_in};      // Z = x . W^T
    g[1] = GemmShape{hf, l.n_in, n};      // dW = dZ^T . x
    g[2] = GemmShape{n, l.n_in, hf};      // dx = dZ . W
}
}  // namespace

// Bytes of gist_gat_step_plan.workspace: the largest gist_gemm_workspace_bytes over every projection of every layer and
// every batch size up to n_max (the split-K choice is not monotone in the row count).  Host function.
extern "C" int64_t gist_gat_step_workspace_bytes(const gist_gat_step_plan *p) {
    if (!shapes_ok(p)) return 0;
    int64_t need = 0;
    for (int k = 0; k < p->n_layers; ++k)
        for (int64_t n = 1; n <= p->n_max; ++n) {
            GemmShape g[3];
            layer_gemms(p->layer[k], n, g);
            for (int q = 0; q < (k > 0 ? 3 : 2); ++q) {
                const int64_t b = gist_gemm_workspace_bytes(g[q].m, g[q].n, g[q].k);
                need = b > need ? b : need;
            }
        }
    return need;
}

// Floats of gist_gat_step_plan.attn_partials: the widest layer's gist_gat_attn_grad_workspace_floats at n_max rows.
extern "C" int64_t gist_gat_step_attn_partials_floats(const gist_gat_step_plan *p) {
    if (!shapes_ok(p)) return 0;
    int64_t need = 0;
    for (int k = 0; k < p->n_layers; ++k) {
        const int64_t b = gist_gat_attn_grad_workspace_floats(p->n_max, p->layer[k].heads, p->layer[k].n_out);
        need = b > need ? b : need;
    }
    return need;
}

namespace {
// What one call runs.  gist_gat_step runs all of them (the forward alone without GIST_STEP_TRAIN); gist_gat_step_phase
// exactly one.  The extraction belongs to the forward.
enum { RUN_FORWARD = 1, RUN_BACKWARD = 2, RUN_OPTIMIZER = 4 };

// One call's decisions, made once by validate() before any device work and read by the phase functions.
struct Ws { void *p; int64_t bytes; };
struct Call {
    const gist_gat_step_plan *p;
    const int32_t *ids;
    int64_t n;
    int flags;
    bool by_parts;                     // the one-launch extraction (part tables) instead of gist_extract_batch
    Ws ws[GIST_MAX_LAYERS][3];         // split-K scratch of layer k's three projections (layer_gemms order)
    gist_stream_t s;
    hipStream_t st;
};

// Every check of what the parts `run` of an iteration read, all of it before any device work.  `who` names the entry
// point in the messages; phase_call: the flags are gist_gat_step_phase's (one phase bit, GIST_STEP_TRAIN).
int validate(const char *who, const gist_gat_step_plan *p, const int32_t *ids, int64_t n, int64_t adam_step, int flags,
             int run, bool phase_call, gist_stream_t s, Call &c) {
    GIST_REQUIRE(p != nullptr, "%s: null plan", who);
    GIST_REQUIRE(p->n_layers >= 1 && p->n_layers <= GIST_MAX_LAYERS, "%s: bad n_layers", who);
    GIST_REQUIRE(shapes_ok(p), "%s: bad layer shapes or n_max", who);
    GIST_REQUIRE(n > 0, "%s: empty batch", who);
    GIST_REQUIRE(n <= p->n_max, "%s: batch of %lld rows exceeds n_max = %lld", who, (long long)n, (long long)p->n_max);
    const int phases = GIST_STEP_PHASE_FORWARD | GIST_STEP_PHASE_BACKWARD | GIST_STEP_PHASE_OPTIMIZER;
    int known = GIST_STEP_EXTRACT | GIST_STEP_TRAIN | GIST_STEP_EXTRACT_NEXT | GIST_STEP_PREEXTRACTED;
    if (phase_call) {
        known |= phases | GIST_STEP_DLOGITS_GIVEN;
        const int ph = flags & phases;
        GIST_REQUIRE(ph != 0, "%s: no GIST_STEP_PHASE_* bit (the whole iteration in one call is gist_gat_step)", who);
        GIST_REQUIRE((ph & (ph - 1)) == 0, "%s: more than one GIST_STEP_PHASE_* bit (one phase per call)", who);
        GIST_REQUIRE(flags & GIST_STEP_TRAIN, "%s: a phase call needs GIST_STEP_TRAIN (forward only: gist_gat_step)", who);
        GIST_REQUIRE(!(flags & GIST_STEP_DLOGITS_GIVEN) || ph == GIST_STEP_PHASE_BACKWARD,
                     "%s: GIST_STEP_DLOGITS_GIVEN belongs to GIST_STEP_PHASE_BACKWARD", who);
    } else {
        GIST_REQUIRE(!(flags & (phases | GIST_STEP_DLOGITS_GIVEN)),
                     "%s: GIST_STEP_PHASE_* / GIST_STEP_DLOGITS_GIVEN are not supported (one call per iteration; the "
                     "phase calls are gist_gat_step_phase)", who);
    }
    GIST_REQUIRE((flags & ~known) == 0, "%s: unknown flag bits", who);
    GIST_REQUIRE(!((flags & GIST_STEP_EXTRACT) && (flags & GIST_STEP_PREEXTRACTED)),
                 "%s: GIST_STEP_EXTRACT and GIST_STEP_PREEXTRACTED exclude each other", who);
    const bool train = (flags & GIST_STEP_TRAIN) != 0;
    GIST_REQUIRE(!(flags & (GIST_STEP_EXTRACT_NEXT | GIST_STEP_PREEXTRACTED)) || train,
                 "%s: GIST_STEP_EXTRACT_NEXT / GIST_STEP_PREEXTRACTED belong to training steps", who);
    const int L = p->n_layers;
    const bool fwd = (run & RUN_FORWARD) != 0, bwd = (run & RUN_BACKWARD) != 0, opt = (run & RUN_OPTIMIZER) != 0;
    if (fwd || bwd)
        GIST_REQUIRE(p->x0 && p->rowptr && p->col && p->t_rowptr && p->t_col && p->labels && p->dlogits && p->row_loss &&
                         p->loss,
                     "%s: null batch / loss buffer", who);
    for (int k = 0; (fwd || bwd) && k < L; ++k) {
        const gist_gat_layer_desc &l = p->layer[k];
        GIST_REQUIRE(l.W && l.A && l.Z && l.out && l.s_src && l.s_dst && l.m && l.l, "%s: null buffer in layer %d", who, k);
        GIST_REQUIRE(!bwd || (l.dW && l.dA), "%s: null gradient view in layer %d", who, k);
    }
    if (bwd)
        GIST_REQUIRE(p->dZ && p->g && p->ds_dst && p->dd && p->ds_src && (L == 1 || (p->d_out[0] && p->d_out[1])),
                     "%s: null backward scratch", who);
    if (opt) {
        GIST_REQUIRE(p->params && p->grads && p->exp_avg && p->exp_avg_sq && p->n_params > 0, "%s: null arena", who);
        GIST_REQUIRE(adam_step >= 1, "%s: adam_step is 1-based", who);
    }
    if (bwd)
        GIST_REQUIRE(p->attn_partial_floats >= 0 && (p->attn_partials || p->attn_partial_floats == 0),
                     "%s: bad attn_partials", who);
    c.p = p; c.ids = ids; c.n = n; c.flags = flags; c.s = s; c.st = as_stream(s);
    c.by_parts = p->node_part && p->part_slot && p->extract_scratch && p->batch_index >= 0 &&
                 gist_extract_parts_supported(p->n_max) == 1;
    if (fwd && (flags & GIST_STEP_EXTRACT)) {
        GIST_REQUIRE(ids != nullptr, "%s: null ids", who);
        GIST_REQUIRE(p->g_rowptr && p->g_col && p->g_t_rowptr && p->g_t_col && p->feat && p->norm &&
                         p->ld_feat >= p->layer[0].n_in && p->col_capacity >= 0,
                     "%s: null / bad resident graph", who);
        GIST_REQUIRE(c.by_parts || p->remap != nullptr, "%s: extraction needs the part tables or remap", who);
    }
    if (opt && (flags & GIST_STEP_EXTRACT_NEXT))
        GIST_REQUIRE(p->node_part && p->part_slot && p->extract_scratch && p->next_ids && p->next_batch_index >= 0 &&
                         p->next_n > 0 && p->next_n <= p->n_max && gist_extract_parts_supported(p->n_max) == 1 &&
                         p->g_rowptr && p->g_col && p->g_t_rowptr && p->g_t_col && p->feat && p->norm && p->x0 &&
                         p->rowptr && p->col && p->t_rowptr && p->t_col && p->labels,
                     "%s: GIST_STEP_EXTRACT_NEXT needs the part tables, the scratch and next_*", who);
    // every projection gets what the op-level wrappers give it (the split-K choice depends on the bytes): nothing where
    // gist_gemm_workspace_bytes says 0, the plan's workspace otherwise
    for (int k = 0; k < L; ++k) {
        GemmShape g[3];
        layer_gemms(p->layer[k], n, g);
        for (int q = 0; q < 3; ++q) {
            const bool runs = q == 0 ? fwd : (bwd && (q == 1 || k > 0));      // (layer 0 has no dx projection)
            const int64_t need = runs ? gist_gemm_workspace_bytes(g[q].m, g[q].n, g[q].k) : 0;
            if (need > 0 && (p->workspace == nullptr || p->workspace_bytes < need)) {
                set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)p->workspace_bytes,
                          (long long)need);
                return GIST_ENOSPACE;
            }
            c.ws[k][q] = need > 0 ? Ws{p->workspace, p->workspace_bytes} : Ws{nullptr, 0};
        }
        if (bwd) {
            const int64_t need = gist_gat_attn_grad_workspace_floats(n, p->layer[k].heads, p->layer[k].n_out);
            if (need > p->attn_partial_floats) {
                set_error("%s: attn_partials too small (%lld < %lld floats)", who, (long long)p->attn_partial_floats,
                          (long long)need);
                return GIST_ENOSPACE;
            }
        }
    }
    return GIST_OK;
}

// ---- extraction ---------------------------------------------------------------------------------------
int extract(const Call &c) {
    const gist_gat_step_plan *p = c.p;
    if (!(c.flags & GIST_STEP_EXTRACT)) return GIST_OK;
    const gist_gat_layer_desc &l0 = p->layer[0];
    if (c.by_parts) {
        const gist_extract_parts_desc x = parts_desc(p, c.ids, c.n, p->batch_index, l0.n_in, p->x0, l0.n_in);
        GIST_TRY(gist_extract_parts_desc_batch(&x, c.s));
    } else {
        GIST_TRY(gist_extract_batch(p->g_rowptr, p->g_col, p->g_t_rowptr, p->g_t_col, c.ids, c.n, p->remap, p->rowptr,
                                    p->col, p->t_rowptr, p->t_col, p->col_capacity, p->norm, p->feat, p->ld_feat,
                                    l0.n_in, p->x0, l0.n_in, p->labels_all, p->labels, c.s));
    }
    return GIST_OK;
}

// ---- forward (modules.GAT.forward: h = F.elu(layer(g, h)) for every layer, the last included), then the mean CE over
// the batch rows and its gradient w.r.t. the logits ------------------------------------------------------
int forward(const Call &c) {
    const gist_gat_step_plan *p = c.p;
    const int64_t n = c.n;
    const int L = p->n_layers;
    for (int k = 0; k < L; ++k) {
        const gist_gat_layer_desc &l = p->layer[k];
        const int64_t hf = l.heads * l.n_out;
        const float *x = k == 0 ? p->x0 : p->layer[k - 1].out;      // (dense: out_width(k - 1) = n_in wide)
        {
            Scope sc(p->timer, 1, n, hf, l.n_in, c.st);
            GIST_TRY(gist_gemm_nt_f32(x, l.n_in, l.W, l.n_in, nullptr, l.Z, hf, n, hf, l.n_in, c.ws[k][0].p,
                                      c.ws[k][0].bytes, c.s));
        }
        GIST_TRY(gist_gat_scores_f32(l.Z, hf, l.A, n, l.heads, l.n_out, l.s_src, l.s_dst, c.s));
        Scope sc(p->timer, 0, n, n, hf, c.st);
        GIST_TRY((layer_cats(p, k) ? gist_gat_aggregate_cat_f32 : gist_gat_aggregate_f32)(
            p->rowptr, p->col, l.Z, hf, l.s_src, l.s_dst, n, l.heads, l.n_out, 1, l.out, out_width(p, k), l.m, l.l, c.s));
    }
    const gist_gat_layer_desc &last = p->layer[L - 1];
    return gist_softmax_xent_f32(last.out, last.n_out, p->labels, nullptr, n, p->row_loss, p->loss, p->dlogits,
                                 last.n_out, n, last.n_out, c.s);
}

// ---- backward (ops.py gat_layer_bwd, layer by layer from the last), from plan->dlogits: the forward's, or the caller's
// own (GIST_STEP_DLOGITS_GIVEN: for a GAT it is simply the last layer's d_out) --------------------------------
int backward(const Call &c) {
    const gist_gat_step_plan *p = c.p;
    const int64_t n = c.n;
    const float *d_out = p->dlogits;      // (the upstream gradient 1.0 of the module path's loss.backward() is exact)
    for (int k = p->n_layers - 1; k >= 0; --k) {
        const gist_gat_layer_desc &l = p->layer[k];
        const int64_t hf = l.heads * l.n_out;
        const float *x = k == 0 ? p->x0 : p->layer[k - 1].out;
        const bool cat = layer_cats(p, k);
        const int64_t ow = out_width(p, k);
        {
            Scope sc(p->timer, 0, n, n, hf, c.st);
            GIST_TRY((cat ? gist_gat_backward_dst_cat_f32 : gist_gat_backward_dst_f32)(
                p->rowptr, p->col, l.Z, hf, l.out, ow, d_out, ow, l.s_src, l.s_dst, l.m, l.l, n, l.heads, l.n_out, 1,
                p->g, ow, p->ds_dst, p->dd, c.s));
        }
        {
            Scope sc(p->timer, 0, n, n, hf, c.st);
            GIST_TRY((cat ? gist_gat_backward_src_cat_f32 : gist_gat_backward_src_f32)(
                p->t_rowptr, p->t_col, l.Z, hf, p->g, ow, l.A, l.s_src, l.s_dst, l.m, l.l, p->dd, p->ds_dst, n, l.heads,
                l.n_out, p->dZ, hf, p->ds_src, c.s));
        }
        GIST_TRY(gist_gat_attn_grad_f32(l.Z, hf, p->ds_src, p->ds_dst, n, l.heads, l.n_out, p->attn_partials,
                                        p->attn_partial_floats, l.dA, c.s));
        {
            Scope sc(p->timer, 1, hf, l.n_in, n, c.st);
            GIST_TRY(gist_gemm_tn_f32(p->dZ, hf, x, l.n_in, l.dW, l.n_in, hf, l.n_in, n, c.ws[k][1].p, c.ws[k][1].bytes,
                                      c.s));
        }
        if (k > 0) {      // (layer 0's input is the features: no gradient)
            float *dx = p->d_out[k & 1];
            Scope sc(p->timer, 1, n, l.n_in, hf, c.st);
            GIST_TRY(gist_gemm_nn_f32(p->dZ, hf, l.W, l.n_in, dx, l.n_in, n, l.n_in, hf, c.ws[k][2].p, c.ws[k][2].bytes,
                                      c.s));
            d_out = dx;
        }
    }
    return GIST_OK;
}

// ---- one optimiser launch over the arena; with EXTRACT_NEXT the next batch is extracted in its grid -----
int optimise(const Call &c, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t adam_step) {
    const gist_gat_step_plan *p = c.p;
    if (c.flags & GIST_STEP_EXTRACT_NEXT) {
        const gist_extract_parts_desc x = parts_desc(p, p->next_ids, p->next_n, p->next_batch_index, p->layer[0].n_in, p->x0,
                                                     p->layer[0].n_in);
        return gist_adam_segments_extract_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, lr, beta1,
                                              beta2, eps, weight_decay, adam_step, nullptr, 0, nullptr, 0, 0, nullptr,
                                              &x, c.s);
    }
    return gist_adam_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, lr, beta1, beta2, eps,
                         weight_decay, adam_step, c.s);
}
}  // namespace

extern "C" int gist_gat_step(const gist_gat_step_plan *p, const int32_t *ids, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int64_t adam_step, int flags,
                             gist_stream_t s) {
    const int run = (flags & GIST_STEP_TRAIN) ? RUN_FORWARD | RUN_BACKWARD | RUN_OPTIMIZER : RUN_FORWARD;
    Call c;
    GIST_TRY(validate("gist_gat_step", p, ids, n, adam_step, flags, run, false, s, c));
    ActiveTimer active(p->timer);
    GIST_TRY(extract(c));
    GIST_TRY(forward(c));
    if (!(run & RUN_BACKWARD)) return GIST_OK;
    GIST_TRY(backward(c));
    return optimise(c, lr, beta1, beta2, eps, weight_decay, adam_step);
}

// One third of gist_gat_step's iteration: the functions above, one phase per call (include/gist_hip.h).  No state is
// kept between the calls: the plan's buffers are the state, and the phase order is the caller's contract.
extern "C" int gist_gat_step_phase(const gist_gat_step_plan *p, const int32_t *ids, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int64_t adam_step, int flags,
                                   gist_stream_t s) {
    const int run = (flags & GIST_STEP_PHASE_FORWARD)    ? RUN_FORWARD
                    : (flags & GIST_STEP_PHASE_BACKWARD) ? RUN_BACKWARD
                                                         : RUN_OPTIMIZER;
    Call c;
    GIST_TRY(validate("gist_gat_step_phase", p, ids, n, adam_step, flags, run, true, s, c));
    ActiveTimer active(p->timer);
    if (run == RUN_FORWARD) {
        GIST_TRY(extract(c));
        return forward(c);
    }
    return run == RUN_BACKWARD ? backward(c) : optimise(c, lr, beta1, beta2, eps, weight_decay, adam_step);
}
