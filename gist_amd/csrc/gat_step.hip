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
    if (!plan_sizes_ok(p)) return false;
    for (int k = 0; k < p->n_layers; ++k) {
        const gist_gat_layer_desc &l = p->layer[k];
        if (l.n_in < 1 || l.n_out < 1 || l.heads < 1 || l.heads * l.n_out >= (1LL << 22) || l.n_in >= (1LL << 22))
            return false;
        if (k > 0 && l.n_in != p->layer[k - 1].n_out && l.n_in != p->layer[k - 1].heads * p->layer[k - 1].n_out)
            return false;
    }
    return true;
}

// the three projections of layer k on a batch of n rows
void layer_gemms(const gist_gat_layer_desc &l, int64_t n, GemmShape (&g)[3]) {
    const int64_t hf = l.heads * l.n_out;
    g[0] = GemmShape{n, hf, l.n_in};      // Z = x . W^T
    g[1] = GemmShape{hf, l.n_in, n};      // dW = dZ^T . x
    g[2] = GemmShape{n, l.n_in, hf};      // dx = dZ . W
}
}  // namespace

// Bytes of gist_gat_step_plan.workspace (step_host.h, step_workspace_bytes).  Host function.
extern "C" int64_t gist_gat_step_workspace_bytes(const gist_gat_step_plan *p) {
    return shapes_ok(p) ? step_workspace_bytes(p, layer_gemms) : 0;
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
    GIST_TRY(check_plan(who, p, shapes_ok(p), n));
    GIST_TRY(check_flags(who, flags, phase_call, phase_call ? "gist_gat_step" : "gist_gat_step_phase"));
    const int L = p->n_layers;
    const bool fwd = (run & RUN_FORWARD) != 0, bwd = (run & RUN_BACKWARD) != 0, opt = (run & RUN_OPTIMIZER) != 0;
    if (fwd || bwd) GIST_TRY(check_batch_buffers(who, p, p->x0 != nullptr));
    for (int k = 0; (fwd || bwd) && k < L; ++k) {
        const gist_gat_layer_desc &l = p->layer[k];
        GIST_REQUIRE(l.W && l.A && l.Z && l.out && l.s_src && l.s_dst && l.m && l.l, "%s: null buffer in layer %d", who, k);
        GIST_REQUIRE(!bwd || (l.dW && l.dA), "%s: null gradient view in layer %d", who, k);
    }
    if (bwd)
        GIST_REQUIRE(p->dZ && p->g && p->ds_dst && p->dd && p->ds_src && (L == 1 || (p->d_out[0] && p->d_out[1])),
                     "%s: null backward scratch", who);
    if (opt) GIST_TRY(check_arena(who, p, adam_step));
    if (bwd)
        GIST_REQUIRE(p->attn_partial_floats >= 0 && (p->attn_partials || p->attn_partial_floats == 0),
                     "%s: bad attn_partials", who);
    c.p = p; c.ids = ids; c.n = n; c.flags = flags; c.s = s; c.st = as_stream(s);
    c.by_parts = extracts_by_parts(p);
    if (fwd && (flags & GIST_STEP_EXTRACT))
        GIST_TRY(check_extract(who, p, ids, c.by_parts, p->norm && p->ld_feat >= p->layer[0].n_in, ""));
    if (opt && (flags & GIST_STEP_EXTRACT_NEXT))      // (it writes every batch buffer the next forward reads)
        GIST_TRY(check_extract_next(who, p, p->norm && p->x0 && p->rowptr && p->col && p->t_rowptr && p->t_col && p->labels));
    for (int k = 0; k < L; ++k) {
        GemmShape g[3];
        layer_gemms(p->layer[k], n, g);
        GIST_TRY(pick_workspaces(who, p, k, g, fwd, bwd, c.ws[k]));
        if (bwd)
            GIST_TRY(enough(who, "attn_partials", p->attn_partial_floats,
                            gist_gat_attn_grad_workspace_floats(n, p->layer[k].heads, p->layer[k].n_out), "floats"));
    }
    return GIST_OK;
}

// the features go to x0, dense
int extract(const Call &c) {
    const int64_t f = c.p->layer[0].n_in;
    return gist::extract(c.p, c.by_parts, c.flags, c.ids, c.n, f, c.p->x0, f, c.s);
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

// the optimiser launch; with GIST_STEP_EXTRACT_NEXT the next batch's features go to x0 as well
int optimise(const Call &c, const AdamHyper &a) {
    const int64_t f = c.p->layer[0].n_in;
    return gist::optimise(c.p, c.flags, f, c.p->x0, f, a, c.s);
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
    return optimise(c, AdamHyper{lr, beta1, beta2, eps, weight_decay, adam_step});
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
    return run == RUN_BACKWARD ? backward(c) : optimise(c, AdamHyper{lr, beta1, beta2, eps, weight_decay, adam_step});
}
