// Host-side helpers of the native step drivers.  All three (step.hip: the SAGE GCN, gat_step.hip: GAT, graphsage_step.hip:
// GraphSAGE) share the timer scopes, parts_desc and round_up2; the two with no kernel of their own also everything their
// plans, which name these fields alike, and their calls have in common: the checks, the projections' split-K scratch,
// the extraction and the optimiser launch.  What only one family has stays in its driver.
#pragma once
#include "common.h"

#define GIST_TRY(expr)            \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != GIST_OK) return rc_; \
    } while (0)

namespace gist {
struct Scope {   // records start now, stop at scope exit
    gist_timer *t; int64_t slot; hipStream_t s;
    Scope(gist_timer *t_, int kind, int64_t m, int64_t n, int64_t k, hipStream_t s_)
        : t(t_), slot(timer_begin(t_, kind, m, n, k, s_)), s(s_) {}
    ~Scope() { timer_end(t, slot, s); }
};
struct ActiveTimer {   // kernels below the entry points see the armed timer for this call only
    explicit ActiveTimer(gist_timer *t) { tl_timer = t; }
    ~ActiveTimer() { tl_timer = nullptr; }
};

// a dropout call's share of the counter space: its element count, rounded up to even
inline uint64_t round_up2(uint64_t x) { return x + (x & 1ULL); }

// The one-launch extraction (gist_extract_parts_desc_batch) of batch `batch` = `ids[0..n)` from a step plan's resident
// graph and part tables into its batch buffers: features to z0[n][n_feat] (ld ldz0).  What only one family has (the
// dropout fold, the aggregating gather) stays zero for its caller to fill.
template <class Plan>
gist_extract_parts_desc parts_desc(const Plan *p, const int32_t *ids, int64_t n, int32_t batch, int64_t n_feat,
                                   float *z0, int64_t ldz0) {
    gist_extract_parts_desc x{};
    x.g_rowptr = p->g_rowptr; x.g_col = p->g_col; x.g_t_rowptr = p->g_t_rowptr; x.g_t_col = p->g_t_col;
    x.ids = ids; x.n = n; x.n_max = p->n_max;
    x.node_part = p->node_part; x.part_slot = p->part_slot; x.batch = batch;
    x.rowptr = p->rowptr; x.col = p->col; x.t_rowptr = p->t_rowptr; x.t_col = p->t_col;
    x.col_capacity = p->col_capacity; x.norm = p->norm;
    x.feat = p->feat; x.ld_feat = p->ld_feat; x.n_feat = n_feat; x.z0 = z0; x.ldz0 = ldz0;
    x.labels_all = p->labels_all; x.labels = p->labels;
    x.scratch = p->extract_scratch;
    return x;
}

// ---- the drivers with no kernel of their own ------------------------------------------------------------
// A projection as (m, n, k) of gist_gemm_{nt,tn,nn}_f32.  A layer has three, in this order: its forward product, its
// weight gradient, its input gradient (which layer 0, whose input is the features, does not have).
struct GemmShape { int64_t m, n, k; };
// the split-K scratch a projection is given: nothing where gist_gemm_workspace_bytes says 0, the plan's otherwise
struct Ws { void *p; int64_t bytes; };

// the part of a plan's shape check that is no family's own
template <class Plan>
bool plan_sizes_ok(const Plan *p) {
    return p != nullptr && p->n_layers >= 1 && p->n_layers <= GIST_MAX_LAYERS && p->n_max > 0 && p->n_max < (1LL << 31);
}

// Bytes of a plan's workspace: the largest gist_gemm_workspace_bytes over every projection of every layer and every batch
// size up to n_max (the split-K choice is not monotone in the row count).  layer_gemms(layer, n, g) fills a layer's three.
template <class Plan, class LayerGemms>
int64_t step_workspace_bytes(const Plan *p, LayerGemms layer_gemms) {
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

// The first checks of a call.  shapes_ok: the family's own shape check of p (false for a null plan).
template <class Plan>
int check_plan(const char *who, const Plan *p, bool shapes_ok, int64_t n) {
    GIST_REQUIRE(p != nullptr, "%s: null plan", who);
    GIST_REQUIRE(p->n_layers >= 1 && p->n_layers <= GIST_MAX_LAYERS, "%s: bad n_layers (1 .. GIST_MAX_LAYERS = %d)", who,
                 GIST_MAX_LAYERS);
    GIST_REQUIRE(shapes_ok, "%s: bad layer shapes (a layer's n_in must follow from its predecessor's n_out) or n_max", who);
    GIST_REQUIRE(n > 0, "%s: empty batch", who);
    GIST_REQUIRE(n <= p->n_max, "%s: batch of %lld rows exceeds n_max = %lld", who, (long long)n, (long long)p->n_max);
    return GIST_OK;
}

// The flags of a one-call step, or (phase_call) of a phase call: one phase bit and GIST_STEP_TRAIN.  other: the family's
// other entry point, the phase call's for a one-call step (nullptr: the family has none) and the other way round.
inline int check_flags(const char *who, int flags, bool phase_call, const char *other) {
    const int phases = GIST_STEP_PHASE_FORWARD | GIST_STEP_PHASE_BACKWARD | GIST_STEP_PHASE_OPTIMIZER;
    int known = GIST_STEP_EXTRACT | GIST_STEP_TRAIN | GIST_STEP_EXTRACT_NEXT | GIST_STEP_PREEXTRACTED;
    if (phase_call) {
        known |= phases | GIST_STEP_DLOGITS_GIVEN;
        const int ph = flags & phases;
        GIST_REQUIRE(ph != 0, "%s: no GIST_STEP_PHASE_* bit (the whole iteration in one call is %s)", who, other);
        GIST_REQUIRE((ph & (ph - 1)) == 0, "%s: more than one GIST_STEP_PHASE_* bit (one phase per call)", who);
        GIST_REQUIRE(flags & GIST_STEP_TRAIN, "%s: a phase call needs GIST_STEP_TRAIN (forward only: %s)", who, other);
        GIST_REQUIRE(!(flags & GIST_STEP_DLOGITS_GIVEN) || ph == GIST_STEP_PHASE_BACKWARD,
                     "%s: GIST_STEP_DLOGITS_GIVEN belongs to GIST_STEP_PHASE_BACKWARD", who);
    } else {
        GIST_REQUIRE(!(flags & (phases | GIST_STEP_DLOGITS_GIVEN)),
                     "%s: GIST_STEP_PHASE_* / GIST_STEP_DLOGITS_GIVEN are not supported (one call per iteration; the phase "
                     "calls: %s)", who, other ? other : "this step has none");
    }
    GIST_REQUIRE((flags & ~known) == 0, "%s: unknown flag bits", who);
    GIST_REQUIRE(!((flags & GIST_STEP_EXTRACT) && (flags & GIST_STEP_PREEXTRACTED)),
                 "%s: GIST_STEP_EXTRACT and GIST_STEP_PREEXTRACTED exclude each other", who);
    GIST_REQUIRE(!(flags & (GIST_STEP_EXTRACT_NEXT | GIST_STEP_PREEXTRACTED)) || (flags & GIST_STEP_TRAIN),
                 "%s: GIST_STEP_EXTRACT_NEXT / GIST_STEP_PREEXTRACTED belong to training steps", who);
    return GIST_OK;
}

// The batch's graph, labels and loss buffers.  family: what else the family's forward and backward read of the batch.
template <class Plan>
int check_batch_buffers(const char *who, const Plan *p, bool family) {
    GIST_REQUIRE(family && p->rowptr && p->col && p->t_rowptr && p->t_col && p->labels && p->dlogits && p->row_loss &&
                     p->loss,
                 "%s: null batch / loss buffer", who);
    return GIST_OK;
}
template <class Plan>
int check_arena(const char *who, const Plan *p, int64_t adam_step) {
    GIST_REQUIRE(p->params && p->grads && p->exp_avg && p->exp_avg_sq && p->n_params > 0, "%s: null arena", who);
    GIST_REQUIRE(adam_step >= 1, "%s: adam_step is 1-based", who);
    return GIST_OK;
}

// the one-launch extraction (part tables) instead of gist_extract_batch?
template <class Plan>
bool extracts_by_parts(const Plan *p) {
    return p->node_part && p->part_slot && p->extract_scratch && p->batch_index >= 0 &&
           gist_extract_parts_supported(p->n_max) == 1;
}
template <class Plan>
bool resident_graph_ok(const Plan *p) {
    return p->g_rowptr && p->g_col && p->g_t_rowptr && p->g_t_col && p->feat;
}

// What GIST_STEP_EXTRACT reads.  family: the family's own conditions on the resident graph, `note` what its message
// adds about them.
template <class Plan>
int check_extract(const char *who, const Plan *p, const int32_t *ids, bool by_parts, bool family, const char *note) {
    GIST_REQUIRE(ids != nullptr, "%s: null ids", who);
    GIST_REQUIRE(resident_graph_ok(p) && family && p->col_capacity >= 0, "%s: null / bad resident graph%s", who, note);
    GIST_REQUIRE(by_parts || p->remap != nullptr, "%s: extraction needs the part tables or remap", who);
    return GIST_OK;
}

// What GIST_STEP_EXTRACT_NEXT reads.  family: what else the family's extraction in the optimiser's grid needs.
template <class Plan>
int check_extract_next(const char *who, const Plan *p, bool family) {
    GIST_REQUIRE(p->node_part && p->part_slot && p->extract_scratch && p->next_ids && p->next_batch_index >= 0 &&
                     p->next_n > 0 && p->next_n <= p->n_max && gist_extract_parts_supported(p->n_max) == 1 &&
                     resident_graph_ok(p) && family,
                 "%s: GIST_STEP_EXTRACT_NEXT needs the part tables, the scratch and next_*", who);
    return GIST_OK;
}

// GIST_ENOSPACE unless the plan's buffer `what` has the `need` units this call asks of it
inline int enough(const char *who, const char *what, int64_t have, int64_t need, const char *unit) {
    if (need <= have) return GIST_OK;
    set_error("%s: %s too small (%lld < %lld %s)", who, what, (long long)have, (long long)need, unit);
    return GIST_ENOSPACE;
}

// Layer k's three projections g get what the op-level wrappers give them (the split-K choice depends on the bytes).
// fwd / bwd: does this call run the layer's forward product / its two gradients (layer 0 has no input gradient)?
template <class Plan>
int pick_workspaces(const char *who, const Plan *p, int k, const GemmShape (&g)[3], bool fwd, bool bwd, Ws (&ws)[3]) {
    for (int q = 0; q < 3; ++q) {
        const bool runs = q == 0 ? fwd : (bwd && (q == 1 || k > 0));
        const int64_t need = runs ? gist_gemm_workspace_bytes(g[q].m, g[q].n, g[q].k) : 0;
        GIST_TRY(enough(who, "workspace", p->workspace ? p->workspace_bytes : 0, need, "bytes"));
        ws[q] = need > 0 ? Ws{p->workspace, p->workspace_bytes} : Ws{nullptr, 0};
    }
    return GIST_OK;
}

// GIST_STEP_EXTRACT: batch ids[0..n) into the plan's batch buffers, n_feat feature columns to z0 (ld ldz0)
template <class Plan>
int extract(const Plan *p, bool by_parts, int flags, const int32_t *ids, int64_t n, int64_t n_feat, float *z0,
            int64_t ldz0, gist_stream_t s) {
    if (!(flags & GIST_STEP_EXTRACT)) return GIST_OK;
    if (by_parts) {
        const gist_extract_parts_desc x = parts_desc(p, ids, n, p->batch_index, n_feat, z0, ldz0);
        return gist_extract_parts_desc_batch(&x, s);
    }
    return gist_extract_batch(p->g_rowptr, p->g_col, p->g_t_rowptr, p->g_t_col, ids, n, p->remap, p->rowptr, p->col,
                              p->t_rowptr, p->t_col, p->col_capacity, p->norm, p->feat, p->ld_feat, n_feat, z0, ldz0,
                              p->labels_all, p->labels, s);
}

// One optimiser launch over the arena; with GIST_STEP_EXTRACT_NEXT the next batch is extracted in its grid.
struct AdamHyper { float lr, beta1, beta2, eps, weight_decay; int64_t step; };
template <class Plan>
int optimise(const Plan *p, int flags, int64_t n_feat, float *z0, int64_t ldz0, const AdamHyper &a, gist_stream_t s) {
    if (flags & GIST_STEP_EXTRACT_NEXT) {
        const gist_extract_parts_desc x = parts_desc(p, p->next_ids, p->next_n, p->next_batch_index, n_feat, z0, ldz0);
        return gist_adam_segments_extract_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, a.lr, a.beta1,
                                              a.beta2, a.eps, a.weight_decay, a.step, nullptr, 0, nullptr, 0, 0, nullptr,
                                              &x, s);
    }
    return gist_adam_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, a.lr, a.beta1, a.beta2, a.eps,
                         a.weight_decay, a.step, s);
}
}  // namespace gist
