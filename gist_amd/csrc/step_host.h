// Host-side helpers the two native step drivers share (step.hip: GraphSAGE, gat_step.hip: GAT).
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

// The one-launch extraction (gist_extract_parts_desc_batch) of batch `batch` = `ids[0..n)` from a step plan's resident
// graph and part tables into its batch buffers: features to z0[n][n_feat] (ld ldz0).  gist_step_plan and
// gist_gat_step_plan name these fields alike.  What only one family has (the dropout fold, the aggregating gather) stays
// zero for its caller to fill.
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
}  // namespace gist
