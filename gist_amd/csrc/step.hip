// Native step driver: one C-ABI call issues the whole training iteration (batch
// extraction -> forward -> CE -> backward -> Adam) on one stream.  The host-side
// sequencing of the reference's loop body (cluster_gcn_ist_distrib.py:408-417) moves
// from ~45 interpreter round trips to ~45 back-to-back hipLaunch calls, which is what
// bounds the small-width (many-GPU) regime.  Arithmetic is unchanged: it calls the same
// entry points the op-level API exposes.
#include <math.h>

#include <new>

#include "step_host.h"
#include "class_dw_body.h"

using namespace gist;

// ---- HIP-event timer ------------------------------------------------------------------
struct gist_timer {
    int64_t capacity, count;
    hipEvent_t *start, *stop;
    int32_t *kind;
    int64_t *m, *n, *k;
};

extern "C" gist_timer *gist_timer_create(int64_t capacity) {
    if (capacity <= 0) return nullptr;
    gist_timer *t = new (std::nothrow) gist_timer();
    if (!t) return nullptr;
    t->capacity = capacity;
    t->count = 0;
    t->start = new hipEvent_t[capacity];
    t->stop = new hipEvent_t[capacity];
    t->kind = new int32_t[capacity];
    t->m = new int64_t[capacity];
    t->n = new int64_t[capacity];
    t->k = new int64_t[capacity];
    for (int64_t i = 0; i < capacity; ++i) {
        if (hipEventCreate(&t->start[i]) != hipSuccess || hipEventCreate(&t->stop[i]) != hipSuccess) {
            set_error("gist_timer_create: hipEventCreate failed");
            t->capacity = i;
            break;
        }
    }
    return t;
}

extern "C" void gist_timer_destroy(gist_timer *t) {
    if (!t) return;
    for (int64_t i = 0; i < t->capacity; ++i) {
        (void)hipEventDestroy(t->start[i]);
        (void)hipEventDestroy(t->stop[i]);
    }
    delete[] t->start; delete[] t->stop; delete[] t->kind;
    delete[] t->m; delete[] t->n; delete[] t->k;
    delete t;
}

extern "C" void gist_timer_reset(gist_timer *t) { if (t) t->count = 0; }
extern "C" int64_t gist_timer_count(const gist_timer *t) { return t ? t->count : 0; }

extern "C" int gist_timer_read(gist_timer *t, int64_t i, float *ms, int32_t *kind, int64_t *m,
                               int64_t *n, int64_t *k) {
    GIST_REQUIRE(t && i >= 0 && i < t->count && ms, "gist_timer_read: bad index");
    hipError_t e = hipEventElapsedTime(ms, t->start[i], t->stop[i]);
    if (e != hipSuccess) { set_error("gist_timer_read: %s", hipGetErrorString(e)); return GIST_ELAUNCH; }
    if (kind) *kind = t->kind[i];
    if (m) *m = t->m[i];
    if (n) *n = t->n[i];
    if (k) *k = t->k[i];
    return GIST_OK;
}

namespace gist {
thread_local gist_timer *tl_timer = nullptr;

int64_t timer_begin(gist_timer *t, int kind, int64_t m, int64_t n, int64_t k, hipStream_t s) {
    if (!t || t->count >= t->capacity) return -1;
    const int64_t slot = t->count++;
    t->kind[slot] = kind; t->m[slot] = m; t->n[slot] = n; t->k[slot] = k;
    (void)hipEventRecord(t->start[slot], s);
    return slot;
}

void timer_end(gist_timer *t, int64_t slot, hipStream_t s) {
    if (t && slot >= 0) (void)hipEventRecord(t->stop[slot], s);
}
}  // namespace gist

// ---- split projection operands kept by the step (gist_step_plan.h3_workspace) ---------------
namespace {
struct H3Layer {
    bool on;                       // this layer's three projections run on pre-split operands
    int shift;                     // fixed scale exponent of its input activations Z_k
    uint32_t *Zs, *ZsT, *Ws, *WsT; // [n][kpad(2in)], [2in][kpad(n)], [out][kpad(2in)], [2in][kpad(out)]
    float *inv_zr, *inv_zt, *inv_wr, *inv_wt;
};
struct H3Step {
    bool any;
    H3Layer layer[GIST_MAX_LAYERS];
    uint32_t *dYs, *dYsT;          // [n][kpad(out)], [out][kpad(n)] (shared by the layers)
    float *inv_dyr, *inv_dyt, *rowmax, *colmax, *pmax;
    unsigned *amax;                // [GIST_MAX_LAYERS]
    int64_t bytes;
};

// the plan (gemm_plan.h) of a projection on the step's kept split operands in `mode`, with all the scratch it asks for
inline GemmPlan kept_plan(int mode, int64_t m, int64_t n, int64_t k, int64_t ldc = 0) {
    GemmQuery q = gemm_query(0, m, n, k, mode, GEMM_CALL_KEPT, false);
    q.ldc = ldc;
    return plan_gemm(q);
}

inline int bound_shift(double bound) {      // 2^shift * bound <= 2^13
    int e = 0;
    (void)frexp(bound, &e);                  // bound = f * 2^e, f in [0.5, 1)
    const int s = 13 - e;
    return s < -60 ? -60 : (s > 60 ? 60 : s);
}

// Deterministic carve-up of the workspace from the plan's shapes in GEMM mode `mode`; base may be NULL (sizing).
H3Step h3_layout(const gist_step_plan *p, char *base, int mode) {
    H3Step h{};
    const int L1 = p->n_layers;
    const int64_t n = p->n_max;
    if (mode != 1 || n <= 0) return h;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char *q = base ? base + off : nullptr;
        off += ceil_div(bytes, 256) * 256;
        return q;
    };
    int64_t max_out = 0;
    const double keep = drop_scale_of(p->p_drop);      // the fp32 factor the kernels multiply a kept element by
    for (int k = 0; k < L1; ++k) {
        const gist_layer_desc &l = p->layer[k];
        const int64_t i2 = 2 * l.n_in, o = l.n_out;
        H3Layer &hl = h.layer[k];
        const double bound = k == 0 ? (double)p->feat_absmax * keep
                                    : (p->use_layernorm ? sqrt((double)(l.n_in > 1 ? l.n_in - 1 : 1)) * keep : 0.0);
        // the class layer (k == L1-1) stays on the per-call path: its dY = dlogits comes from the CE
        // kernel, which writes no row maxima for the gradient split
        hl.on = k < L1 - 1 && bound > 0.0 && kept_plan(mode, n, o, i2).kept_ok && kept_plan(mode, o, i2, n).kept_ok &&
                (k == 0 || kept_plan(mode, n, i2, o).kept_ok) && l.ldz % 4 == 0 && l.ldy % 4 == 0 &&
                aligned16(l.W) && aligned16(l.Z) && aligned16(l.Y) && aligned16(l.dW);
        if (!hl.on) continue;
        h.any = true;
        hl.shift = bound_shift(bound);
        hl.Zs = reinterpret_cast<uint32_t *>(take(n * h3_kpad(i2) * 4));
        hl.ZsT = reinterpret_cast<uint32_t *>(take(i2 * h3_kpad(n) * 4));
        hl.Ws = reinterpret_cast<uint32_t *>(take(o * h3_kpad(i2) * 4));
        hl.WsT = k > 0 ? reinterpret_cast<uint32_t *>(take(i2 * h3_kpad(o) * 4)) : nullptr;
        hl.inv_zr = reinterpret_cast<float *>(take(n * 4));
        hl.inv_zt = reinterpret_cast<float *>(take(i2 * 4));
        hl.inv_wr = reinterpret_cast<float *>(take(o * 4));
        hl.inv_wt = k > 0 ? reinterpret_cast<float *>(take(i2 * 4)) : nullptr;
        max_out = o > max_out ? o : max_out;
    }
    if (!h.any) return h;
    h.dYs = reinterpret_cast<uint32_t *>(take(n * h3_kpad(max_out) * 4));
    h.dYsT = reinterpret_cast<uint32_t *>(take(max_out * h3_kpad(n) * 4));
    h.inv_dyr = reinterpret_cast<float *>(take(n * 4));
    h.inv_dyt = reinterpret_cast<float *>(take(max_out * 4));
    h.rowmax = reinterpret_cast<float *>(take(n * 4));
    h.colmax = reinterpret_cast<float *>(take(max_out * 4));
    h.pmax = reinterpret_cast<float *>(take(gist_colsum_partials(n) * max_out * 4));
    h.amax = reinterpret_cast<unsigned *>(take(GIST_MAX_LAYERS * 4));
    h.bytes = off;
    return h;
}

// bf16x3 mode: the same idea without scales -- three bf16 pieces per element, 6 bytes each
struct B3Layer {
    bool on;
    uint16_t *Zs, *ZsT, *Ws, *WsT; // [n][kpad(2in)], [2in][kpad(n)], [out][kpad(2in)], [2in][kpad(out)]
};
struct B3Step {
    bool any;
    B3Layer layer[GIST_MAX_LAYERS];
    uint16_t *dYs, *dYsT;          // [n][kpad(out)], [out][kpad(n)] (shared by the layers)
    float *slabs; int64_t slab_bytes;     // split-K slabs of the layers' projections (shared)
    int64_t bytes;
};

B3Step b3_layout(const gist_step_plan *p, char *base, int mode) {
    B3Step h{};
    const int L1 = p->n_layers;
    const int64_t n = p->n_max;
    if (mode != 2 || n <= 0) return h;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char *q = base ? base + off : nullptr;
        off += ceil_div(bytes, 256) * 256;
        return reinterpret_cast<uint16_t *>(q);
    };
    int64_t max_out = 0;
    for (int k = 0; k < L1; ++k) {
        const gist_layer_desc &l = p->layer[k];
        const int64_t i2 = 2 * l.n_in, o = l.n_out;
        B3Layer &hl = h.layer[k];
        // (Y = Z . W^T, dW = dY^T . Z, dZ = dY . W, each with its output's leading dimension)
        hl.on = kept_plan(mode, n, o, i2, l.ldy).kept_ok && kept_plan(mode, o, i2, n, i2).kept_ok &&
                (k == 0 || kept_plan(mode, n, i2, o, i2).kept_ok);
        if (!hl.on) continue;
        h.any = true;
        hl.Zs = take(n * b3_kpad(i2) * 6);
        hl.ZsT = take(i2 * b3_kpad(n) * 6);
        hl.Ws = take(o * b3_kpad(i2) * 6);
        hl.WsT = k > 0 ? take(i2 * b3_kpad(o) * 6) : nullptr;
        max_out = o > max_out ? o : max_out;
        // split-K slabs: the slice count depends on the batch rows through the tile count, and a batch
        // may have fewer rows than n_max (one 256-row tile less can double the slices): the largest
        // need over every row count up to n_max (the launcher uses one slice if the slab is too small)
        // (sampled at every row count that changes a tile count AND at every row count that changes the
        // number of 64-row k pairs of the dW projection: the slice count is not monotone in either)
        int64_t sb = 0;
        for (int64_t rows = n; rows > 0; rows = (rows - 1) / 64 * 64) {
            const int64_t need[3] = {kept_plan(mode, rows, o, i2).scratch_bytes, kept_plan(mode, o, i2, rows).scratch_bytes,
                                     k > 0 ? kept_plan(mode, rows, i2, o).scratch_bytes : 0};
            for (int q = 0; q < 3; ++q) sb = need[q] > sb ? need[q] : sb;
        }
        if (sb > h.slab_bytes) h.slab_bytes = sb;
    }
    if (!h.any) return h;
    h.dYs = take(n * b3_kpad(max_out) * 6);
    h.dYsT = take(max_out * b3_kpad(n) * 6);
    h.slabs = h.slab_bytes > 0 ? reinterpret_cast<float *>(take(h.slab_bytes)) : nullptr;
    h.bytes = off;
    return h;
}
}  // namespace

// ---- fused sequence: slabs of the deferred split-K projections, bias-gradient chunk sums -------------
namespace {
constexpr int64_t kLnbMaxUnits = 256;
struct FusedLayout {
    float *dw_slabs[GIST_MAX_LAYERS]; int64_t dw_bytes[GIST_MAX_LAYERS];   // dW_k = dY_k^T . Z_k
    float *logit_slabs; int64_t logit_bytes;                               // class layer's Y = Z . W^T
    float *y_slabs; int64_t y_bytes;      // a hidden layer's Y = Z . W^T until its LayerNorm has read it (one buffer)
    float *partials[GIST_MAX_LAYERS];                                      // [partial_rows[k] >= row_chunks16(n_max)][n_out_k]
    int64_t partial_rows[GIST_MAX_LAYERS];
    int64_t bytes, partial_floats;
};

// the largest slab need over the batch sizes a plan sees (the split count depends on the reduction
// length); a batch that would need more falls back to one k slice inside the launcher
int64_t slab_need(int64_t m, int64_t n, int64_t k_max, bool k_is_rows) {
    // (called for every layer of every step: remembered per shape and GEMM mode)
    struct Memo { int64_t m, n, k; int rows, mode; int64_t need; };
    static thread_local Memo memo[32];
    static thread_local int memo_n = 0;
    const int mode = gist_gemm_get_mode();
    // (tuning overrides change tile and slice choices: neither read nor fill the memo while one is set)
    const bool tuned = tune(GIST_TUNE_GEMM_TILE) != 0.0 || tune(GIST_TUNE_GEMM_SPLITS) != 0.0 || tune(GIST_TUNE_B3C) != 0.0 ||
                       tune(GIST_TUNE_B3C_SPLITS) != 0.0;
    for (int i = 0; i < memo_n && !tuned; ++i)
        if (memo[i].m == m && memo[i].n == n && memo[i].k == k_max && memo[i].rows == (int)k_is_rows && memo[i].mode == mode)
            return memo[i].need;
    int64_t need = 0;
    // every 32 rows down to half the largest batch (the model's slice count is not monotone in the reduction
    // length: two neighbouring batch sizes can differ by a factor of two)
    for (int64_t rows = k_max; rows > 0 && rows >= k_max / 2; rows -= 32) {
        const int64_t b = k_is_rows ? gemm_slab_bytes(2, m, n, rows, mode) : gemm_slab_bytes(0, rows, n, m, mode);
        need = b > need ? b : need;
    }
    if (!tuned) {      // a full table overwrites its oldest entry instead of recomputing every call
        static thread_local int memo_next = 0;
        if (memo_n < 32) memo[memo_n++] = Memo{m, n, k_max, (int)k_is_rows, mode, need};
        else { memo[memo_next] = Memo{m, n, k_max, (int)k_is_rows, mode, need}; memo_next = (memo_next + 1) % 32; }
    }
    return need;
}

FusedLayout fused_layout(const gist_step_plan *p, char *base, float *partials) {
    FusedLayout f{};
    const int L1 = p->n_layers;
    int64_t off = 0, poff = 0;
    auto take = [&](int64_t bytes) {
        char *q = base ? base + off : nullptr;
        off += ceil_div(bytes, 256) * 256;
        return reinterpret_cast<float *>(q);
    };
    const int64_t chunks = gist_row_chunks16(p->n_max);
    for (int k = 0; k < L1; ++k) {
        const gist_layer_desc &l = p->layer[k];
        f.dw_bytes[k] = slab_need(l.n_out, 2 * l.n_in, p->n_max, true);
        if (k == L1 - 1 && gist_class_layer_takes(p->n_max, l.n_out, 2 * l.n_in, 2 * l.n_in, 2 * l.n_in, nullptr, nullptr)) {
            // the fused class layer leaves dW as one slab per 128 rows (gist_class_dw_slabs_f32)
            const int64_t b = gist_class_dw_slab_bytes(p->n_max, l.n_out, 2 * l.n_in);
            f.dw_bytes[k] = b > f.dw_bytes[k] ? b : f.dw_bytes[k];
        }
        f.dw_slabs[k] = f.dw_bytes[k] > 0 ? take(f.dw_bytes[k]) : nullptr;
        f.partials[k] = partials ? partials + poff : nullptr;
        // (a hidden layer of <= 256 columns may get its chunk sums from the reverse aggregation above it: one row per
        // workgroup of that launch, at most kLnbMaxUnits of them)
        const int64_t rows = (k + 1 < L1 && l.n_out <= 256 && chunks < kLnbMaxUnits) ? kLnbMaxUnits : chunks;
        f.partial_rows[k] = rows;
        poff += ceil_div(rows * l.n_out, 64) * 64;
    }
    const gist_layer_desc &last = p->layer[L1 - 1];
    f.logit_bytes = slab_need(2 * last.n_in, last.n_out, p->n_max, false);
    f.logit_slabs = f.logit_bytes > 0 ? take(f.logit_bytes) : nullptr;
    f.y_bytes = 0;
    for (int k = 0; k + 1 < L1; ++k) {
        const int64_t b = slab_need(2 * p->layer[k].n_in, p->layer[k].n_out, p->n_max, false);
        f.y_bytes = b > f.y_bytes ? b : f.y_bytes;
    }
    f.y_slabs = f.y_bytes > 0 ? take(f.y_bytes) : nullptr;
    f.bytes = off;
    f.partial_floats = poff;
    return f;
}
}  // namespace

extern "C" int64_t gist_step_fused_workspace_bytes(const gist_step_plan *plan) {
    if (!plan || plan->n_layers < 1 || plan->n_layers > GIST_MAX_LAYERS || plan->n_max <= 0) return 0;
    return fused_layout(plan, nullptr, nullptr).bytes;
}
// bytes reserved for the slabs of layer k's weight gradient (k == n_layers: the class layer's logits)
extern "C" int64_t gist_step_fused_slab_bytes(const gist_step_plan *plan, int32_t k) {
    if (!plan || plan->n_layers < 1 || plan->n_layers > GIST_MAX_LAYERS || plan->n_max <= 0) return 0;
    if (k < 0 || k > plan->n_layers + 1) return 0;
    const FusedLayout f = fused_layout(plan, nullptr, nullptr);
    if (k == plan->n_layers + 1) return f.y_bytes;      // the hidden layers' forward projections (shared)
    return k == plan->n_layers ? f.logit_bytes : f.dw_bytes[k];
}
extern "C" int64_t gist_step_col_partials_floats(const gist_step_plan *plan) {
    if (!plan || plan->n_layers < 1 || plan->n_layers > GIST_MAX_LAYERS || plan->n_max <= 0) return 0;
    return fused_layout(plan, nullptr, nullptr).partial_floats;
}

extern "C" int64_t gist_step_h3_workspace_bytes(const gist_step_plan *plan) {
    return gist_step_h3_workspace_bytes_mode(plan, gist_gemm_get_mode());
}

// the same for a given GEMM mode, without touching the process-wide one (a caller that sizes for every
// mode it may switch to must not change the arithmetic of launches other threads issue meanwhile)
extern "C" int64_t gist_step_h3_workspace_bytes_mode(const gist_step_plan *plan, int mode) {
    if (!plan || plan->n_layers < 1 || plan->n_layers > GIST_MAX_LAYERS || mode < 0 || mode > 2) return 0;
    return mode == 2 ? b3_layout(plan, nullptr, mode).bytes : h3_layout(plan, nullptr, mode).bytes;
}

// ---- one call's decisions, each made once ----------------------------------------------------------------
namespace {
constexpr int kPhaseBits = GIST_STEP_PHASE_FORWARD | GIST_STEP_PHASE_BACKWARD | GIST_STEP_PHASE_OPTIMIZER;

// Everything gist_sage_step decides before it launches, filled by decide() from (plan, n, drop_offset, flags).
// Phases (gist_hip.h, GIST_STEP_PHASE_*): a caller whose loop is `pred = model(g); loss = f(pred); loss.backward();
// optimizer.step()` issues the same iteration as three calls.  Only do_* and split_phases read the phase bits, so the
// three calls agree on everything else.
struct StepDecisions {
    bool train, drop;
    bool do_fwd, do_bwd, do_opt;   // the phases this call runs
    bool split_phases;             // one phase of three calls (not none / all three bits)
    bool dlogits_given;
    bool blocked;                  // the batch comes with its locality blocks
    bool pairs;                    // may the batch have sibling blocks (speed only: gist_hip.h)
    int gemm_mode;
    H3Step h3;                     // split operands kept by the step (gist_step_plan.h3_workspace), by GEMM mode;
    B3Step b3;                     //   a layer that is `on` in neither splits per call inside gist_gemm_*
    bool fuse;                     // the fused sequence (gist_step_plan.fuse)
    bool defer;                    // slabs + chunk sums consumed by the loss kernel / the optimiser
    FusedLayout fl;
    uint64_t offs[GIST_MAX_LAYERS];        // mask offset of layer k's [h | ah]
    bool plain[GIST_MAX_LAYERS];           // layer k is on neither kept-split path
    bool fwd_fold[GIST_MAX_LAYERS];        // forward: dropout([h | ah]) written by the producers, the aggregation reads hsrc[k]
    bool mask_in_spmm[GIST_MAX_LAYERS];    // backward: the mask of dZ_k applied by the reverse aggregation as it reads dZ_k
    bool cls_fused;                // the class layer as gist_class_layer_f32 + gist_class_dw_slabs_f32
};

// a kept-split layout carved from the plan's workspace; none if the workspace is missing, misaligned or too small, or
// the batch has more rows than it was sized for
template <class Step>
Step kept_splits(const gist_step_plan *p, int64_t n, int mode, Step (*layout)(const gist_step_plan *, char *, int)) {
    if (p->h3_workspace == nullptr || !aligned16(p->h3_workspace) || n > p->n_max) return Step{};
    const Step h = layout(p, static_cast<char *>(p->h3_workspace), mode);
    return h.bytes > p->h3_workspace_bytes ? Step{} : h;
}

// May layer k's dropout be folded into the producers of [h | ah] when its mask starts at `offset`?  A function of the
// layer and the offset, so that the optimiser can apply it to the NEXT batch's layer 0 (gist_extract_parts_desc.x0) the
// way the next call applies it to itself.  Reads d.fuse, d.drop and d.plain.  (Every aggregation kernel carries the
// forward mask, whatever the shape: spmm_choose.)
bool folds_forward(const gist_step_plan *p, const StepDecisions &d, int k, uint64_t offset) {
    const gist_layer_desc &l = p->layer[k];
    return d.fuse && d.drop && d.plain[k] && p->hsrc[k] != nullptr && (offset & 1) == 0 && p->ld_hsrc[k] >= l.n_in;
}

// The step's aggregations run on the batch's locality blocks when it comes with them (otherwise on the row kernels), read
// the batch's prepared block structure of their orientation where there is one (StepState), and look for sibling blocks
// only if the plan says the batch may have them.
// Layer k's reverse aggregation: dO_{k-1} = the A^T-aggregate of dZ_k's right half, added into its left half; masked:
// under dZ_k's dropout mask, applied by the aggregation as it reads dZ_k.
SpmmCall reverse_call(const gist_step_plan *p, const StepDecisions &d, int64_t n, int k, bool masked) {
    const gist_layer_desc &l = p->layer[k];
    SpmmCall c{"gist_sage_step", p->t_rowptr, p->t_col, n, p->dZ + l.n_in, 2 * l.n_in, p->dZ, 2 * l.n_in, l.n_in, nullptr,
               p->norm, 1};
    c.set_blocks(d.blocked ? p->row_blocks : nullptr, p->n_row_blocks, SPMM_BLOCKS_NONE);
    c.pairs = d.pairs;
    if (masked) c.dr = spmm_drop_of(2, p->p_drop, p->seed, d.offs[k], d.offs[k] + (uint64_t)l.n_in, 2 * l.n_in);
    return c;
}

StepDecisions decide(const gist_step_plan *p, int64_t n, uint64_t drop_offset, int flags) {
    StepDecisions d{};
    const int L1 = p->n_layers;
    const int phases = flags & kPhaseBits;
    d.train = (flags & GIST_STEP_TRAIN) != 0;
    d.drop = d.train && p->p_drop > 0.f;
    d.do_fwd = phases == 0 || (phases & GIST_STEP_PHASE_FORWARD);
    d.do_bwd = d.train && (phases == 0 || (phases & GIST_STEP_PHASE_BACKWARD));
    d.do_opt = d.train && (phases == 0 || (phases & GIST_STEP_PHASE_OPTIMIZER));
    d.split_phases = phases != 0 && phases != kPhaseBits;
    d.dlogits_given = (flags & GIST_STEP_DLOGITS_GIVEN) != 0;
    d.blocked = p->row_blocks != nullptr && p->n_row_blocks > 0;
    d.pairs = p->sibling_parts != 0;
    d.gemm_mode = gist_gemm_get_mode();
    d.h3 = kept_splits<H3Step>(p, n, d.gemm_mode, h3_layout);
    d.b3 = kept_splits<B3Step>(p, n, d.gemm_mode, b3_layout);
    d.fuse = p->fuse != 0 && n <= p->n_max;
    if (d.fuse && p->col_partials != nullptr && aligned16(p->col_partials)) {
        d.fl = fused_layout(p, static_cast<char *>(p->fused_workspace), p->col_partials);
        d.defer = p->fused_workspace == nullptr ? d.fl.bytes == 0
                                                : (aligned16(p->fused_workspace) && d.fl.bytes <= p->fused_workspace_bytes);
        if (!d.defer) d.fl = FusedLayout{};
    }
    uint64_t off = drop_offset;
    for (int k = 0; k < L1; ++k) {
        const gist_layer_desc &l = p->layer[k];
        d.offs[k] = off;
        if (d.drop) off += round_up2((uint64_t)n * 2 * l.n_in);
        d.plain[k] = !d.h3.layer[k].on && !d.b3.layer[k].on;
        // (layer 0's producer is the extraction: this call's, or the previous call's GIST_STEP_EXTRACT_NEXT)
        d.fwd_fold[k] = (k > 0 || (flags & (GIST_STEP_EXTRACT | GIST_STEP_PREEXTRACTED))) && folds_forward(p, d, k, d.offs[k]);
        d.mask_in_spmm[k] = d.fuse && d.drop && k > 0 && k < L1 - 1 && (d.offs[k] & 1) == 0 &&
                            spmm_choose(reverse_call(p, d, n, k, true)).refusal == nullptr;
    }
    // the class layer as gist_class_layer_f32 + gist_class_dw_slabs_f32 (projection, CE, dZ with its mask and the
    // bias gradient's chunk sums in one launch, dW as slabs for the optimiser) instead of four launches
    const gist_layer_desc &l = p->layer[L1 - 1];
    d.cls_fused = d.train && d.defer && d.plain[L1 - 1] && p->ldc <= 64 && (d.offs[L1 - 1] & 1) == 0 &&
                  (int)tune(GIST_TUNE_CLASS_FUSED) != 1 &&
                  gist_class_layer_takes(n, l.n_out, 2 * l.n_in, l.ldz, 2 * l.n_in, l.Z, l.W) == 1 &&
                  d.fl.dw_slabs[L1 - 1] != nullptr &&
                  d.fl.dw_bytes[L1 - 1] >= gist_class_dw_slab_bytes(n, l.n_out, 2 * l.n_in);
    return d;
}

// can batch `batch` = ids[0..n) be extracted by gist_extract_parts_batch's kernel?
bool extracts_by_parts(const gist_step_plan *p, const StepDecisions &d, const int32_t *ids, int64_t n, int32_t batch) {
    return d.fuse && p->node_part && p->part_slot && p->extract_scratch && ids && batch >= 0 && n > 0 && n <= p->n_max &&
           gist_extract_parts_supported(p->n_max) == 1;
}

// does the optimiser launch of this step also extract the next batch (plan->next_*)?
// (beside a LARGE optimiser pass the extraction's 1024-thread workgroups cost more than they hide: each holds half a
// CU's wave slots for the ~20 us of its look-back chain -- 233 against 199 + 21 us at 38.8 M parameters, 32 against
// 16 + 21 at 1.2 M.  With the aggregating extraction's loads restructured the break-even is at ~11 M: H = 2048,
// 11.0 M parameters, 0.9788 / 0.9822 ms per step against 0.9807 / 0.9836 without; H = 4096, 38.8 M: +70 us)
constexpr int64_t kPrefetchMaxParams = 12LL << 20;
bool prefetches_next(const gist_step_plan *p, const StepDecisions &d) {
    return d.defer && p->n_params <= kPrefetchMaxParams &&
           extracts_by_parts(p, d, p->next_ids, p->next_n, p->next_batch_index);
}

// the one-launch extraction of a batch whose masks start at `offset`: layer 0's mask goes into the feature gather where
// folds_forward says so, and layer 0's aggregation comes with it when the plan has the intra-part sums
gist_extract_parts_desc sage_parts_desc(const gist_step_plan *p, const StepDecisions &d, const int32_t *ids, int64_t n,
                                        int32_t batch, uint64_t offset) {
    const gist_layer_desc &l0 = p->layer[0];
    gist_extract_parts_desc x = parts_desc(p, ids, n, batch, l0.n_in, l0.Z, l0.ldz);
    x.x0 = folds_forward(p, d, 0, offset) ? p->hsrc[0] : nullptr; x.ldx0 = p->ld_hsrc[0]; x.p = p->p_drop; x.seed = p->seed;
    x.offset = offset; x.mask_ld = 2 * l0.n_in;
    if (p->feat_intra != nullptr) { x.feat_intra = p->feat_intra; x.ld_intra = p->ld_feat_intra; x.ah = l0.Z + l0.n_in; }
    return x;
}

// what crosses the phases of one call
struct StepState {
    bool pre_ah;                       // layer 0's aggregation was formed by the extraction
    const void *prep_fwd, *prep_bwd;   // the batch's prepared block structure, per orientation (NULL: none)
    gist_grad_segment segs[2 * GIST_MAX_LAYERS];      // gradient sums left to the optimiser
    int n_segs;
};

// grads[dst .. dst + count) = the sum of n_src dense partial arrays at src (chunk sums of a bias gradient, split-K slabs
// of a weight gradient), formed by the optimiser
void add_segment(const gist_step_plan *p, StepState &x, const float *dst, int64_t count, const float *src, int64_t n_src) {
    gist_grad_segment &g = x.segs[x.n_segs++];
    g.begin = dst - p->grads; g.end = g.begin + count;
    g.src = src; g.stride = count; g.n_src = (int32_t)n_src;
}

// ---- phase 1: this step's weights as kept split operands ---------------------------------------------------
int split_weights(const gist_step_plan *p, const StepDecisions &d, hipStream_t st) {
    const int L1 = p->n_layers;
    if (d.b3.any) {      // one read each, one launch for all of them
        Scope sc(p->timer, 3, 0, 0, 0, st);
        B3Dual jobs[GIST_MAX_LAYERS];
        int n_jobs = 0;
        for (int k = 0; k < L1; ++k) {
            const B3Layer &hl = d.b3.layer[k];
            if (!hl.on) continue;
            const gist_layer_desc &l = p->layer[k];
            B3Dual &j = jobs[n_jobs++];
            j = B3Dual{};
            j.src = l.W; j.ld = 2 * l.n_in; j.rows = l.n_out; j.cols = 2 * l.n_in;
            j.dst_r = hl.Ws;
            j.dst_t = d.train ? hl.WsT : nullptr;
        }
        for (int i = 0; i < n_jobs; i += B3_SPLIT_MAX_JOBS)
            GIST_TRY(b3_split_jobs(jobs + i, n_jobs - i < B3_SPLIT_MAX_JOBS ? n_jobs - i : B3_SPLIT_MAX_JOBS, st));
    }
    if (d.h3.any) {      // rows split for Y = Z.W^T, transposed for dZ = dY.W
        Scope sc(p->timer, 3, 0, 0, 0, st);
        bool zeroed = false;
        for (int k = 0; k < L1; ++k) {
            const H3Layer &hl = d.h3.layer[k];
            if (!hl.on) continue;
            const gist_layer_desc &l = p->layer[k];
            if (k > 0 && d.train) {      // one read of W_k, one scale for the tensor, both layouts
                if (!zeroed && hipMemsetAsync(d.h3.amax, 0, GIST_MAX_LAYERS * 4, st) != hipSuccess) {
                    set_error("gist_sage_step: hipMemsetAsync failed");
                    return GIST_ELAUNCH;
                }
                zeroed = true;
                GIST_TRY(h3_absmax(l.W, 2 * l.n_in, l.n_out, 2 * l.n_in, d.h3.amax + k, st));
                H3Dual j{};
                j.src = l.W; j.ld = 2 * l.n_in; j.rows = l.n_out; j.cols = 2 * l.n_in;
                j.amax = d.h3.amax + k;
                j.dst_r = hl.Ws; j.inv_r = hl.inv_wr; j.dst_t = hl.WsT; j.inv_t = hl.inv_wt;
                GIST_TRY(h3_dual_split(j, st));
            } else {
                GIST_TRY(h3_split_rows(l.W, 2 * l.n_in, l.n_out, 2 * l.n_in, hl.Ws, hl.inv_wr, st));
            }
        }
    }
    return GIST_OK;
}

// ---- phase 2: the batch (GIST_STEP_EXTRACT) and its block structure, once for all its aggregations -----------
int extract_and_prepare(const gist_step_plan *p, const StepDecisions &d, StepState &x, const int32_t *ids, int64_t n,
                        int flags, gist_stream_t s) {
    const gist_layer_desc &l0 = p->layer[0];
    x.pre_ah = (flags & GIST_STEP_PREEXTRACTED) && p->feat_intra != nullptr;
    if ((flags & GIST_STEP_EXTRACT) && d.do_fwd) {
        if (extracts_by_parts(p, d, ids, n, p->batch_index)) {
            const gist_extract_parts_desc desc = sage_parts_desc(p, d, ids, n, p->batch_index, d.offs[0]);
            x.pre_ah = p->feat_intra != nullptr;      // (layer 0's aggregation comes with the extraction)
            GIST_TRY(gist_extract_parts_desc_batch(&desc, s));
        } else if (d.fwd_fold[0])
            GIST_TRY(gist_extract_batch_drop(p->g_rowptr, p->g_col, p->g_t_rowptr, p->g_t_col, ids, n, p->remap, p->rowptr,
                                             p->col, p->t_rowptr, p->t_col, p->col_capacity, p->norm, p->feat, p->ld_feat,
                                             l0.n_in, l0.Z, l0.ldz, p->labels_all, p->labels, p->hsrc[0], p->ld_hsrc[0],
                                             p->p_drop, p->seed, d.offs[0], 2 * l0.n_in, s));
        else
            GIST_TRY(gist_extract_batch(p->g_rowptr, p->g_col, p->g_t_rowptr, p->g_t_col, ids, n, p->remap, p->rowptr,
                                        p->col, p->t_rowptr, p->t_col, p->col_capacity, p->norm, p->feat, p->ld_feat,
                                        l0.n_in, l0.Z, l0.ldz, p->labels_all, p->labels, s));
    }
    if (!d.blocked || p->spmm_prepared == nullptr || !aligned16(p->spmm_prepared)) return GIST_OK;
    const int64_t one = gist_spmm_blocks_bytes(p->n_row_blocks);
    bool wide = false;      // is there an aggregation the prepared kernel takes?
    for (int k = 0; k < p->n_layers; ++k)
        wide = wide || spmm_prepared_takes(p->layer[k].n_in, p->layer[k].ldz, p->layer[k].ldz, p->layer[k].Z,
                                           p->layer[k].Z + p->layer[k].n_in);
    if (!wide || p->spmm_prepared_bytes < (d.train ? 2 : 1) * one) return GIST_OK;
    char *base = static_cast<char *>(p->spmm_prepared), *back = d.train ? base + one : nullptr;
    x.prep_fwd = base;
    x.prep_bwd = back;
    if (d.do_fwd)      // (a backward-phase call reads what the forward-phase call prepared)
        GIST_TRY(launch_spmm_blocks_prepare(p->rowptr, p->col, d.train ? p->t_rowptr : nullptr, d.train ? p->t_col : nullptr,
                                            n, p->row_blocks, p->n_row_blocks, base, back, as_stream(s), d.pairs));
    return GIST_OK;
}

// ---- phase 3: forward (modules.py:310-314 / :218-237) and the loss -----------------------------------------
int forward(const gist_step_plan *p, const StepDecisions &d, const StepState &x, int64_t n, gist_stream_t s) {
    const int L1 = p->n_layers;
    hipStream_t st = as_stream(s);
    const FusedLayout &fl = d.fl;
    int logit_slabs = 0;           // > 1: the class layer's logits are still split-K slabs
    for (int k = 0; k < L1; ++k) {
        const gist_layer_desc &l = p->layer[k];
        int y_slabs_n = 1;                   // > 1: this layer's pre-norm output is still split-K slabs
        const float *y_slabs = nullptr;
        if (!(k == 0 && x.pre_ah)) {
            Scope sc(p->timer, 0, n, n, l.n_in, st);
            SpmmCall c{"gist_sage_step", p->rowptr, p->col, n, l.Z, l.ldz, l.Z + l.n_in, l.ldz, l.n_in, p->norm, nullptr, 0};
            c.set_blocks(d.blocked ? p->row_blocks : nullptr, p->n_row_blocks, SPMM_BLOCKS_NONE);
            c.prepared = x.prep_fwd; c.pairs = d.pairs; c.st = st;
            if (d.fwd_fold[k]) {      // source = the undropped input, store = dropout(ah)
                c.x = p->hsrc[k]; c.ldx = p->ld_hsrc[k];
                c.dr = spmm_drop_of(1, p->p_drop, p->seed, d.offs[k] + (uint64_t)l.n_in, 0, 2 * l.n_in);
            }
            GIST_TRY(spmm_run(c));
        }
        if (d.h3.layer[k].on) {
            // dropout + split of Z_k in one pass (both layouts when training); the dropped fp32 Z_k is never written: the
            // backward only needs its transposed split
            const H3Layer &hl = d.h3.layer[k];
            Scope sc(p->timer, 1, n, l.n_out, 2 * l.n_in, st);
            H3Dual j{};
            j.src = l.Z; j.ld = l.ldz; j.rows = n; j.cols = 2 * l.n_in;
            j.p = d.drop ? p->p_drop : 0.f; j.seed = p->seed; j.offset = d.offs[k];
            j.fixed_shift = hl.shift;
            j.dst_r = hl.Zs; j.inv_r = hl.inv_zr;
            j.dst_t = d.train ? hl.ZsT : nullptr; j.inv_t = hl.inv_zt;
            GIST_TRY(h3_dual_split(j, st));
            GIST_TRY(h3_gemm_presplit("gist_sage_step", hl.Zs, hl.inv_zr, hl.Ws, hl.inv_wr, l.b, l.Y, l.ldy, n, l.n_out,
                                      2 * l.n_in, st));
        } else if (d.b3.layer[k].on) {
            const B3Layer &hl = d.b3.layer[k];
            Scope sc(p->timer, 1, n, l.n_out, 2 * l.n_in, st);
            B3Dual j{};
            j.src = l.Z; j.ld = l.ldz; j.rows = n; j.cols = 2 * l.n_in;
            j.p = d.drop ? p->p_drop : 0.f; j.seed = p->seed; j.offset = d.offs[k];
            j.dst_r = hl.Zs;
            j.dst_t = d.train ? hl.ZsT : nullptr;
            GIST_TRY(b3_dual_split(j, st));
            // (a hidden layer's k slices stay slabs: its LayerNorm, the next launch, sums them as it reads)
            // (with one slice the kernel adds the bias itself; slabs get it from the LayerNorm)
            const bool to_ln = d.defer && k + 1 < L1;
            GIST_TRY(b3_gemm_presplit("gist_sage_step", hl.Zs, hl.Ws, l.b, l.Y, l.ldy, n, l.n_out,
                                      2 * l.n_in, d.b3.slabs, d.b3.slab_bytes, st, to_ln ? &y_slabs_n : nullptr));
            if (to_ln) y_slabs = d.b3.slabs;
        } else {
            if (d.drop && !d.fwd_fold[k])
                GIST_TRY(gist_dropout_f32(l.Z, l.ldz, n, 2 * l.n_in, p->p_drop, p->seed, d.offs[k], s));
            if (d.cls_fused && k == L1 - 1) continue;      // (projection, loss and dZ follow in one launch)
            Scope sc(p->timer, 1, n, l.n_out, 2 * l.n_in, st);
            if (d.defer && k == L1 - 1 && fl.logit_slabs != nullptr) {      // the loss kernel sums the slabs
                GIST_TRY(gemm_slabs(0, l.Z, l.ldz, l.W, 2 * l.n_in, l.b, l.Y, l.ldy, n, l.n_out, 2 * l.n_in,
                                    fl.logit_slabs, fl.logit_bytes, &logit_slabs, st, GEMM_CALL_SLABS));
            } else if (d.defer && k + 1 < L1 && fl.y_slabs != nullptr &&
                       !splits_operands(plan_gemm(gemm_query(0, n, l.n_out, 2 * l.n_in, d.gemm_mode, GEMM_CALL_SPLITS, false)))) {
                // the LayerNorm sums the slabs (a projection the per-call split paths take keeps their workspace).  The query is
                // gist_gemm_splits_operands' own -- a call that reduces its own slices, not a deferred one -- because that is
                // the question the op-by-op twin asks (hip.gemm_splits_own_operands) and the one the workspace was sized by:
                // modes 0-2 answer both forms alike, mode 3 (bf16x1) takes no deferred call and would send the step to slabs
                // where the twin and the size query say gist_gemm_nt_f32
                GIST_TRY(gemm_slabs(0, l.Z, l.ldz, l.W, 2 * l.n_in, l.b, l.Y, l.ldy, n, l.n_out, 2 * l.n_in,
                                    fl.y_slabs, fl.y_bytes, &y_slabs_n, st, GEMM_CALL_SLABS));
                y_slabs = fl.y_slabs;
            } else {
                GIST_TRY(gist_gemm_nt_f32(l.Z, l.ldz, l.W, 2 * l.n_in, l.b, l.Y, l.ldy, n, l.n_out, 2 * l.n_in, p->workspace,
                                          p->workspace_bytes, s));
            }
        }
        if (k + 1 < L1) {
            const gist_layer_desc &nx = p->layer[k + 1];
            const bool fold = d.fwd_fold[k + 1];      // the LayerNorm writes layer k + 1's input with its mask
            float *rstd = p->use_layernorm ? l.rstd : nullptr;
            if (y_slabs_n > 1)
                GIST_TRY(gist_ln_relu_fwd_slabs_f32(l.Y, l.ldy, y_slabs, n * l.n_out, y_slabs_n, l.b, nx.Z, nx.ldz,
                                                    fold ? p->hsrc[k + 1] : nullptr, fold ? p->ld_hsrc[k + 1] : 0, rstd, n,
                                                    l.n_out, p->use_layernorm, 1, 1e-5f, fold ? p->p_drop : 0.f, p->seed,
                                                    fold ? d.offs[k + 1] : 0, fold ? 2 * nx.n_in : l.n_out, s));
            else if (fold)
                GIST_TRY(gist_ln_relu_fwd_drop_f32(l.Y, l.ldy, nx.Z, nx.ldz, p->hsrc[k + 1], p->ld_hsrc[k + 1], rstd, n,
                                                   l.n_out, p->use_layernorm, 1, 1e-5f, p->p_drop, p->seed,
                                                   d.offs[k + 1], 2 * nx.n_in, s));
            else
                GIST_TRY(gist_ln_relu_fwd_f32(l.Y, l.ldy, nx.Z, nx.ldz, rstd, n, l.n_out, p->use_layernorm, 1, 1e-5f, s));
        }
    }
    const gist_layer_desc &last = p->layer[L1 - 1];
    // the optimiser kernel reduces the loss when it runs with deferred work anyway
    const bool loss_in_adam = d.train && d.defer;
    if (d.cls_fused) {
        Scope sc(p->timer, 1, n, (L1 > 1 ? 2 : 1) * last.n_out, 2 * last.n_in, st);
        GIST_TRY(gist_class_layer_f32(last.Z, last.ldz, last.W, 2 * last.n_in, last.b, p->labels, n, last.Y, last.ldy,
                                      p->dlogits, p->ldc, p->row_loss, L1 > 1 ? p->dZ : nullptr, 2 * last.n_in,
                                      d.drop ? p->p_drop : 0.f, p->seed, d.offs[L1 - 1], fl.partials[L1 - 1], n,
                                      last.n_out, 2 * last.n_in, s));
    } else {
        GIST_TRY(softmax_xent_ex("gist_sage_step", last.Y, last.ldy, logit_slabs > 1 ? fl.logit_slabs : nullptr,
                                 n * last.n_out, logit_slabs > 1 ? logit_slabs : 0, last.b, p->labels, nullptr, n, p->row_loss,
                                 loss_in_adam ? nullptr : p->loss, p->dlogits, p->ldc, n, last.n_out, st));
    }
    // a forward-phase call leaves the loss complete: its optimiser launch is another call
    if (d.split_phases && loss_in_adam) GIST_TRY(loss_finish(p->row_loss, n, n, p->loss, st));
    return GIST_OK;
}

// ---- phase 4: backward, layer by layer from the last ---------------------------------
// what a layer's backward leaves for the layer below it
struct LayerCarry {
    int64_t lnb_rows;          // > 0: the layer below got its LayerNorm backward (and that many rows of partial sums) from
                               // the reverse aggregation just launched
    ClassDwArgs dw_args;       // the class layer's weight-gradient slabs, deferred to the LayerNorm backward below it
    bool dw_pending;
};

// reverse_call under dZ_k's dropout mask: folded into the aggregation's reader (mask_in_spmm), or, for the unmasked dZ of
// a split projection, by a pass over dZ_k first (a plain layer's dZ kernel has applied it).  ln: the LayerNorm backward of
// layer k - 1 riding in this launch's store.
int reverse_aggregate(const gist_step_plan *p, const StepDecisions &d, const StepState &x, int64_t n, int k,
                      gist_stream_t s, const SpmmLnBwd *ln = nullptr) {
    const gist_layer_desc &l = p->layer[k];
    if (!d.mask_in_spmm[k] && d.drop && !d.plain[k])
        GIST_TRY(gist_dropout_f32(p->dZ, 2 * l.n_in, n, 2 * l.n_in, p->p_drop, p->seed, d.offs[k], s));
    Scope sc(p->timer, 0, n, n, l.n_in, as_stream(s));
    SpmmCall c = reverse_call(p, d, n, k, d.mask_in_spmm[k]);
    c.prepared = x.prep_bwd; c.ln = ln; c.st = as_stream(s);
    return spmm_run(c);
}

// dY_k of a hidden layer from dO_k (the left half of dZ_{k+1}), over yhat in Y_k.  *db_done: the bias gradient's chunk
// sums were written on the way.
int hidden_dy(const gist_step_plan *p, const StepDecisions &d, int64_t n, int k, LayerCarry &c, bool *db_done,
              hipStream_t st) {
    const gist_layer_desc &l = p->layer[k];
    const int64_t i_next = p->layer[k + 1].n_in;      // == l.n_out
    const float *rstd = p->use_layernorm ? l.rstd : nullptr;
    if (c.lnb_rows > 0) {      // (came with the reverse aggregation of layer k + 1)
        c.lnb_rows = 0;
        *db_done = true;
        return GIST_OK;
    }
    if (!d.defer || !d.plain[k])
        return ln_relu_bwd_ex(p->dZ, 2 * i_next, l.Y, l.ldy, rstd, l.Y, l.ldy, n, l.n_out, p->use_layernorm, 1,
                              d.h3.layer[k].on ? d.h3.rowmax : nullptr, st);
    *db_done = true;
    if (!c.dw_pending)
        return ln_relu_bwd_colsum(p->dZ, 2 * i_next, l.Y, l.ldy, rstd, l.Y, l.ldy, n, l.n_out, p->use_layernorm, 1,
                                  d.fl.partials[k], st);
    c.dw_pending = false;      // ... with the class layer's weight-gradient slabs in the same grid
    return ln_relu_bwd_colsum_class_dw(p->dZ, 2 * i_next, l.Y, l.ldy, rstd, l.Y, l.ldy, n, l.n_out, p->use_layernorm, 1,
                                       d.fl.partials[k], c.dw_args, st);
}

// layer k on kept f16x3 operands: bias gradient + column maxima of dY_k, one read of dY_k -> both split layouts
// (row maxima came from the LayerNorm backward), then dZ_k and dW_k on the splits
int backward_h3(const gist_step_plan *p, const StepDecisions &d, const StepState &x, int64_t n, int k, const float *dy,
                int64_t lddy, gist_stream_t s) {
    const gist_layer_desc &l = p->layer[k];
    const H3Step &h3 = d.h3;
    const H3Layer &hl = h3.layer[k];
    hipStream_t st = as_stream(s);
    GIST_TRY(colsum_ex(dy, lddy, n, l.n_out, p->partials, l.db, h3.pmax, h3.colmax, st));
    {
        Scope sc(p->timer, 3, 0, 0, 0, st);
        H3Dual j{};
        j.src = dy; j.ld = lddy; j.rows = n; j.cols = l.n_out;
        j.rowmax = h3.rowmax; j.colmax = h3.colmax;
        j.dst_r = k > 0 ? h3.dYs : nullptr; j.inv_r = h3.inv_dyr;
        j.dst_t = h3.dYsT; j.inv_t = h3.inv_dyt;
        GIST_TRY(h3_dual_split(j, st));
    }
    if (k > 0) {
        Scope sc(p->timer, 1, n, 2 * l.n_in, l.n_out, st);
        GIST_TRY(h3_gemm_presplit("gist_sage_step", h3.dYs, h3.inv_dyr, hl.WsT, hl.inv_wt,
                                  nullptr, p->dZ, 2 * l.n_in, n, 2 * l.n_in, l.n_out, st));
    }
    {
        Scope sc(p->timer, 1, l.n_out, 2 * l.n_in, n, st);
        GIST_TRY(h3_gemm_presplit("gist_sage_step", h3.dYsT, h3.inv_dyt, hl.ZsT, hl.inv_zt,
                                  nullptr, l.dW, 2 * l.n_in, l.n_out, 2 * l.n_in, n, st));
    }
    return k > 0 ? reverse_aggregate(p, d, x, n, k, s) : GIST_OK;
}

// layer k on kept bf16x3 operands: bias gradient, then one read of dY_k -> both split layouts, dZ_k and dW_k on the splits
int backward_b3(const gist_step_plan *p, const StepDecisions &d, StepState &x, int64_t n, int k, const float *dy,
                int64_t lddy, gist_stream_t s) {
    const gist_layer_desc &l = p->layer[k];
    const B3Step &b3 = d.b3;
    const B3Layer &hl = b3.layer[k];
    hipStream_t st = as_stream(s);
    // (fused step: the split tiles' column sums stay in the layer's own partials and the optimiser forms db_k from them
    // -- 32 sources per element, a dedicated-block segment -- instead of a 5-us reduce launch per layer)
    const bool db_in_adam = d.defer && d.fl.partials[k] != nullptr;
    {   // (the split's 64 x 64 tiles also give the bias gradient's per-chunk column sums)
        Scope sc(p->timer, 3, 0, 0, 0, st);
        B3Dual j{};
        j.src = dy; j.ld = lddy; j.rows = n; j.cols = l.n_out;
        j.dst_r = k > 0 ? b3.dYs : nullptr;
        j.dst_t = b3.dYsT;
        j.col_partials = db_in_adam ? d.fl.partials[k] : p->partials;
        GIST_TRY(b3_dual_split(j, st));
    }
    if (db_in_adam)
        add_segment(p, x, l.db, l.n_out, d.fl.partials[k], gist_colsum_partials(n));
    else
        GIST_TRY(colsum_finish(p->partials, gist_colsum_partials(n), l.n_out, l.db, st));
    if (k > 0) {
        Scope sc(p->timer, 1, n, 2 * l.n_in, l.n_out, st);
        GIST_TRY(b3_gemm_presplit("gist_sage_step", b3.dYs, hl.WsT, nullptr, p->dZ, 2 * l.n_in, n,
                                  2 * l.n_in, l.n_out, b3.slabs, b3.slab_bytes, st));
    }
    {
        Scope sc(p->timer, 1, l.n_out, 2 * l.n_in, n, st);
        // the step's LAST projection may leave its k slices to the optimiser (the slab scratch is not reused before it runs)
        int ns = 1;
        GIST_TRY(b3_gemm_presplit("gist_sage_step", b3.dYsT, hl.ZsT, nullptr, l.dW, 2 * l.n_in, l.n_out, 2 * l.n_in, n,
                                  b3.slabs, b3.slab_bytes, st, d.defer && k == 0 ? &ns : nullptr));
        if (ns > 1) add_segment(p, x, l.dW, l.n_out * 2 * l.n_in, b3.slabs, ns);
    }
    return k > 0 ? reverse_aggregate(p, d, x, n, k, s) : GIST_OK;
}

// dW_k of a plain layer: slabs for the optimiser in the fused step, gist_gemm_tn_f32 otherwise
int plain_dw(const gist_step_plan *p, const StepDecisions &d, StepState &x, int64_t n, int k, const float *dy,
             int64_t lddy, LayerCarry &c, gist_stream_t s) {
    const int L1 = p->n_layers;
    const gist_layer_desc &l = p->layer[k];
    const FusedLayout &fl = d.fl;
    hipStream_t st = as_stream(s);
    const bool cls = d.cls_fused && k == L1 - 1;
    // The class layer's weight-gradient slabs need dlogits and the layer's input only; the LayerNorm backward of
    // the layer below (next in the backward loop, behind the reverse aggregation) runs 128 workgroups for ~6 us:
    // the slabs' workgroups go into ITS grid (ln_relu_bwd_cs_dw_kernel) -- one launch fewer per step
    const bool dw_with_ln = cls && L1 >= 2 && d.defer && d.plain[L1 - 2] && (int)tune(GIST_TUNE_CLASS_FUSED) != 2;
    Scope sc(dw_with_ln ? nullptr : p->timer, 1, l.n_out, 2 * l.n_in, n, st);
    if (cls) {
        int32_t ns = 1;
        if (dw_with_ln) {
            GIST_TRY(class_dw_args("gist_sage_step", dy, lddy, l.Z, l.ldz, fl.dw_slabs[k], fl.dw_bytes[k], n, l.n_out,
                                   2 * l.n_in, &c.dw_args, &ns));
            c.dw_pending = true;
        } else {
            GIST_TRY(gist_class_dw_slabs_f32(dy, lddy, l.Z, l.ldz, fl.dw_slabs[k], fl.dw_bytes[k], &ns, n, l.n_out,
                                             2 * l.n_in, s));
        }
        add_segment(p, x, l.dW, l.n_out * 2 * l.n_in, fl.dw_slabs[k], ns);
    } else if (d.defer && fl.dw_slabs[k] != nullptr) {      // the optimiser sums the slabs
        int ns = 1;
        GIST_TRY(gemm_slabs(2, dy, lddy, l.Z, l.ldz, nullptr, l.dW, 2 * l.n_in, l.n_out, 2 * l.n_in, n,
                            fl.dw_slabs[k], fl.dw_bytes[k], &ns, st, GEMM_CALL_SLABS));
        if (ns > 1) add_segment(p, x, l.dW, l.n_out * 2 * l.n_in, fl.dw_slabs[k], ns);
    } else {
        GIST_TRY(gist_gemm_tn_f32(dy, lddy, l.Z, l.ldz, l.dW, 2 * l.n_in, l.n_out, 2 * l.n_in, n, p->workspace,
                                  p->workspace_bytes, s));
    }
    return GIST_OK;
}

// layer k on the fp32 / per-call-split projections.  db_done: dY_k's chunk sums (db_rows rows of them) are written
int backward_plain(const gist_step_plan *p, const StepDecisions &d, StepState &x, int64_t n, int k, const float *dy,
                   int64_t lddy, bool db_done, int64_t db_rows, LayerCarry &c, gist_stream_t s) {
    const int L1 = p->n_layers;
    const gist_layer_desc &l = p->layer[k];
    const FusedLayout &fl = d.fl;
    hipStream_t st = as_stream(s);
    // dZ_k and dW_k of a narrow hidden layer read the same dY_k: one launch of the fp32 kernel's tiles for both
    // (gist_gemm_nn_tn_dual_f32) when the mask of dZ_k is the reverse aggregation's business anyway
    if (d.defer && k > 0 && k < L1 - 1 && db_done && (!d.drop || d.mask_in_spmm[k]) &&
        gemm_dual_takes(n, 2 * l.n_in, l.n_out, lddy, 2 * l.n_in, l.ldz, 2 * l.n_in, dy, l.W, l.Z, p->dZ)) {
        Scope sc(p->timer, 1, n, 4 * l.n_in, l.n_out, st);
        int ns = 1;
        GIST_TRY(gemm_dual_nn_tn("gist_sage_step", dy, lddy, l.W, 2 * l.n_in, p->dZ, 2 * l.n_in, l.Z, l.ldz, l.dW,
                                 2 * l.n_in, n, 2 * l.n_in, l.n_out, fl.dw_slabs[k], fl.dw_bytes[k], &ns, st));
        if (ns > 1) add_segment(p, x, l.dW, l.n_out * 2 * l.n_in, fl.dw_slabs[k], ns);
    } else {
        // GIST_STEP_DLOGITS_GIVEN: plan->dlogits was written by the caller (any loss on the logits): the class layer's dZ
        // and bias chunk sums of the fused forward belong to ANOTHER dlogits and are recomputed from the given one
        if (d.cls_fused && !d.dlogits_given && k == L1 - 1) {
            db_done = true;      // (dZ and the bias chunks came with the loss)
        } else if (k > 0) {      // dZ with its dropout mask (or the mask left to the reverse aggregation)
            Scope sc(p->timer, 1, n, 2 * l.n_in, l.n_out, st);
            const bool chunk_db = d.defer && k == L1 - 1;      // the class layer's dZ kernel sees dlogits in 16-row chunks
            GIST_TRY(gemm_nn_dropout_ex("gist_sage_step", dy, lddy, l.W, 2 * l.n_in, p->dZ, 2 * l.n_in, n,
                                        2 * l.n_in, l.n_out, (d.drop && !d.mask_in_spmm[k]) ? p->p_drop : 0.f, p->seed,
                                        d.offs[k], p->workspace, p->workspace_bytes,
                                        chunk_db ? fl.partials[k] : nullptr, st));
            db_done = db_done || chunk_db;
        }
        GIST_TRY(plain_dw(p, d, x, n, k, dy, lddy, c, s));
    }
    if (d.defer) {      // db_k = chunk sums, formed by the optimiser
        if (!db_done)      // (a one-layer model: no dZ kernel has seen dlogits)
            GIST_TRY(colsum_rows16(dy, lddy, n, l.n_out, fl.partials[k], k == L1 - 1 ? false : true, st));
        add_segment(p, x, l.db, l.n_out, fl.partials[k], db_rows);
    } else {
        GIST_TRY(gist_colsum_f32(dy, lddy, n, l.n_out, p->partials, l.db, s));
    }
    if (k == 0) return GIST_OK;
    if (!d.mask_in_spmm[k]) return reverse_aggregate(p, d, x, n, k, s);
    // the LayerNorm + ReLU backward of layer k - 1 in the aggregation's store (its rows are whole in one wave)
    const gist_layer_desc &lo = p->layer[k - 1];
    const int64_t units = d.blocked ? spmm_lnb_units(p->n_row_blocks) : 0;
    const SpmmLnBwd ln{lo.Y, lo.ldy, p->use_layernorm ? lo.rstd : nullptr, lo.Y, lo.ldy, fl.partials[k - 1], 1};
    SpmmCall ask = reverse_call(p, d, n, k, true);      // can the call carry it?
    ask.prepared = x.prep_bwd; ask.ln = &ln;
    const bool with_ln = d.defer && d.plain[k - 1] && !c.dw_pending && (int)tune(GIST_TUNE_LNB_FUSED) != 1 &&
                         units > 0 && units <= fl.partial_rows[k - 1] && (!p->use_layernorm || lo.rstd != nullptr) &&
                         spmm_choose(ask).refusal == nullptr;
    if (with_ln) c.lnb_rows = units;
    return reverse_aggregate(p, d, x, n, k, s, with_ln ? &ln : nullptr);
}

int backward(const gist_step_plan *p, const StepDecisions &d, StepState &x, int64_t n, gist_stream_t s) {
    const int L1 = p->n_layers;
    const int64_t chunks16 = gist_row_chunks16(n);
    LayerCarry c{};
    for (int k = L1 - 1; k >= 0; --k) {
        const gist_layer_desc &l = p->layer[k];
        const float *dy = k == L1 - 1 ? p->dlogits : l.Y;
        const int64_t lddy = k == L1 - 1 ? p->ldc : l.ldy;
        bool db_done = false;      // this layer's bias gradient is already in chunks
        const int64_t db_rows = c.lnb_rows > 0 ? c.lnb_rows : chunks16;
        if (k < L1 - 1) GIST_TRY(hidden_dy(p, d, n, k, c, &db_done, as_stream(s)));
        if (d.h3.layer[k].on)
            GIST_TRY(backward_h3(p, d, x, n, k, dy, lddy, s));
        else if (d.b3.layer[k].on)
            GIST_TRY(backward_b3(p, d, x, n, k, dy, lddy, s));
        else
            GIST_TRY(backward_plain(p, d, x, n, k, dy, lddy, db_done, db_rows, c, s));
    }
    GIST_REQUIRE(!c.dw_pending, "gist_sage_step: internal error (class-layer weight gradient not launched)");
    // without the optimiser phase the gradient arena is complete on return (p.grad is read by the caller's optimiser,
    // possibly by its own code first): the deferred sums in the optimiser's order, without the update
    if (!d.do_opt && d.defer && x.n_segs > 0)
        GIST_TRY(gist_grad_segments_finish_f32(p->grads, p->n_params, x.segs, x.n_segs, s));
    return GIST_OK;
}

// ---- phase 5: the optimiser, with the NEXT batch's extraction in its grid when asked and possible ---------------
struct AdamArgs { float lr, beta1, beta2, eps, weight_decay; int64_t step; };

int optimise(const gist_step_plan *p, const StepDecisions &d, const StepState &x, int64_t n, const AdamArgs &a, int flags,
             gist_stream_t s) {
    // (an optimiser-phase call has no segments -- the backward-phase call finished the gradients -- and no loss to
    // reduce: the forward-phase call did)
    const float *row_loss = d.do_bwd || !d.split_phases ? p->row_loss : nullptr;
    if ((flags & GIST_STEP_EXTRACT_NEXT) && prefetches_next(p, d)) {      // nothing reads the batch buffers any more
        const gist_extract_parts_desc next =
            sage_parts_desc(p, d, p->next_ids, p->next_n, p->next_batch_index, p->next_drop_offset);
        return gist_adam_segments_extract_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, a.lr, a.beta1,
                                              a.beta2, a.eps, a.weight_decay, a.step, x.segs, x.n_segs, row_loss, n, n,
                                              p->loss, &next, s);
    }
    if (d.defer)
        return gist_adam_segments_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, a.lr, a.beta1, a.beta2,
                                      a.eps, a.weight_decay, a.step, x.segs, x.n_segs, row_loss, n, n, p->loss, s);
    return gist_adam_f32(p->params, p->grads, p->exp_avg, p->exp_avg_sq, p->n_params, a.lr, a.beta1, a.beta2, a.eps,
                         a.weight_decay, a.step, s);
}
}  // namespace

extern "C" int gist_sage_step_extracts_next(const gist_step_plan *p, int64_t n, int flags) {
    if (p == nullptr || !(flags & GIST_STEP_TRAIN) || n <= 0 || p->n_layers < 1 || p->n_layers > GIST_MAX_LAYERS) return 0;
    return prefetches_next(p, decide(p, n, 0, flags)) ? 1 : 0;
}

extern "C" int gist_sage_step(const gist_step_plan *p, const int32_t *ids, int64_t n, uint64_t drop_offset, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int64_t adam_step, int flags,
                              gist_stream_t s) {
    // ---- validation: all of it before any device work -------------------------------------------------
    GIST_REQUIRE(p != nullptr, "gist_sage_step: null plan");
    GIST_REQUIRE(p->n_layers >= 1 && p->n_layers <= GIST_MAX_LAYERS, "gist_sage_step: bad n_layers");
    GIST_REQUIRE(n > 0, "gist_sage_step: empty batch");
    GIST_REQUIRE(!((flags & GIST_STEP_EXTRACT) && (flags & GIST_STEP_PREEXTRACTED)),
                 "gist_sage_step: GIST_STEP_EXTRACT and GIST_STEP_PREEXTRACTED exclude each other");
    GIST_REQUIRE(!(flags & (GIST_STEP_EXTRACT_NEXT | GIST_STEP_PREEXTRACTED)) || (flags & GIST_STEP_TRAIN),
                 "gist_sage_step: GIST_STEP_EXTRACT_NEXT / GIST_STEP_PREEXTRACTED belong to training steps");
    const int phases = flags & kPhaseBits;
    GIST_REQUIRE(phases == 0 || (flags & GIST_STEP_TRAIN), "gist_sage_step: GIST_STEP_PHASE_* belong to training steps");
    GIST_REQUIRE(!(flags & GIST_STEP_DLOGITS_GIVEN) || phases == GIST_STEP_PHASE_BACKWARD,
                 "gist_sage_step: GIST_STEP_DLOGITS_GIVEN belongs to a GIST_STEP_PHASE_BACKWARD call");
    GIST_REQUIRE(__builtin_popcount(phases) != 2, "gist_sage_step: one GIST_STEP_PHASE_* per call (or none / all three)");
    const bool extracts = (flags & GIST_STEP_EXTRACT) && (phases == 0 || (phases & GIST_STEP_PHASE_FORWARD));
    GIST_REQUIRE(!extracts || ids != nullptr, "gist_sage_step: null ids");

    const StepDecisions d = decide(p, n, drop_offset, flags);
    StepState x{};
    ActiveTimer active(p->timer);
    if (d.do_fwd) GIST_TRY(split_weights(p, d, as_stream(s)));
    GIST_TRY(extract_and_prepare(p, d, x, ids, n, flags, s));
    if (d.do_fwd) GIST_TRY(forward(p, d, x, n, s));
    if (d.do_bwd) GIST_TRY(backward(p, d, x, n, s));
    if (d.do_opt) GIST_TRY(optimise(p, d, x, n, AdamArgs{lr, beta1, beta2, eps, weight_decay, adam_step}, flags, s));
    return GIST_OK;
}
