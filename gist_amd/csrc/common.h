// Shared helpers for libgist_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/gist_hip.h"
#include "dropout.h"
#include "gemm_plan.h"
#include "kernel_kit.h"      // the device primitives the kernels share (wave_sum, the tile map, the C-tile store, ...)

namespace gist {

constexpr int kWave = 64;

void set_error(const char *fmt, ...);

static inline hipStream_t as_stream(gist_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Kernel launches issued by this process through the library (gist_launch_count): a measurement aid -- the launch count
// of a step, next to the cost of as many EMPTY launches (gist_empty_launches), is the floor of a launch-bound step.
extern std::atomic<uint64_t> g_launches;

// Checks the launch itself (not completion): calls stay asynchronous.
static inline int launch_status(const char *what) {
    g_launches.fetch_add(1, std::memory_order_relaxed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return GIST_ELAUNCH;
    }
    return GIST_OK;
}

#define GIST_REQUIRE(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            gist::set_error(__VA_ARGS__);  \
            return GIST_EINVAL;            \
        }                                  \
    } while (0)

// HIP-event timer of the native step driver (step.hip).  While gist_sage_step runs with a timer
// armed, tl_timer points at it so that a kernel below an entry point (the split GEMM's main
// kernel) can be bracketed on its own: slot = timer_begin(...); launch; timer_end(slot).
extern thread_local gist_timer *tl_timer;
int64_t timer_begin(gist_timer *t, int kind, int64_t m, int64_t n, int64_t k, hipStream_t s);
void timer_end(gist_timer *t, int64_t slot, hipStream_t s);

// The projection family.  How a projection runs -- path, tile, k slices, tail units, scratch -- is plan_gemm()'s answer
// (gemm_plan.h); what follows are the launchers that read it and the pre-passes.
// gemm_h3.hip: building blocks of the split projection path for a caller that manages the
// split operands itself (the step driver).  Split operand = [rows][h3_kpad(k)] 32-bit words
// + one inverse scale (power of two) per row.
struct H3Dual {                       // one read of src[rows, cols] -> up to two split operands
    const float *src; int64_t ld; int64_t rows, cols;
    float p; uint64_t seed, offset;   // dropout applied on the fly (p = 0: none), gist_dropout_f32's stream
    int fixed_shift;                  // uniform scale 2^fixed_shift ...
    const unsigned *amax;             // ... or, if not NULL, from the tensor's max |x| (float bits)
    const float *rowmax, *colmax;     // if not NULL: per-row / per-column maxima instead
    uint32_t *dst_r; float *inv_r;    // [rows][kpad(cols)]: k = columns of src   (NULL: skip)
    uint32_t *dst_t; float *inv_t;    // [cols][kpad(rows)]: k = rows of src      (NULL: skip)
};
int h3_dual_split(const H3Dual &d, hipStream_t st);
int h3_split_rows(const float *src, int64_t ld, int64_t rows, int64_t k, uint32_t *dst, float *inv,
                  hipStream_t st);
int h3_absmax(const float *src, int64_t ld, int64_t rows, int64_t cols, unsigned *out, hipStream_t st);
int h3_gemm_presplit(const char *name, const uint32_t *sa, const float *inv_a, const uint32_t *sb,
                     const float *inv_b, const float *bias, float *c, int64_t ldc, int64_t m,
                     int64_t n, int64_t k, hipStream_t st);

// gemm_b3.hip: the bf16x3 split projection path (all 24 operand bits, no scales).  Split operand =
// [rows][b3_kpad(k)] elements of 6 bytes (three bf16 pieces per element, 16-byte chunks per 8 k).
struct B3Dual {                       // one read of src[rows, cols] -> up to two split operands
    const float *src; int64_t ld; int64_t rows, cols;
    float p; uint64_t seed, offset;   // dropout applied on the fly (p = 0: none), gist_dropout_f32's stream
    uint16_t *dst_r;                  // [rows][kpad(cols)]: k = columns of src   (NULL: skip)
    uint16_t *dst_t;                  // [cols][kpad(rows)]: k = rows of src      (NULL: skip)
    float *col_partials;              // [ceil(rows / 64)][cols] column sums per 64-row chunk of src (NULL: none):
                                      // the first stage of gist_colsum_f32, taken from the tile the split reads anyway
    bool vec4;                        // set by the launcher: 16-byte loads allowed
};
int b3_dual_split(const B3Dual &d, hipStream_t st);
constexpr int B3_SPLIT_MAX_JOBS = 4;
int b3_split_jobs(const B3Dual *jobs, int n_jobs, hipStream_t st);      // up to B3_SPLIT_MAX_JOBS splits, one launch
// (slabs: the scratch of the GEMM_CALL_KEPT plan -- fp32 slabs of the k slices or the tail units' partials)
int b3_gemm_presplit(const char *name, const uint16_t *sa, const uint16_t *sb, const float *bias, float *c,
                     int64_t ldc, int64_t m, int64_t n, int64_t k, float *slabs, int64_t slab_bytes,
                     hipStream_t st, int *deferred = nullptr);
// gemm.hip: gist_gemm_{nt,nn,tn}_f32 (layout 0, 1, 2) whose split-K partial sums stay as dense slabs
// [*n_slabs][m][n] at `slabs` for the consumer to sum in slab order (+ bias); *n_slabs = 1: c is final
int gemm_slabs(int layout, const float *a, int64_t lda, const float *b, int64_t ldb, const float *bias, float *c,
               int64_t ldc, int64_t m, int64_t n, int64_t k, void *slabs, int64_t slab_bytes, int *n_slabs,
               hipStream_t st, GemmCall call = GEMM_CALL_SPLITS);      // GEMM_CALL_SLABS: `slabs` was sized by gemm_slab_bytes
// gemm.hip: gist_gemm_nn_f32 for a caller with an epilogue of its own (in GEMM mode 3 it keeps the fp32 kernel)
int gemm_nn_epilogue_call(const float *g, int64_t ldg, const float *w, int64_t ldw, float *z, int64_t ldz,
                          int64_t m, int64_t n, int64_t k, void *workspace, int64_t workspace_bytes, hipStream_t st);
// gemm.hip: dz = dy . w (NN) and dW = dy^T . z (TN, slabs) in one launch of the fp32 kernel's tiles
bool gemm_dual_takes(int64_t m, int64_t n1, int64_t k1, int64_t lddy, int64_t ldw, int64_t ldz, int64_t lddz,
                     const float *dy, const float *w, const float *z, const float *dz);
int gemm_dual_nn_tn(const char *name, const float *dy, int64_t lddy, const float *w, int64_t ldw, float *dz,
                    int64_t lddz, const float *z, int64_t ldz, float *dw, int64_t lddw, int64_t m, int64_t n1,
                    int64_t k1, void *slabs, int64_t slab_bytes, int *n_slabs, hipStream_t st);
// gemm.hip: c[m, n] (ldc) = sum of `splits` dense slabs [m][n] + bias
int splitk_reduce(const char *name, const float *slabs, int64_t slab, int splits, const float *bias, float *c,
                  int64_t ldc, int64_t m, int64_t n, hipStream_t st);

// spmm.hip: dropout folded into an aggregation (gist_spmm_csr_drop_f32); element (row, c) of y has mask
// index y_base + row * ld + c, of x src_base + row * ld + c
struct SpmmDrop {
    int mode;                 // 0 none, 1 forward (mask what is stored), 2 backward (mask x and the old y)
    DropMask m;
    uint64_t y_base, src_base;
    int64_t ld;
};
// LayerNorm + ReLU backward of the layer BELOW in the store of a reverse aggregation (mode 2, d <= 256: a wave holds a
// whole row): what would be stored is d_out of that layer's output; dy = rstd . (g - mean(g) - yhat . mean(g . yhat)),
// g = d_out . [yhat > 0], goes to `dy` (may be `yhat` itself), nothing to y; col_partials[unit][0..d) = the column sums of
// the dy rows one workgroup stored (spmm_lnb_units(n_row_blocks) rows: the bias gradient's partial sums)
struct SpmmLnBwd {
    const float *yhat; int64_t ldy;
    const float *rstd;            // NULL: no LayerNorm (dy = g)
    float *dy; int64_t lddy;
    float *col_partials;
    int relu;
};
// gist_spmm_csr_drop_f32's arguments as a SpmmDrop (a mode other than 1 and 2 becomes -1, which spmm_run refuses)
static inline SpmmDrop spmm_drop_of(int mode, float p, uint64_t seed, uint64_t y_offset, uint64_t src_offset, int64_t ld) {
    SpmmDrop dr{};
    dr.mode = (mode == 1 || mode == 2) ? mode : -1; dr.m = drop_mask_of(p, seed);
    dr.y_base = y_offset; dr.src_base = src_offset; dr.ld = ld;
    return dr;
}
// rows of x and y start on 16-byte boundaries and are whole float4s
static inline bool spmm_rows16(int64_t d, int64_t ldx, int64_t ldy, const float *x, const float *y) {
    return d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(x) && aligned16(y);
}
// blocks of a blocked aggregation: the caller's, or uniform blocks of 128 rows (kL2Rows, MF_ROWS)
static inline int64_t spmm_block_count(const int32_t *row_blocks, int64_t n_row_blocks, int64_t n_rows) {
    return row_blocks ? n_row_blocks : ceil_div(n_rows, 128);
}
// One aggregation call y (+)= out_scale . A . (src_scale . x), as every function between a C entry point (or the step)
// and a kernel launch sees it.  Aggregate order: entry .. accumulate are the leading arguments of the C entry points.
enum SpmmBlocks { SPMM_BLOCKS_NONE, SPMM_BLOCKS_UNIFORM, SPMM_BLOCKS_GIVEN };
struct SpmmCall {
    const char *entry;                // the entry point that was called, for error texts
    const int32_t *rowptr, *col; int64_t n_rows;
    const float *x; int64_t ldx;
    float *y; int64_t ldy;
    int64_t d;
    const float *out_scale, *src_scale;
    int accumulate;
    SpmmBlocks blocks;                // NONE: the plain entry, a drop entry without row_blocks; UNIFORM: the blocked and
    const int32_t *row_blocks;        // prepared entries without row_blocks; GIVEN: row_blocks[0 .. n_row_blocks]
    int64_t n_row_blocks;
    const void *prepared;             // the blocks' prepared structure (gist_spmm_blocks_prepare), or NULL
    bool need_prepared;               // gist_spmm_csr_prepared_f32: prepared == NULL is a null-pointer error
    bool pairs;                       // may the batch have sibling blocks (launch_spmm_mfma)
    SpmmDrop dr;                      // mode 0: none
    const SpmmLnBwd *ln;              // NULL: none
    hipStream_t st;
    void set_blocks(const int32_t *rb, int64_t nb, SpmmBlocks without) {
        blocks = rb ? SPMM_BLOCKS_GIVEN : without; row_blocks = rb; n_row_blocks = nb;
    }
    bool rows16() const { return spmm_rows16(d, ldx, ldy, x, y); }
    int64_t n_blocks() const { return spmm_block_count(row_blocks, n_row_blocks, n_rows); }
};
// Which kernel family runs a call (spmm.hip: the decision table is above spmm_choose), and the one path from a record
// to a launch: validate, choose, launch.
enum SpmmKernel { SPMM_ROWS, SPMM_LDS2, SPMM_MFMA, SPMM_DENSE32 };      // ROWS: the lane-group / row-split kernels
struct SpmmChoice {
    SpmmKernel kernel;
    bool reads_prepared;
    const char *refusal;              // not NULL: the call is refused (GIST_EINVAL) with this text
};
SpmmChoice spmm_choose(const SpmmCall &c);
int spmm_run(const SpmmCall &c);
int64_t spmm_lnb_units(int64_t n_row_blocks);      // partial rows a call with SpmmLnBwd writes
// spmm_mfma.hip: the block-dense aggregation kernel behind gist_spmm_csr_blocked_f32 / _prepared_f32
// (prepared = NULL: every workgroup builds its block's counts itself).  pairs: may the batch have sibling blocks?  false
// (gist_sage_step with plan->sibling_parts == 0): the prepare kernel looks for none and no pairs launch follows an
// aggregation; a structure prepared either way is read correctly either way (spmm_prep.h), the choice is speed only.
int launch_spmm_mfma(const SpmmCall &c, const void *prepared);
int64_t spmm_blocks_bytes(int64_t n_blocks);
// spmm_dense32.hip: the block-dense aggregation on the fp32 matrix cores, operands from memory (prepared blocks only)
bool spmm_dense32_takes(int64_t d, int64_t ldx, int64_t ldy);
int launch_spmm_dense32(const SpmmCall &c);
bool spmm_prepared_takes(int64_t d, int64_t ldx, int64_t ldy, const float *x, const float *y);   // spmm.hip
int launch_spmm_blocks_prepare(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr2,
                               const int32_t *col2, int64_t n_rows, const int32_t *row_blocks,
                               int64_t n_row_blocks, void *prepared, void *prepared2, hipStream_t st, bool pairs = true);

// rowops.hip: the C-ABI kernels with the extra outputs the split projection path consumes
int ln_relu_bwd_ex(const float *d_out, int64_t ldg, const float *yhat, int64_t ldy, const float *rstd,
                   float *dy, int64_t lddy, int64_t n_rows, int64_t d, int use_lynorm, int relu,
                   float *rowmax, hipStream_t st);
int colsum_ex(const float *g, int64_t ldg, int64_t n_rows, int64_t d, float *partials, float *out,
              float *pmax, float *outmax, hipStream_t st);
// second stage alone: out[d] = sum over `chunks` rows of partials[chunks][d], fixed order
int colsum_finish(const float *partials, int64_t chunks, int64_t d, float *out, hipStream_t st);
// rowops.hip: the fused producers of "column sums per 16-row chunk" and their consumers
int ln_relu_bwd_colsum(const float *d_out, int64_t ldg, const float *yhat, int64_t ldy, const float *rstd,
                       float *dy, int64_t lddy, int64_t n_rows, int64_t d, int use_lynorm, int relu,
                       float *col_partials, hipStream_t st);
struct ClassDwArgs;
int ln_relu_bwd_colsum_class_dw(const float *d_out, int64_t ldg, const float *yhat, int64_t ldy, const float *rstd,
                                float *dy, int64_t lddy, int64_t n_rows, int64_t d, int use_lynorm, int relu,
                                float *col_partials, const ClassDwArgs &dw, hipStream_t st);
int gemm_nn_dropout_ex(const char *name, const float *g, int64_t ldg, const float *w, int64_t ldw, float *z,
                       int64_t ldz, int64_t m, int64_t n, int64_t k, float p, uint64_t seed, uint64_t offset,
                       void *workspace, int64_t workspace_bytes, float *dy_col_partials, hipStream_t st);
int softmax_xent_ex(const char *name, float *logits, int64_t ldl, const float *slabs, int64_t slab_stride,
                    int n_slabs, const float *bias, const int32_t *labels, const uint8_t *mask, int64_t count,
                    float *row_loss, float *loss, float *d_logits, int64_t ldg, int64_t n_rows,
                    int64_t n_classes, hipStream_t st);
int colsum_rows16(const float *g, int64_t ldg, int64_t n_rows, int64_t d, float *partials, bool interleaved,
                  hipStream_t st);
// loss[0] = sum(row_loss[0..n_rows)) / count, the reduction gist_adam_segments_f32 performs, as its own launch
int loss_finish(const float *row_loss, int64_t n_rows, int64_t count, float *loss, hipStream_t st);

// Tuning hooks (gist_tuning_set, include/gist_hip.h): explicit process-wide overrides of the
// launchers' own choices, for sweeps and for tests that must reach both variants of a kernel.
// 0 = the launcher decides.  The library never reads the environment on a launch path.
double tune(int knob);

// Per-device one-time setup (hipFuncSetAttribute applies to the current device only).  Usage:
//   static DeviceOnce once;  int dev;  if (once.needed(&dev)) { ...set...; once.done(dev); }
// Racing threads may both run the setup, which is idempotent.
struct DeviceOnce {
    std::atomic<uint64_t> mask{0};
    bool needed(int *dev) {
        if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev > 63) { *dev = -1; return true; }
        return ((mask.load(std::memory_order_acquire) >> *dev) & 1ULL) == 0;
    }
    void done(int dev) {
        if (dev >= 0) mask.fetch_or(1ULL << dev, std::memory_order_release);
    }
};

}  // namespace gist
