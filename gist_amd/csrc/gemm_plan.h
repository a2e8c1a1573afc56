// How one projection of the GEMM family runs (gemm.hip, gemm_h3.hip, gemm_b3.hip, gemm_b3c.hip): decided ONCE, by
// plan_gemm(), from the shape and the circumstances of the call.  The size queries read a plan made with unbounded
// scratch, the launchers one made with the scratch they were given: both see the same path, tile, k slices and tail units.
// Host code only (gemm_plan.cpp); tested without a GPU through gist_gemm_plan_query.
#pragma once
#include <stdint.h>

#include "../../include/gist_hip.h"

namespace gist {

int gemm_mode();                      // 0 fp32 MFMA, 1 f16x3, 2 bf16x3, 3 bf16x1 (gist_gemm_set_mode; GIST_GEMM_MODE at first use)

// geometry of the kernels that the planner and the callers that lay out split operands share
constexpr int H3_T = 128;             // f16x3: block tile edge (A tile 64 or 128 rows)
constexpr int H3_BK = 32;             // f16x3: k per tile = 32-bit words per image row
constexpr int B3_TM = 256, B3_TN = 128, B3_BK = 32;      // bf16x3: tile, k per tile
constexpr int B3W_TN = 256;           // bf16x3: columns of the 256 x 256 tile
constexpr int B3_CUS = 256;           // one 512-thread bf16x3 workgroup per CU
constexpr int C3_BK = 32;             // convert-on-load: k per tile
// split operand = [rows][kpad(k)] elements: f16x3 32-bit words (+ one scale per row), bf16x3 6 bytes
static inline int64_t h3_kpad(int64_t k) { return (k + H3_BK - 1) / H3_BK * H3_BK; }
static inline int64_t b3_kpad(int64_t k) { return (k + 2 * B3_BK - 1) / (2 * B3_BK) * (2 * B3_BK); }   // an even number of k tiles
// bf16x1 (gemm_bf16.hip): operand image = [rows][x1_kpad(k)] bf16, zeros past k; 128 x 128 tile, 64 k per tile
constexpr int X1_T = 128, X1_BK = 64;
static inline int64_t x1_kpad(int64_t k) { return (k + X1_BK - 1) / X1_BK * X1_BK; }

// (paths and kinds of call: include/gist_hip.h, GIST_GEMM_PATH_* and GIST_GEMM_CALL_*)
enum GemmPath { GEMM_PATH_F32, GEMM_PATH_H3, GEMM_PATH_B3, GEMM_PATH_B3C, GEMM_PATH_BF16X1 };
enum GemmCall { GEMM_CALL_SPLITS, GEMM_CALL_KEPT, GEMM_CALL_SLABS };
constexpr int64_t kScratchUnbounded = -1;

struct GemmQuery {
    bool a_kc, b_kc;                  // A: a_kc ? [m][k] : [k][m];  B: b_kc ? [n][k] : [k][n]   (NT 1 1, NN 1 0, TN 0 0)
    int64_t m, n, k;
    int mode;                         // gemm_mode(), or the mode a layout is sized for
    bool aligned;                     // both operands 16-byte aligned, both leading dimensions multiples of 4 and >= 4
    int64_t ldc;                      // of the output (the bf16x3 tiles limit it: 256 rows x ldc in 32-bit byte offsets); 0: any
    GemmCall call;
    bool deferred;                    // k slices may stay slabs for the consumer to sum (no reduce launch)
    int64_t scratch;                  // bytes on hand (a null workspace: 0), kScratchUnbounded for a size query
    bool scratch_aligned;             // the workspace is 16-byte aligned
};

using GemmPlan = gist_gemm_plan;      // the record (include/gist_hip.h): path, tile, slices, tail units, bytes, launches

GemmPlan plan_gemm(const GemmQuery &q);
static inline GemmQuery gemm_query(int layout, int64_t m, int64_t n, int64_t k, int mode, GemmCall call, bool deferred,
                                   bool aligned = true, int64_t scratch = kScratchUnbounded) {
    return GemmQuery{layout != 2, layout == 0, m, n, k, mode, aligned, 0, call, deferred, scratch, true};
}
static inline bool splits_operands(const GemmPlan &p) { return p.operand_bytes > 0; }

// dz = dy . w (NN, m x n1 x k1) and dW = dy^T . z (TN, k1 x n1 x m, slabs) as ONE launch of the fp32 kernel's 64 x 64 tiles:
// taken when both run on those tiles anyway and together fit ~one round of the chip's workgroup slots
struct GemmDualPlan { bool takes; int splits; int64_t k_per_split; };
GemmDualPlan plan_gemm_dual(int64_t m, int64_t n1, int64_t k1, int mode, int64_t scratch);

// slab bytes of a projection whose k slices are left to its consumer (a GEMM_CALL_SLABS call, operands aligned or not)
int64_t gemm_slab_bytes(int layout, int64_t m, int64_t n, int64_t k, int mode);

}  // namespace gist
