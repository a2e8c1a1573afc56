// plan_gemm(): the one place that decides how a projection runs (gemm_plan.h).  The rules below were the launchers' and
// the size queries' own; their thresholds and tuning hooks (GIST_TUNE_*, 0 = the function decides) are unchanged.
#include "gemm_plan.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>

#include "common.h"

namespace gist {

static_assert(GEMM_PATH_B3C == GIST_GEMM_PATH_BF16X3_LOAD && GEMM_CALL_SLABS == GIST_GEMM_CALL_SLABS &&
                  GEMM_PATH_BF16X1 == GIST_GEMM_PATH_BF16X1,
              "gemm_plan.h's enums are gist_hip.h's codes");

// ---- the process-wide mode ---------------------------------------------------------------------------
static std::atomic<int> g_gemm_mode{-1};      // -1: read GIST_GEMM_MODE on first use

int gemm_mode() {
    int m = g_gemm_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        const char *e = getenv("GIST_GEMM_MODE");
        // default: large projections as three bf16 pieces per operand (all 24 bits, six cross terms:
        // error at the fp32-MFMA kernel's level, gemm_b3.hip), everything else fp32 MFMA
        m = 2;
        if (e && (!strcmp(e, "f32") || !strcmp(e, "0"))) m = 0;
        else if (e && (!strcmp(e, "f16x3") || !strcmp(e, "1"))) m = 1;
        else if (e && (!strcmp(e, "bf16x3") || !strcmp(e, "2"))) m = 2;
        else if (e && (!strcmp(e, "bf16x1") || !strcmp(e, "3"))) m = 3;
        int expected = -1;
        g_gemm_mode.compare_exchange_strong(expected, m, std::memory_order_relaxed);
        m = g_gemm_mode.load(std::memory_order_relaxed);
    }
    return m;
}

namespace {

bool fits(const GemmQuery &q, int64_t bytes) { return q.scratch < 0 || q.scratch >= bytes; }

// ---- fp32 kernel: tile / split-K choice ----------------------------------------------------------------
// Everything here is fp32 MFMA work, so time ~ MFMA work of the busiest SIMD.  A block is 4
// waves (one per SIMD of a CU); blocks are dealt round-robin to 256 CUs, a CU keeps up to
// `cap` of them resident (128-tile: 2, 64-tile: 4) and fewer co-resident waves hide less
// latency.  Model, in units of one 64x64x32 MFMA block (16 MFMAs, ~0.43 us), calibrated on
// scripts/gemm_sweep.py measurements (MI355X, 34 shapes, within ~10% of the best config):
//   per_cu  = ceil(blocks / 256)
//   cost    = per_cu * unit(tile) * (k_tiles_per_split + 3) / eff(min(cap, per_cu))
//           + [splits > 1] * (12 + 6.5 * splits * m*n/1e6)      (slab traffic + reduce launch)
struct GemmCfg { int tile; int splits; };

// deferred: the k slices are summed by the kernel that consumes the result (gist_gemm_slabs_f32) -- no reduce
// launch, only the slabs' write and read.
GemmCfg choose_cfg(int64_t m, int64_t n, int64_t k, bool deferred = false) {
    const int64_t kt = ceil_div(k, 32);      // the model counts k in units of 32
    // explicit override for tuning sweeps (scripts/gemm_sweep.py) and tests; 0 = the model decides
    const int t_tile = (int)tune(GIST_TUNE_GEMM_TILE), t_split = (int)tune(GIST_TUNE_GEMM_SPLITS);
    if (t_tile && t_split) {
        int sp = t_split;
        while (sp > 1 && kt / sp < 1) sp >>= 1;
        return GemmCfg{t_tile == 64 ? 64 : 128, sp < 1 ? 1 : sp};
    }
    static const double eff128[3] = {0.0, 0.90, 1.00};
    static const double eff64[5] = {0.0, 0.60, 0.80, 0.92, 1.00};
    GemmCfg best{128, 1};
    double best_cost = 1e300;
    const double mn = (double)m * (double)n / 1e6;
    for (int tile : {128, 64}) {
        const int64_t tiles = ceil_div(m, tile) * ceil_div(n, tile);
        const int cap = tile == 128 ? 2 : 4;
        const double unit = tile == 128 ? 4.0 : 1.12;
        for (int sp : {1, 2, 4, 8, 16, 32}) {
            if (sp > 1 && kt / sp < 2) break;
            const int64_t per_cu = ceil_div(tiles * sp, 256);
            const int64_t kt_per = ceil_div(kt, sp);
            const int conc = (int)(per_cu < cap ? per_cu : cap);
            const double eff = tile == 128 ? eff128[conc] : eff64[conc];
            double cost = (double)per_cu * unit * (double)(kt_per + 3) / eff;
            // (deferred: no reduce launch, but the slabs are written by this kernel and read by the consumer; fitted to
            // same-box A/B runs of the forward projections of BASELINE configs 2 and 4; probe removed,
            // `git show 4165530:scripts/ab_yslabs.sh`)
            if (sp > 1) cost += deferred ? 4.5 + 9.0 * sp * mn : 12.0 + 6.5 * sp * mn;
            if (cost < best_cost) { best_cost = cost; best = GemmCfg{tile, sp}; }
        }
    }
    return best;
}

// The slice count after the scratch rule and the rounding of a slice to whole k tiles of 64 (a multiple of either BK).
// A slab buffer too small for the model's slice count: the largest power of two that fits, not one slice (the class
// layer's 41 x 4096 x 2046 weight gradient fell from 8 slices to 1 for most batch sizes of the h = 2048 step -- 39 us
// instead of 13 -- because the count is not monotone in k and the step had sized its buffer from a few sampled batch sizes)
struct F32Slices { int asked, splits; int64_t k_per; };
F32Slices f32_slices(int model_splits, int64_t m, int64_t n, int64_t k, int64_t scratch) {
    F32Slices s{model_splits, 1, 64};
    while (s.asked > 1 && scratch >= 0 && scratch < (int64_t)s.asked * m * n * 4) s.asked >>= 1;
    s.k_per = ceil_div(ceil_div(k, 64), s.asked) * 64;
    s.splits = (int)ceil_div(k, s.k_per > 0 ? s.k_per : 1);
    if (s.splits < 1) s.splits = 1;
    if (k == 0) { s.k_per = 64; s.splits = 1; }
    return s;
}

void plan_f32(const GemmQuery &q, GemmPlan &p) {
    const GemmCfg cfg = choose_cfg(q.m, q.n, q.k, q.deferred);
    const F32Slices s = f32_slices(cfg.splits, q.m, q.n, q.k, q.scratch);
    p.path = GEMM_PATH_F32;
    p.tile_m = p.tile_n = cfg.tile;
    p.splits = s.splits; p.k_per_split = s.k_per;
    p.whole_tiles = (int32_t)(ceil_div(q.m, cfg.tile) * ceil_div(q.n, cfg.tile));
    p.scratch_bytes = s.asked > 1 ? (int64_t)s.asked * q.m * q.n * 4 : 0;
    p.workspace_bytes = p.scratch_bytes;
    p.launches = 1 + (s.splits > 1 && !q.deferred);
}

// ---- f16x3 -----------------------------------------------------------------------------------------------
// Shapes the split path takes: enough 128x128 tiles to occupy the chip and enough flops to
// pay for the pre-pass.  Break-even measured at ~20 GFLOP when every call splits its own
// operands (probe removed; `git show 4165530:scripts/h3_bench.py`) and at ~4 GFLOP inside the
// step, which shares one split of an operand between the GEMMs that use it (bench.py
// --n-hidden 1024: 0.606 -> 0.551 ms/step).
// Everything else stays on the fp32 kernel.
bool h3_shape_ok(int64_t m, int64_t n, int64_t k, double default_min_gflop) {
    const double t_gflop = tune(GIST_TUNE_H3_MIN_GFLOP), t_tiles = tune(GIST_TUNE_H3_MIN_TILES);
    const double min_gflop = t_gflop > 0.0 ? t_gflop : default_min_gflop;
    const int min_tiles = t_tiles > 0.0 ? (int)t_tiles : 64;
    // (an explicit tile threshold -- tests -- also lifts the minimum extents: the kernel itself
    // handles any m, n, k >= 1)
    if (t_tiles <= 0.0 && (m < 64 || n < 64 || k < 64)) return false;
    if (m < 1 || n < 1 || k < 1) return false;
    if (ceil_div(m, H3_T) * ceil_div(n, H3_T) < min_tiles) return false;
    if (2.0 * (double)m * (double)n * (double)k < min_gflop * 1e9) return false;
    if (h3_kpad(k) >= (1LL << 22)) return false;
    return true;
}

// per-call workspace: [inv_a: m floats][inv_b: n floats][max bits: m + n] padded to 256 B, then the splits
void plan_h3(const GemmQuery &q, GemmPlan &p) {
    const bool kept = q.call == GEMM_CALL_KEPT;
    p.path = GEMM_PATH_H3;
    p.kept_ok = kept && h3_shape_ok(q.m, q.n, q.k, 4.0);
    // 64-row A tiles when 128-row tiles would leave CUs without a second workgroup
    const int t_tm = (int)tune(GIST_TUNE_H3_TM);      // 0 = auto, 64 / 128 = forced
    const bool tm64 = t_tm ? t_tm == 64 : ceil_div(q.m, 128) * ceil_div(q.n, H3_T) < 512;
    p.tile_m = tm64 ? 64 : 128; p.tile_n = H3_T;
    p.splits = 1; p.k_per_split = q.k;
    p.whole_tiles = (int32_t)(ceil_div(q.m, p.tile_m) * ceil_div(q.n, H3_T));
    p.launches = 1;
    if (kept) return;
    p.operand_offset = ceil_div((q.m + q.n) * 8, 256) * 256;
    p.operand_bytes = (q.m + q.n) * h3_kpad(q.k) * 4;
    p.workspace_bytes = p.operand_offset + p.operand_bytes;
    // pre-passes: a k-contiguous source [rows][k] one fused kernel; a [k][rows] source column maxima, then the transposing split
    p.launches += (q.a_kc ? 1 : 2) + (q.b_kc ? 1 : 2);
}

// ---- bf16x3, operands split by a pre-pass ------------------------------------------------------------
// Split-K: an output with fewer than ~3/4 of 256 tiles leaves CUs idle (one 512-thread workgroup per
// CU), so its k range is cut into `splits` slices, one workgroup each (blockIdx.y), which write fp32
// slabs that one pass sums (+ bias).  A slice keeps >= 8 k tiles; slices are an even number of tiles.
int b3_splits(int64_t m, int64_t n, int64_t k) {
    const int64_t tiles = ceil_div(m, B3_TM) * ceil_div(n, B3_TN);
    const int64_t n_kt = b3_kpad(k) / B3_BK;
    const int forced = (int)tune(GIST_TUNE_GEMM_SPLITS);
    int64_t s = forced > 0 ? forced : (tiles >= 192 ? 1 : 256 / tiles);
    if (forced <= 0 && tiles > 128 && tiles < 192) {
        // between half a chip and 3/4 of one (dW_0 of the H = 4096 step: 160 tiles) one slice runs a single
        // under-full round; the slice count that minimises rounds x k tiles per slice wins even with the
        // slab sum (4096 x 1204 x 2046: 3 slices = 2 rounds of 22 k tiles against 1 of 64; 165 -> 154 us
        // per call with the sum in the call; probe removed, `git show 4165530:scripts/b3_split_probe.py`)
        int64_t best = n_kt + 4;      // one slice: no slabs (the +4: a slab sum costs about 4 k tiles)
        for (int64_t c = 2; c <= 4; ++c) {
            const int64_t per = ceil_div(ceil_div(n_kt, c), 2) * 2;
            const int64_t cost = ceil_div(tiles * c, 256) * per + 8;
            if (per >= 8 && cost < best) { best = cost; s = c; }
        }
    }
    if (forced <= 0 && s > n_kt / 8) s = n_kt / 8;
    if (s > n_kt / 2) s = n_kt / 2;
    if (s < 1) s = 1;
    const int64_t per = ceil_div(ceil_div(n_kt, s), 2) * 2;
    return (int)ceil_div(n_kt, per);
}
// Tail units: with one k slice and T tiles on P = 256 one-workgroup CUs the last round holds r = T mod P
// tiles and leaves P - r CUs idle for a whole tile's k loop (a batch of 2049-2304 rows has a ninth row
// tile: 288 tiles = one round + 32, twice the time of 256).  The r tiles of that round are cut into
// floor(P / r) k slices of >= 8 k tiles, one workgroup each, so the round lasts 1 / slices of a tile;
// the slices of a tile leave fp32 partials that gemm_b3_tail_sum_kernel, the next launch, adds in slice
// order (a hand-over inside the kernel -- the last slice to arrive sums -- was measured first: its
// device-scope fences cost 45-70 us per launch).  Nothing here depends on anything but the shape.
// (the convert-on-load kernel's: S workgroup slots -- 64 x 64 tiles: two workgroups per CU = 512, the larger tiles one = 256 --
// with 0 < T mod S <= S / 2: a batch of 2049-2112 rows makes 528 tiles of 64 x 64 out of 512, 272 of 128 x 128 out of 256;
// slices of >= 4 k tiles, of any number of tiles)
struct Tail { int64_t whole_tiles; int splits; int64_t k_per, bytes; };      // splits 1: none
Tail tail_units(int64_t tiles, int64_t slots, int64_t n_kt, int64_t min_kt, int64_t kt_multiple, int64_t tile_bytes) {
    Tail t{tiles, 1, 0, 0};
    if (tune(GIST_TUNE_B3_TAIL) == 1.0 || tiles <= slots) return t;
    const int64_t r = tiles % slots;
    if (r == 0 || r > slots / 2) return t;
    int64_t s = std::min(slots / r, n_kt / min_kt);
    if (s < 2) return t;
    const int64_t per = ceil_div(ceil_div(n_kt, s), kt_multiple) * kt_multiple;
    s = ceil_div(n_kt, per);
    if (s < 2) return t;
    return Tail{tiles - r, (int)s, per * B3_BK, r * s * tile_bytes};
}
Tail b3_tail(int64_t m, int64_t n, int64_t k) {
    return tail_units(ceil_div(m, B3_TM) * ceil_div(n, B3_TN), B3_CUS, b3_kpad(k) / B3_BK, 8, 2, (int64_t)B3_TM * B3_TN * 4);
}

// Shapes the bf16x3 path takes: enough workgroups (256 x 128 tiles x k slices) to occupy the chip, and
// enough flops to pay for the pre-pass (~ the f16x3 path's thresholds).  Everything else stays on the
// fp32 kernel.  (Inside the step, operands split once per tensor: measured break-even between 8.6 GFLOP -- the
// h = 1024 projections, 0.595 vs 0.587 ms/step on the fp32 kernel -- and 10.1 GFLOP -- the layer-0 projections at
// h = 2048, 1.071 vs 1.095: 9 GFLOP there, 16 for a call that splits its own operands.)
bool b3_shape_ok(int64_t m, int64_t n, int64_t k, int splits, double default_min_gflop) {
    const double t_gflop = tune(GIST_TUNE_H3_MIN_GFLOP), t_tiles = tune(GIST_TUNE_H3_MIN_TILES);
    const double min_gflop = t_gflop > 0.0 ? t_gflop : default_min_gflop;
    const int min_wgs = t_tiles > 0.0 ? (int)t_tiles : 128;
    // (an explicit tile threshold -- tests -- also lifts the minimum extents: the kernel itself
    // handles any m, n, k >= 1)
    if (t_tiles <= 0.0 && (m < 64 || n < 64 || k < 64)) return false;
    if (m < 1 || n < 1 || k < 1) return false;
    const int64_t tiles = ceil_div(m, B3_TM) * ceil_div(n, B3_TN);
    if (tiles * splits < min_wgs) return false;
    if (t_tiles <= 0.0 && (double)m * (double)n < 0.6 * (double)(tiles * B3_TM * B3_TN)) return false;   // mostly padding
    if (2.0 * (double)m * (double)n * (double)k < min_gflop * 1e9) return false;
    if (b3_kpad(k) * 6 >= (1LL << 23)) return false;          // 32-bit DMA byte offsets: 256 rows * pitch
    return true;
}
// the store epilogue's 32-bit byte offsets: 256 rows x ldc
bool b3_ldc_ok(int64_t ldc) { return ldc * B3_TM * 4 < (1LL << 31); }

// Returns whether the shape passes the thresholds of its kind of call.  Scratch holds the fp32 slabs of a split-K call or the
// partials of its tail units, never both; slabs that do not fit: one slice; tail partials that do not fit: whole tiles.
bool plan_b3(const GemmQuery &q, GemmPlan &p) {
    const bool kept = q.call == GEMM_CALL_KEPT;
    const int64_t m = q.m, n = q.n, k = q.k, n_kt = b3_kpad(k) / B3_BK;
    const int model_splits = b3_splits(m, n, k);
    const bool takes = b3_shape_ok(m, n, k, model_splits, kept ? 9.0 : 16.0) && b3_ldc_ok(q.ldc);
    p.path = GEMM_PATH_B3;
    p.kept_ok = kept && takes;
    if (!kept && !takes) return false;
    GemmQuery room = q;      // (a call that splits its own operands is taken only with all it asks: nothing degrades)
    if (!kept) room.scratch = kScratchUnbounded, room.scratch_aligned = true;
    const int asked = model_splits > 1 && !fits(room, (int64_t)model_splits * m * n * 4) ? 1 : model_splits;
    const int64_t kt_per = ceil_div(ceil_div(n_kt, asked), 2) * 2;
    p.splits = (int32_t)ceil_div(n_kt, kt_per); p.k_per_split = kt_per * B3_BK;
    p.tile_m = B3_TM; p.tile_n = B3_TN;
    p.whole_tiles = (int32_t)(ceil_div(m, B3_TM) * ceil_div(n, B3_TN)); p.tail_splits = 1;
    const Tail t = p.splits == 1 ? b3_tail(m, n, k) : Tail{p.whole_tiles, 1, 0, 0};
    if (t.splits > 1 && room.scratch_aligned && fits(room, t.bytes)) {
        p.whole_tiles = (int32_t)t.whole_tiles; p.tail_splits = t.splits; p.tail_k = t.k_per;
    }
    // The 256 x 256 tile (gemm_b3_wide_kernel) takes an output that has at least one full round of such tiles and that
    // the 256 x 128 kernel would run as one k slice with no tail units (tuning hook GIST_TUNE_B3_WIDE = 1: never).  On
    // the H = 4096 step: dZ1 (256 wide tiles, one round instead of two) and dW1 (512: two instead of four); the forward
    // Z1.W1 (128) and layer 0's projections stay on the 256 x 128 kernel.
    if (tune(GIST_TUNE_B3_WIDE) != 1.0 && ceil_div(m, B3_TM) * ceil_div(n, B3W_TN) >= B3_CUS && model_splits == 1 &&
        t.splits < 2) {
        p.tile_n = B3W_TN;
        p.whole_tiles = (int32_t)(ceil_div(m, B3_TM) * ceil_div(n, B3W_TN));
    }
    p.scratch_bytes = asked > 1 ? (int64_t)asked * m * n * 4 : (p.tail_splits > 1 ? t.bytes : 0);
    p.launches = 1 + (p.tail_splits > 1) + (p.splits > 1 && !(kept && q.deferred));
    if (!kept) {
        p.operand_bytes = ceil_div((m + n) * b3_kpad(k) * 6 + 512, 256) * 256;
        p.scratch_offset = p.operand_bytes;
        p.launches += 2;      // one split pre-pass per operand
    }
    p.workspace_bytes = p.operand_bytes + p.scratch_bytes;
    return takes;
}

// ---- bf16x3, operands converted on load --------------------------------------------------------------
// Which calls take this kernel by default.  MEASURED (profiles/r03_b3c_bench.txt; us,
// standalone calls, fp32 kernel -> this kernel with 64 x 64 tiles and one k slice): NT 2046 x 1024 x 2048
// 76 -> 59, NT 2046 x 1024 x 1204 50 -> 43, NN 2046 x 2048 x 1024 73 -> 66, NT 2046 x 512 x 1204 24.9 -> 22.3;
// TN (both operands k-major: 16 scalar row loads per thread and step) 1024 x 2048 x 2046 68.5 -> 64, but
// 1024 x 1204 x 2046 54 -> 60 and 512 x 1024 x 2046 25 -> 43.  So by default the NT and NN layouts from
// 2 GFLOP with at least 256 tiles of 64 x 64 come here and TN stays on the fp32 kernel; the tuning hook
// GIST_TUNE_B3C = 2 sends every shape with m, n, k >= 64 (tests, sweeps), 1 none.  A k step still costs
// several hundred cycles on top of its MFMAs; the matrix pipe is far from saturated.
bool b3c_takes(const GemmQuery &q) {
    const int hook = (int)tune(GIST_TUNE_B3C);
    const int64_t m = q.m, n = q.n, k = q.k;
    if (q.mode != 2 || hook == 1 || m < 64 || n < 64 || k < 64) return false;
    if (hook != 2 && !(ceil_div(m, 64) * ceil_div(n, 64) >= 256 && 2.0 * (double)m * (double)n * (double)k >= 2e9)) return false;
    if (!q.aligned) return false;
    if (!q.a_kc && q.b_kc) return false;            // (no caller uses this layout)
    return hook == 2 || q.a_kc;                     // by default: NT and NN only (see above)
}

// Tile and k slices (fp32 slabs, reduced by the call or left to the consumer).  Fitted to profiles/r03_b3c_bench.txt.
void b3c_choice(int64_t m, int64_t n, int64_t k, int *tm, int *tn, int *splits) {
    const int t_tile = (int)tune(GIST_TUNE_GEMM_TILE), t_split = (int)tune(GIST_TUNE_GEMM_SPLITS);
    auto tiles = [&](int a, int b) { return ceil_div(m, a) * ceil_div(n, b); };
    // 64 x 64 unless the output has 256 tiles of 128 x 128 (measured: NN 2046 x 2048 x 1024 62 -> 54 us; with fewer
    // tiles the 128 x 128 grid leaves CUs idle or needs k slices and loses: NT 2046 x 1024 x 2048 59 vs 82 / 60 with
    // 1 / 2 slices; 128 x 64 is slower than 64 x 64 on every per-rank shape).  A k step of the 128 x 128 tile takes
    // ~2700 cycles for 1536 of MFMA, one of the 64 x 64 tile ~1200 for 384: the producers' step (176 / 88 vector
    // instructions, 12 / 6 ds_write_b128 at ~13 issue cycles, 8 / 4 loads) sets the pace in both, and neither deeper
    // load prefetch (PD 4-6), nor LDS writes issued before the conversion, nor cheaper instructions (v_perm for
    // v_cvt_pk, v_sub for v_pk_add), nor half as many MFMA issues (32 x 32 x 16) moved it
    // (probe removed; `git show 4165530:scripts/b3c_probe.py`).
    *tm = 64; *tn = 64;
    if (tiles(128, 128) >= 256) { *tm = 128; *tn = 128; }
    if (t_tile == 64) { *tm = 64; *tn = 64; }
    if (t_tile == 128 || t_tile == 12864) { *tm = 128; *tn = 64; }
    if (t_tile == 128128) { *tm = 128; *tn = 128; }
    const int64_t wgs = tiles(*tm, *tn);
    const int64_t kt = ceil_div(k, C3_BK);
    int64_t sp = 1;
    if (wgs < 128) sp = 256 / wgs;                            // (only reachable through the tuning hook)
    if (sp > kt / 8) sp = kt / 8;                             // a slice keeps >= 8 k tiles
    if (t_split > 0) sp = t_split;
    if ((int)tune(GIST_TUNE_B3C_SPLITS) > 0) sp = (int)tune(GIST_TUNE_B3C_SPLITS);
    if (sp > kt) sp = kt;
    *splits = (int)(sp < 1 ? 1 : sp);
}

Tail b3c_tail(int64_t m, int64_t n, int64_t k, int tm, int tn) {
    static_assert(C3_BK == B3_BK, "tail_units counts k in tiles of B3_BK");
    return tail_units(ceil_div(m, tm) * ceil_div(n, tn), (tm == 64 && tn == 64) ? 512 : 256, ceil_div(k, C3_BK), 4, 1,
                      (int64_t)tm * tn * 4);
}

// slabs that do not fit: one slice; tail partials that do not fit: whole tiles
void plan_b3c(const GemmQuery &q, GemmPlan &p) {
    const int64_t m = q.m, n = q.n, k = q.k;
    int tm, tn, asked;
    b3c_choice(m, n, k, &tm, &tn, &asked);
    if (asked > 1 && !fits(q, (int64_t)asked * m * n * 4)) asked = 1;
    p.path = GEMM_PATH_B3C;
    p.tile_m = tm; p.tile_n = tn;
    p.k_per_split = ceil_div(ceil_div(k, C3_BK), asked) * C3_BK;
    p.splits = (int32_t)ceil_div(k, p.k_per_split);
    p.whole_tiles = (int32_t)(ceil_div(m, tm) * ceil_div(n, tn)); p.tail_splits = 1;
    const Tail t = p.splits == 1 ? b3c_tail(m, n, k, tm, tn) : Tail{p.whole_tiles, 1, 0, 0};
    if (t.splits > 1 && q.scratch_aligned && fits(q, t.bytes)) {
        p.whole_tiles = (int32_t)t.whole_tiles; p.tail_splits = t.splits; p.tail_k = t.k_per;
    }
    p.scratch_bytes = asked > 1 ? (int64_t)asked * m * n * 4 : (p.tail_splits > 1 ? t.bytes : 0);
    p.workspace_bytes = p.scratch_bytes;
    p.launches = 1 + (p.tail_splits > 1) + (p.splits > 1 && !q.deferred);
}

// ---- bf16x1: operands rounded to bf16 once by a cast pre-pass, one MFMA term (gemm_bf16.hip) -------------
// Mode 3 only, and only a gist_gemm_* call that reduces its own k slices (GEMM_CALL_SPLITS, not deferred): the step's
// slab and kept calls and the fused-epilogue entry points get the record mode 0 gives them.  By default a shape comes
// here from 2.5 GFLOP with m, n, k >= 64, an output that is not mostly tile padding and, k slices included, at least 128
// workgroups.  Measured per call with the pre-pass in the call, against the fp32 kernel (profiles/gemm_bf16x1.md): 2046 x
// 512 x 1204 (2.52 GFLOP) 25.2 -> 22.4 us, its TN and NN forms too, and everything larger wins, up to 4.2x; 1024 x 1024 x 1024
// (2.15 GFLOP) loses in every layout (21.5 -> 22.6 .. 24.7 us), as do 2046 x 41 x 8192 and everything below 1.1 GFLOP.  Tuning
// hook GIST_TUNE_BF16X1: 1 = never, 2 = every shape with m, n, k >= 1.
// k slices: an output with fewer than 384 tiles of 128 x 128 (two workgroups per CU: 512 slots) is cut along k into
// slices of >= 8 k tiles (>= 2 under the hook), whose fp32 slabs splitk_reduce sums in slice order (+ bias).
int x1_splits(int64_t m, int64_t n, int64_t k, bool any_shape) {
    const int64_t tiles = ceil_div(m, X1_T) * ceil_div(n, X1_T), n_kt = x1_kpad(k) / X1_BK;
    const int forced = (int)tune(GIST_TUNE_GEMM_SPLITS);
    int64_t s = forced > 0 ? forced : (tiles >= 384 ? 1 : 512 / tiles);
    const int64_t min_kt = any_shape ? 2 : 8;
    if (forced <= 0 && s > n_kt / min_kt) s = n_kt / min_kt;
    if (s > n_kt) s = n_kt;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    return (int)ceil_div(n_kt, ceil_div(n_kt, s));
}

bool plan_x1(const GemmQuery &q, GemmPlan &p) {
    const int hook = (int)tune(GIST_TUNE_BF16X1);
    const int64_t m = q.m, n = q.n, k = q.k;
    if (q.mode != 3 || hook == 1 || q.call != GEMM_CALL_SPLITS || q.deferred) return false;
    // 32-bit byte offsets of the DMA staging (128 rows x pitch) and of the slab stores (128 rows x n); the grid
    if (m < 1 || n < 1 || k < 1 || x1_kpad(k) >= (1LL << 22) || n >= (1LL << 22)) return false;
    if (ceil_div(m, X1_T) * ceil_div(n, X1_T) >= (1LL << 30)) return false;
    const int splits = x1_splits(m, n, k, hook == 2);
    const int64_t tiles = ceil_div(m, X1_T) * ceil_div(n, X1_T);
    if (hook != 2) {
        if (m < 64 || n < 64 || k < 64) return false;
        if (tiles * splits < 128) return false;
        if ((double)m * (double)n < 0.6 * (double)(tiles * X1_T * X1_T)) return false;      // mostly padding
        if (2.0 * (double)m * (double)n * (double)k < 2.5e9) return false;
    }
    const int64_t n_kt = x1_kpad(k) / X1_BK, kt_per = ceil_div(n_kt, splits);
    p.path = GEMM_PATH_BF16X1;
    p.tile_m = p.tile_n = X1_T;
    p.splits = splits; p.k_per_split = kt_per * X1_BK;
    p.whole_tiles = (int32_t)tiles; p.tail_splits = 1;
    p.operand_offset = 0;
    p.operand_bytes = ceil_div((m + n) * x1_kpad(k) * 2, 256) * 256;
    p.scratch_offset = p.operand_bytes;
    p.scratch_bytes = splits > 1 ? (int64_t)splits * m * n * 4 : 0;
    p.workspace_bytes = p.operand_bytes + p.scratch_bytes;
    p.launches = 2 + (splits > 1);      // the cast of both operands, the main kernel, the slab sum
    return q.scratch_aligned && fits(q, p.workspace_bytes);
}

}  // namespace

GemmPlan plan_gemm(const GemmQuery &q) {
    const GemmPlan none{0, 0, 0, 0, 1, 0, 1};
    GemmPlan p = none;
    if (q.m <= 0 || q.n <= 0 || q.k < 0) return p;      // nothing to launch
    if (q.k == 0) { plan_f32(q, p); return p; }         // bias or zeros: no path that splits operands or counts k tiles
    if (q.call == GEMM_CALL_KEPT && q.mode == 1) { plan_h3(q, p); return p; }
    if (q.call == GEMM_CALL_KEPT && q.mode == 2) { plan_b3(q, p); return p; }
    // a call that splits its own operands: large, chip-filling shapes, and only with the whole workspace it asks for
    if (q.call != GEMM_CALL_SLABS && q.mode == 1 && q.aligned && h3_shape_ok(q.m, q.n, q.k, 16.0)) {
        plan_h3(q, p);
        if (q.scratch_aligned && fits(q, p.workspace_bytes)) return p;
    }
    if (q.call != GEMM_CALL_SLABS && q.mode == 2 && plan_b3(q, p) && q.scratch_aligned && fits(q, p.workspace_bytes)) return p;
    p = none;
    if (q.mode == 3 && plan_x1(q, p)) return p;
    p = none;
    if (b3c_takes(q)) plan_b3c(q, p);
    else plan_f32(q, p);
    return p;
}

// (c1.splits == 1: dz is written in place; 2 workgroups per CU resident: beyond ~2.5 rounds each product fills the
// chip alone; the per-rank widths <= 512 and config 2)
GemmDualPlan plan_gemm_dual(int64_t m, int64_t n1, int64_t k1, int mode, int64_t scratch) {
    GemmDualPlan d{false, 1, 64};
    if (m <= 0 || n1 <= 0 || k1 <= 0 || (int)tune(GIST_TUNE_GEMM_DUAL) == 1) return d;
    if (tune(GIST_TUNE_GEMM_TILE) != 0.0 || tune(GIST_TUNE_GEMM_SPLITS) != 0.0) return d;
    if (mode == 3) mode = 0;      // (bf16x1: the fused pair stays on the fp32 kernel, with the shapes mode 0 gives it)
    // neither product may be one that a gist_gemm_* call would run on split operands
    const GemmPlan nn = plan_gemm(gemm_query(1, m, n1, k1, mode, GEMM_CALL_SPLITS, false));
    const GemmPlan tn = plan_gemm(gemm_query(2, k1, n1, m, mode, GEMM_CALL_SPLITS, true));
    if (splits_operands(nn) || splits_operands(tn)) return d;
    const GemmCfg c1 = choose_cfg(m, n1, k1), c2 = choose_cfg(k1, n1, m, true);
    if (c1.tile != 64 || c2.tile != 64 || c1.splits != 1) return d;
    if (ceil_div(m, 64) * ceil_div(n1, 64) + ceil_div(k1, 64) * ceil_div(n1, 64) * c2.splits > 1280) return d;
    const F32Slices s = f32_slices(c2.splits, k1, n1, m, scratch);
    return GemmDualPlan{true, s.splits, s.k_per};
}

int64_t gemm_slab_bytes(int layout, int64_t m, int64_t n, int64_t k, int mode) {
    if (m <= 0 || n <= 0 || k <= 0) return 0;
    const GemmPlan a = plan_gemm(gemm_query(layout, m, n, k, mode, GEMM_CALL_SLABS, true, true));
    const GemmPlan u = plan_gemm(gemm_query(layout, m, n, k, mode, GEMM_CALL_SLABS, true, false));
    return std::max(a.scratch_bytes, u.scratch_bytes);
}

}  // namespace gist

extern "C" int gist_gemm_set_mode(int mode) {
    GIST_REQUIRE(mode >= 0 && mode <= 3,
                 "gist_gemm_set_mode: mode must be 0 (fp32 MFMA), 1 (f16x3 split), 2 (bf16x3 split) or 3 (bf16x1)");
    gist::g_gemm_mode.store(mode, std::memory_order_relaxed);
    return GIST_OK;
}

extern "C" int gist_gemm_get_mode(void) { return gist::gemm_mode(); }

extern "C" int gist_gemm_plan_query(int layout, int64_t m, int64_t n, int64_t k, int aligned, int call, int deferred,
                                    int64_t scratch_bytes, gist_gemm_plan *out) {
    GIST_REQUIRE(out != nullptr, "gist_gemm_plan_query: null out");
    GIST_REQUIRE(layout >= 0 && layout <= 2, "gist_gemm_plan_query: layout must be 0 (NT), 1 (NN) or 2 (TN)");
    GIST_REQUIRE(m >= 0 && n >= 0 && k >= 0 && m < (1LL << 31) && n < (1LL << 31) && k < (1LL << 31),
                 "gist_gemm_plan_query: a size is negative or >= 2^31 (no gist_gemm_* call takes it)");
    GIST_REQUIRE(call >= GIST_GEMM_CALL_SPLITS && call <= GIST_GEMM_CALL_SLABS, "gist_gemm_plan_query: unknown kind of call");
    *out = gist::plan_gemm(gist::gemm_query(layout, m, n, k, gist::gemm_mode(), (gist::GemmCall)call, deferred != 0,
                                            aligned != 0, scratch_bytes < 0 ? gist::kScratchUnbounded : scratch_bytes));
    return GIST_OK;
}

/* 1 if a gist_gemm_* call of this shape splits its own operands in the current mode (f16x3 / bf16x3 pre-split
 * kernels: it needs the large workspace of gist_gemm_workspace_bytes and reduces its k slices itself). */
extern "C" int gist_gemm_splits_operands(int64_t m, int64_t n, int64_t k) {
    if (m <= 0 || n <= 0 || k <= 0) return 0;
    return gist::splits_operands(gist::plan_gemm(gist::gemm_query(0, m, n, k, gist::gemm_mode(), gist::GEMM_CALL_SPLITS, false)));
}

/* what a call of this shape may ask for, whatever its layout: the split operands (+ slabs) where it splits them itself;
 * else the slabs or tail partials of aligned operands (convert-on-load) and of unaligned ones (they fall back to the fp32
 * kernel), reducing itself or leaving the slabs (gist_gemm_slabs_f32) */
extern "C" int64_t gist_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k) {
    if (m <= 0 || n <= 0 || k <= 0) return 0;
    using namespace gist;
    const int mode = gemm_mode();
    const GemmPlan a = plan_gemm(gemm_query(0, m, n, k, mode, GEMM_CALL_SPLITS, false));
    if (splits_operands(a)) return a.workspace_bytes;
    const GemmPlan u0 = plan_gemm(gemm_query(0, m, n, k, mode, GEMM_CALL_SPLITS, false, false));
    const GemmPlan u1 = plan_gemm(gemm_query(0, m, n, k, mode, GEMM_CALL_SPLITS, true, false));
    return std::max(a.workspace_bytes, std::max(u0.workspace_bytes, u1.workspace_bytes));
}
