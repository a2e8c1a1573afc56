// Full-graph evaluation of a GAT layer (utils.evaluate over GAT.forward, cluster_gcn/utils.py:70-80 over modules.py:93-98)
// on a graph whose node ids are ordered by part: blocks of at most 128 consecutive rows whose mutual edges are dense.
//
// Two passes make the aggregation linear.  gist_gat_row_stats_f32 finds per (row, head) the softmax max M and
// denominator L from the scores alone (no Z is read).  With both known, alpha_hij = exp(e_hij - M[i,h]) / L[i,h] is a
// plain weight, so a row's sum splits into the edges inside its block and the rest, and the two parts just add:
//
//   dense      per block ONE count image c[j][i] (edges j -> i inside the block, integer LDS atomics, built once for all
//              heads), then per head W_h[i][j] = c_ij exp(e_hij - M) / L -- one exp per (row, source) CELL, not per edge --
//              times Z_h of the block's rows on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fma chain).  The weight
//              is formed in the register that is the MFMA's A operand (lane l: row l & 31, source k + (l >> 5)); the B
//              operand is read from Z as it lies in memory.  One workgroup per block, one wave per 32 rows.
//   remainder  every edge whose source lies outside the row's block is walked as gat_aggregate_kernel walks (one wave
//              per row, groups of lanes over the edges, an xor butterfly at the end) and added; then the epilogue
//              (head mean or concatenation, ELU).
//
// They are two launches: the dense kernel holds 64 KiB of LDS per workgroup (two workgroups, eight waves per CU), which
// is no place for a walker that hides gather latency behind many waves; the walker has no LDS and runs at full
// occupancy.  The pre-activation sums cross through `out` itself.  No float atomics: every sum has a fixed order.
#include <math.h>

#include "common.h"

namespace gist {

constexpr float kEvalSlope = 0.01f;       // F.leaky_relu's default negative slope (modules.py:44), as in gat.hip
constexpr int kEvalBlock = 128;           // rows of a block at most
constexpr int kEvalStatRows = 4;          // rows per workgroup of the statistics kernel: one wave each

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float eval_score(float s_src, float s_dst) {
    const float s = s_src + s_dst;
    return s > 0.f ? s : kEvalSlope * s;      // (the same two operations as gat_aggregate_kernel: the same bits)
}

// M[i,h] = max over the in-edges of e, L[i,h] = sum of exp(e - M); one wave per row.  A lane owns head lane % HP
// (HP = the power of two at or above min(H, 64)) and every (64 / HP)-th edge; heads beyond 64 in further rounds.
__global__ __launch_bounds__(256) void gat_row_stats_kernel(const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ col,
                                                            const float *__restrict__ s_src,
                                                            const float *__restrict__ s_dst, int64_t n, int H, int HP,
                                                            float *__restrict__ M, float *__restrict__ L) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kEvalStatRows + (threadIdx.x >> 6);
    if (row >= n) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const int slot = lane / HP, stride = kWave / HP;
    for (int h0 = 0; h0 < H; h0 += HP) {
        const int h = h0 + lane % HP;
        const bool live = h < H;
        const float sd = live ? s_dst[row * H + h] : 0.f;
        float m = -INFINITY;
        if (live)
            for (int e = e0 + slot; e < e1; e += stride) m = fmaxf(m, eval_score(s_src[(int64_t)col[e] * H + h], sd));
        for (int off = HP; off < kWave; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
        // a lane's share of the sum is compensated (Kahan): a cell repeated tens of thousands of times is a chain of equal
        // terms, whose plain fp32 sum drifts by far more than its length times a random rounding would
        float l = 0.f, comp = 0.f;
        if (live)
            for (int e = e0 + slot; e < e1; e += stride) {
                const float y = expf(eval_score(s_src[(int64_t)col[e] * H + h], sd) - m) - comp;
                const float t = l + y;
                comp = (t - l) - y;
                l = t;
            }
        for (int off = HP; off < kWave; off <<= 1) l += __shfl_xor(l, off, kWave);
        if (live && slot == 0) {
            M[row * H + h] = e1 > e0 ? m : 0.f;
            L[row * H + h] = e1 > e0 ? l : 0.f;
        }
    }
}

struct EvalBlock {
    int b0, bs;       // first row and rows (0 for boundaries that do not describe a block)
};

__device__ __forceinline__ EvalBlock eval_block(const int32_t *__restrict__ block_ptr, int64_t n) {
    int b0 = block_ptr[blockIdx.x], b1 = block_ptr[blockIdx.x + 1];
    b0 = max(b0, 0);
    b1 = (int)min((int64_t)b1, n);
    return {b0, max(min(b1 - b0, kEvalBlock), 0)};
}

// Dense part: out[i, :] (pre-activation; CAT: head h's columns, else the sum over heads) = sum_j W_h[i][j] Z_h[j] over the
// sources j of i's block.  NT = 32-column tiles a wave accumulates at once.
template <int NT>
__global__ __launch_bounds__(256) void gat_blocks_dense_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ block_ptr,
    const float *__restrict__ Z, int64_t ldz, const float *__restrict__ s_src, const float *__restrict__ s_dst,
    const float *__restrict__ M, const float *__restrict__ L, int64_t n, int H, int F, int cat,
    float *__restrict__ out, int64_t ldo) {
    __shared__ uint32_t cnt[kEvalBlock * kEvalBlock];      // [source j][row i]: a wave's A reads run along i
    const EvalBlock B = eval_block(block_ptr, n);
    const int b0 = B.b0, bs = B.bs;
    if (bs <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < bs * kEvalBlock; t += 256) cnt[t] = 0u;
    __syncthreads();
    for (int il = wave; il < bs; il += 4) {
        const int e0 = rowptr[b0 + il], e1 = rowptr[b0 + il + 1];
        for (int e = e0 + lane; e < e1; e += kWave) {
            const int j = col[e] - b0;
            if (j >= 0 && j < bs) atomicAdd(&cnt[j * kEvalBlock + il], 1u);
        }
    }
    __syncthreads();
    if (wave * 32 >= bs) return;      // (no barrier below: a wave without rows is done)
    const int lc = lane & 31, kh = lane >> 5;
    const int il = wave * 32 + lc;
    const bool row_ok = il < bs;
    const int64_t row = b0 + (row_ok ? il : 0);
    for (int c0 = 0; c0 < F; c0 += 32 * NT) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int h = 0; h < H; ++h) {
            const float sd = s_dst[row * H + h], m = M[row * H + h], l = L[row * H + h];
            const float inv_l = (row_ok && l > 0.f) ? 1.0f / l : 0.f;
            const float *zh = Z + (int64_t)h * F + c0 + lc;
            for (int k = 0; k < bs; k += 2) {
                const int j = k + kh;
                const bool j_ok = j < bs;
                const uint32_t c = j_ok ? cnt[j * kEvalBlock + il] : 0u;
                float a = 0.f;
                if (c != 0u && row_ok)
                    a = (float)c * (expf(eval_score(s_src[(int64_t)(b0 + j) * H + h], sd) - m) * inv_l);
                const float *zj = zh + (int64_t)(b0 + (j_ok ? j : 0)) * ldz;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float b = (j_ok && c0 + 32 * t + lc < F) ? zj[32 * t] : 0.f;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
                }
            }
            if (cat || h == H - 1) {
                // accumulator element r of lane (lc, kh): row (r & 3) + 8 (r >> 2) + 4 kh of the wave's 32, column lc
                float *o = out + (cat ? (int64_t)h * F : 0) + c0 + lc;
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ir = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                        if (ir < bs && c0 + 32 * t + lc < F) o[(int64_t)(b0 + ir) * ldo + 32 * t] = acc[t][r];
                        if (cat) acc[t][r] = 0.f;
                    }
            }
        }
    }
}

// Remainder and epilogue: out = act(((dense part, read from out) + sum over the out-of-block edges) [/ H]).  One wave
// per row, four rows per workgroup, as gat_aggregate_kernel (a workgroup per block would leave the chip a few thousand
// waves for a latency-bound gather); the wave finds its row's block by bisection of block_ptr.  The wave's lanes form
// 64 / lpg edge groups of lpg lanes with VEC columns each.
template <int VEC>
__global__ __launch_bounds__(256) void gat_blocks_rest_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ block_ptr,
    int n_blocks, const float *__restrict__ Z, int64_t ldz, const float *__restrict__ s_src,
    const float *__restrict__ s_dst, const float *__restrict__ M, const float *__restrict__ L, int64_t n, int H, int F,
    int elu, int cat, int lpg, float *out, int64_t ldo) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    int lo = 0, hi = n_blocks;      // block_ptr[lo] <= row < block_ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (block_ptr[mid] <= row) lo = mid; else hi = mid;
    }
    const int b0 = block_ptr[lo], b1 = block_ptr[lo + 1];
    const int G = kWave / lpg, grp = lane / lpg, li = lane % lpg;
    const float scale = cat ? 1.0f : 1.0f / (float)H;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c0 = 0; c0 < F; c0 += lpg * VEC) {
        const int c = c0 + li * VEC;
        const bool active = c < F;
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = 0.f;
        for (int h = 0; h < H; ++h) {
            const float sd = s_dst[row * H + h], m = M[row * H + h], l = L[row * H + h];
            const float inv_l = l > 0.f ? 1.0f / l : 0.f;
            const float *zh = Z + (int64_t)h * F + c;
            // the walked sum is kept in double: an edge repeated tens of thousands of times is a chain of equal terms,
            // whose fp32 sum drifts by far more than its length times a random rounding would (the walker hides
            // gather latency, not arithmetic)
            double acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.0;
            for (int e = e0 + grp; e < e1; e += G) {
                const int j = col[e];
                if ((j >= b0 && j < b1) || !active) continue;      // (inside the block: the dense kernel's)
                const double p = (double)(expf(eval_score(s_src[(int64_t)j * H + h], sd) - m) * inv_l);
                float z[VEC];
                vload<VEC>(zh + (int64_t)j * ldz, z);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = fma(p, (double)z[k], acc[k]);
            }
            // (every lane of a group adds the same values in the same order: identical bits per group)
            for (int off = lpg; off < kWave; off <<= 1)
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += __shfl_xor(acc[k], off, kWave);
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] += (float)acc[k];
            if (cat && grp == 0 && active) {
                float *dst = out + row * ldo + (int64_t)h * F + c;
                float d[VEC];
                vload<VEC>(dst, d);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float v = d[k] + o[k];
                    d[k] = (elu && !(v > 0.f)) ? expm1f(v) : v;
                    o[k] = 0.f;
                }
                vstore<VEC>(dst, d);
            }
        }
        if (!cat && grp == 0 && active) {
            float *dst = out + row * ldo + c;
            float d[VEC];
            vload<VEC>(dst, d);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float v = (d[k] + o[k]) * scale;
                d[k] = (elu && !(v > 0.f)) ? expm1f(v) : v;
            }
            vstore<VEC>(dst, d);
        }
    }
}

static bool eval_sizes_ok(int64_t n, int64_t H, int64_t F) {
    return n >= 0 && n < (int64_t)1 << 31 && H >= 1 && F >= 1 && H * F < (int64_t)1 << 31;
}

}  // namespace gist

using namespace gist;

extern "C" int gist_gat_row_stats_f32(const int32_t *rowptr, const int32_t *col, const float *s_src,
                                      const float *s_dst, int64_t n_rows, int64_t heads, float *M, float *L,
                                      gist_stream_t stream) {
    GIST_REQUIRE(eval_sizes_ok(n_rows, heads, 1), "gist_gat_row_stats_f32: bad sizes");
    if (n_rows == 0) return GIST_OK;
    // (col is read only inside rowptr's ranges: it may be NULL for a graph without edges)
    GIST_REQUIRE(rowptr && s_src && s_dst && M && L, "gist_gat_row_stats_f32: null pointer");
    int hp = 1;
    while (hp < heads && hp < kWave) hp <<= 1;
    hipLaunchKernelGGL(gat_row_stats_kernel, dim3((unsigned)ceil_div(n_rows, kEvalStatRows)), dim3(256), 0,
                       as_stream(stream), rowptr, col, s_src, s_dst, n_rows, (int)heads, hp, M, L);
    return launch_status("gist_gat_row_stats_f32");
}

extern "C" int gist_gat_aggregate_blocks_f32(const int32_t *rowptr, const int32_t *col, const int32_t *block_ptr,
                                             int64_t n_blocks, const float *Z, int64_t ldz, const float *s_src,
                                             const float *s_dst, const float *M, const float *L, int64_t n_rows,
                                             int64_t heads, int64_t out_dim, int elu, int cat, float *out, int64_t ldo,
                                             gist_stream_t stream) {
    const char *who = "gist_gat_aggregate_blocks_f32";
    if (heads == 1) cat = 0;      // (one head: nothing to concatenate, and the mean's * 1.0f is exact)
    GIST_REQUIRE(eval_sizes_ok(n_rows, heads, out_dim) && n_blocks >= 0 && n_blocks <= n_rows &&
                     (n_blocks > 0 || n_rows == 0) && n_blocks * kEvalBlock >= n_rows && ldz >= heads * out_dim &&
                     ldo >= (cat ? heads * out_dim : out_dim),
                 "%s: bad sizes", who);
    if (n_rows == 0) return GIST_OK;
    GIST_REQUIRE(rowptr && block_ptr && Z && s_src && s_dst && M && L && out, "%s: null pointer", who);
    const hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)n_blocks), rows((unsigned)ceil_div(n_rows, 4)), wg(256);
    const int H = (int)heads, F = (int)out_dim, c = cat ? 1 : 0;
#define GAT_EVAL_DENSE(NT)                                                                                          \
    hipLaunchKernelGGL(gat_blocks_dense_kernel<NT>, grid, wg, 0, st, rowptr, col, block_ptr, Z, ldz, s_src, s_dst, M, \
                       L, n_rows, H, F, c, out, ldo)
    if (F <= 32) GAT_EVAL_DENSE(1);
    else if (F <= 64) GAT_EVAL_DENSE(2);
    else if (F <= 128) GAT_EVAL_DENSE(4);
    else GAT_EVAL_DENSE(8);
#undef GAT_EVAL_DENSE
    int rc = launch_status("gist_gat_aggregate_blocks_f32 (dense)");
    if (rc) return rc;
    const bool v4 = out_dim % 4 == 0 && ldz % 4 == 0 && ldo % 4 == 0 && aligned16(Z) && aligned16(out);
    const int64_t lanes = ceil_div(out_dim, v4 ? 4 : 1);
    const int lpg = lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64;
    if (v4)
        hipLaunchKernelGGL(gat_blocks_rest_kernel<4>, rows, wg, 0, st, rowptr, col, block_ptr, (int)n_blocks, Z, ldz, s_src,
                           s_dst, M, L, n_rows, H, F, elu ? 1 : 0, c, lpg, out, ldo);
    else
        hipLaunchKernelGGL(gat_blocks_rest_kernel<1>, rows, wg, 0, st, rowptr, col, block_ptr, (int)n_blocks, Z, ldz, s_src,
                           s_dst, M, L, n_rows, H, F, elu ? 1 : 0, c, lpg, out, ldo);
    return launch_status(who);
}
