// Multi-head graph attention (cluster_gcn/modules.py:1-98: GATLayer, MultiHeadGATLayer, GAT) over the in-edge CSR
// of a batch, fp32, no float atomics: every sum has a fixed order, so results are bitwise identical run to run.
//
// Per head h of a layer (Z = x . W^T stacked over heads, [n, H*F]; a_h = [a_src | a_dst], 2F wide):
//   s_src[j,h] = z_h[j] . a_src_h          s_dst[i,h] = z_h[i] . a_dst_h
//   e_hij = leaky_relu(s_src[j,h] + s_dst[i,h], 0.01)      for every in-edge j -> i (duplicates count)
//   alpha_hij = softmax over the in-edges of i             agg_h[i] = sum_j alpha_hij z_h[j]   (0 without in-edges)
//   out[i] = act((1/H) sum_h agg_h[i])                     act = ELU or identity
// or, in the CAT instantiations (the heads concatenated, modules.py:87-89):
//   out[i, hF:(h+1)F] = act(agg_h[i])                       [n, H*F]; G, the gradient into the heads, likewise
//
// Layout of the walkers: one wave per row; the wave's 64 lanes form 64 / LPG edge groups of LPG lanes, a group takes
// every (64 / LPG)-th edge of the row and its lanes cover VEC consecutive columns each.  The groups' partial results
// are combined by an xor butterfly at the end (same operations on every lane of a group, so every lane holds the same
// bits).  Scores of any size are safe: the forward keeps a running max and rescales (online softmax).
#include <math.h>

#include <initializer_list>

#include "common.h"

namespace gist {

constexpr float kGatSlope = 0.01f;       // F.leaky_relu's default negative slope (modules.py:44)
constexpr int kGatRowsPerBlock = 4;      // one row per wave, four waves per workgroup
constexpr int kGatStatRows = 256;        // rows per partial slab of the attention-vector gradient

// sum over the lanes of one group (xor offsets below LPG): pure adds, the same bits in every lane of the group
template <int LPG>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = 1; off < LPG; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// sum over the groups of the wave (xor offsets LPG .. 32)
template <int LPG>
__device__ __forceinline__ float across_groups(float v) {
#pragma unroll
    for (int off = LPG; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// s_src[r, h] = Z[r, hF:(h+1)F] . A[h, 0:F],  s_dst[r, h] = Z[r, hF:(h+1)F] . A[h, F:2F]; one wave per row
__global__ __launch_bounds__(256) void gat_scores_kernel(const float *__restrict__ Z, int64_t ldz,
                                                         const float *__restrict__ A, int64_t n, int H, int F,
                                                         float *__restrict__ s_src, float *__restrict__ s_dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kGatRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *z = Z + row * ldz;
    for (int h = 0; h < H; ++h) {
        const float *a = A + (int64_t)h * 2 * F;
        float ps = 0.f, pd = 0.f;
        for (int c = lane; c < F; c += kWave) {
            const float v = z[(int64_t)h * F + c];
            ps = fmaf(v, a[c], ps);
            pd = fmaf(v, a[F + c], pd);
        }
        ps = wave_sum(ps);
        pd = wave_sum(pd);
        if (lane == 0) {
            s_src[row * H + h] = ps;
            s_dst[row * H + h] = pd;
        }
    }
}

// Forward aggregation: out, and per (row, head) the softmax max M and denominator L (M = L = 0 without in-edges).
// CAT: every head stores its own F columns of the [n, H*F] output (group 0, whole vectors) instead of adding to the mean.
// Its head loop keeps the mean's shape (o starts at 0 and takes acc / l by the same +=), so that the compiler contracts
// the online softmax's a x + b y as it does there and a head has the bits of a one-head layer.
template <int VEC, int LPG, bool CAT>
__global__ __launch_bounds__(256) void gat_aggregate_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ Z, int64_t ldz,
    const float *__restrict__ s_src, const float *__restrict__ s_dst, int64_t n, int H, int F, int elu,
    float *__restrict__ out, int64_t ldo, float *__restrict__ M, float *__restrict__ L) {
    constexpr int G = kWave / LPG;
    const int lane = threadIdx.x & 63;
    const int grp = lane / LPG, li = lane % LPG;
    const int64_t row = (int64_t)blockIdx.x * kGatRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const float inv_h = 1.0f / (float)H;
    for (int c0 = 0; c0 < F; c0 += LPG * VEC) {
        const int c = c0 + li * VEC;
        const bool active = c < F;
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = 0.f;
        for (int h = 0; h < H; ++h) {
            const float sd = s_dst[row * H + h];
            const float *zh = Z + (int64_t)h * F + c;
            float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
            if constexpr (CAT) {      // (no sum over heads: every head starts from 0, as a one-head layer does)
#pragma unroll
                for (int k = 0; k < VEC; ++k) o[k] = 0.f;
            }
            for (int e = e0 + grp; e < e1; e += G) {
                const int j = col[e];
                float s = s_src[(int64_t)j * H + h] + sd;
                s = s > 0.f ? s : kGatSlope * s;
                const float mn = fmaxf(m, s);
                const float corr = expf(m - mn), p = expf(s - mn);
                l = l * corr + p;
                if (active) {
                    float z[VEC];
                    vload<VEC>(zh + (int64_t)j * ldz, z);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * corr + p * z[k];
                }
                m = mn;
            }
#pragma unroll
            for (int off = LPG; off < kWave; off <<= 1) {
                const float mo = __shfl_xor(m, off, kWave), lo = __shfl_xor(l, off, kWave);
                const float mn = fmaxf(m, mo);
                const float ca = m == -INFINITY ? 0.f : expf(m - mn);
                const float cb = mo == -INFINITY ? 0.f : expf(mo - mn);
                // (every lane of a group runs the same operations on the same values: identical bits per group)
                l = l * ca + lo * cb;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float ao = __shfl_xor(acc[k], off, kWave);
                    acc[k] = acc[k] * ca + ao * cb;
                }
                m = mn;
            }
            const float inv_l = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] += acc[k] * inv_l;
            if (c0 == 0 && lane == 0) {
                M[row * H + h] = l > 0.f ? m : 0.f;
                L[row * H + h] = l;
            }
            if constexpr (CAT) {
                if (grp == 0 && active) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) o[k] = (elu && !(o[k] > 0.f)) ? expm1f(o[k]) : o[k];
                    vstore<VEC>(out + row * ldo + (int64_t)h * F + c, o);
                }
            }
        }
        if (!CAT && grp == 0 && active) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float v = o[k] * inv_h;
                o[k] = (elu && !(v > 0.f)) ? expm1f(v) : v;
            }
            vstore<VEC>(out + row * ldo + c, o);
        }
    }
}

// G[i, :] = d_out[i, :] * act'(out[i, :]) / H     (ELU: act' = 1 where out > 0, out + 1 elsewhere)
// CAT: over the H*F columns of the concatenated output, and no division
template <bool CAT>
__global__ __launch_bounds__(256) void gat_grad_in_kernel(const float *__restrict__ d_out, int64_t ldg,
                                                          const float *__restrict__ out, int64_t ldo, int64_t n,
                                                          int F, int H, int elu, float *__restrict__ Gm,
                                                          int64_t ldgm) {
    const int W = CAT ? H * F : F;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * W) return;
    const int64_t r = t / W;
    const int c = (int)(t - r * W);
    float d = d_out[r * ldg + c];
    if (elu) {
        const float o = out[r * ldo + c];
        d *= o > 0.f ? 1.f : o + 1.f;
    }
    Gm[r * ldgm + c] = CAT ? d : d / (float)H;
}

// Backward, destination pass over the in-edge CSR: with gz_hij = G[i] . z_h[j],
//   A = sum_j alpha gz,  B = sum_j alpha lr' gz,  C = sum_j alpha lr'  ->  ds_dst[i,h] = B - A C,  D[i,h] = A
// CAT: head h reads its own slice G[i, hF:(h+1)F] (here and in the source pass)
template <int VEC, int LPG, bool CAT>
__global__ __launch_bounds__(256) void gat_bwd_dst_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ Z, int64_t ldz,
    const float *__restrict__ Gm, int64_t ldgm, const float *__restrict__ s_src, const float *__restrict__ s_dst,
    const float *__restrict__ M, const float *__restrict__ L, int64_t n, int H, int F, float *__restrict__ ds_dst,
    float *__restrict__ D) {
    constexpr int G = kWave / LPG;
    const int lane = threadIdx.x & 63;
    const int grp = lane / LPG, li = lane % LPG;
    const int64_t row = (int64_t)blockIdx.x * kGatRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const float *g0 = Gm + row * ldgm;
    for (int h = 0; h < H; ++h) {
        const float *gi = CAT ? g0 + (int64_t)h * F : g0;
        const float sd = s_dst[row * H + h];
        const float mi = M[row * H + h];
        const float li_ = L[row * H + h];
        const float inv_l = li_ > 0.f ? 1.0f / li_ : 0.f;
        const float *zh = Z + (int64_t)h * F;
        float a = 0.f, b = 0.f, cc = 0.f;
        for (int e = e0 + grp; e < e1; e += G) {
            const int j = col[e];
            const float pre = s_src[(int64_t)j * H + h] + sd;
            const float lr = pre > 0.f ? 1.f : kGatSlope;
            const float alpha = expf(pre * lr - mi) * inv_l;
            float part = 0.f;
            for (int c = li * VEC; c < F; c += LPG * VEC) {
                float g[VEC], z[VEC];
                vload<VEC>(gi + c, g);
                vload<VEC>(zh + (int64_t)j * ldz + c, z);
#pragma unroll
                for (int k = 0; k < VEC; ++k) part = fmaf(g[k], z[k], part);
            }
            const float gz = group_sum<LPG>(part);
            a = fmaf(alpha, gz, a);
            b = fmaf(alpha * lr, gz, b);
            cc = fmaf(alpha, lr, cc);
        }
        a = across_groups<LPG>(a);
        b = across_groups<LPG>(b);
        cc = across_groups<LPG>(cc);
        if (lane == 0) {
            ds_dst[row * H + h] = b - a * cc;
            D[row * H + h] = a;
        }
    }
}

// Backward, source pass over the reversed CSR (row j, its out-edges j -> i):
//   ds_src[j,h] = sum_i alpha_hij (gz_hij - D[i,h]) lr'_hij
//   dZ[j, hF:(h+1)F] = sum_i alpha_hij G[i] + ds_src[j,h] a_src_h + ds_dst[j,h] a_dst_h
template <int VEC, int LPG, bool CAT>
__global__ __launch_bounds__(256) void gat_bwd_src_kernel(
    const int32_t *__restrict__ t_rowptr, const int32_t *__restrict__ t_col, const float *__restrict__ Z,
    int64_t ldz, const float *__restrict__ Gm, int64_t ldgm, const float *__restrict__ A,
    const float *__restrict__ s_src, const float *__restrict__ s_dst, const float *__restrict__ M,
    const float *__restrict__ L, const float *__restrict__ D, const float *__restrict__ ds_dst, int64_t n, int H,
    int F, float *__restrict__ dZ, int64_t lddz, float *__restrict__ ds_src) {
    constexpr int G = kWave / LPG;
    const int lane = threadIdx.x & 63;
    const int grp = lane / LPG, li = lane % LPG;
    const int64_t row = (int64_t)blockIdx.x * kGatRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const int e0 = t_rowptr[row], e1 = t_rowptr[row + 1];
    for (int c0 = 0; c0 < F; c0 += LPG * VEC) {
        const int cw = c0 + li * VEC;             // the columns this lane writes
        const bool active = cw < F;
        for (int h = 0; h < H; ++h) {
            const float ss = s_src[row * H + h];
            const float *zj = Z + row * ldz + (int64_t)h * F;
            float acc[VEC], dsrc = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
            for (int e = e0 + grp; e < e1; e += G) {
                const int64_t i = t_col[e];
                const float pre = ss + s_dst[i * H + h];
                const float lr = pre > 0.f ? 1.f : kGatSlope;
                const float li_ = L[i * H + h];
                const float alpha = expf(pre * lr - M[i * H + h]) / li_;
                const float *gi = Gm + i * ldgm + (CAT ? (int64_t)h * F : 0);
                float part = 0.f;
                for (int c = li * VEC; c < F; c += LPG * VEC) {
                    float g[VEC], z[VEC];
                    vload<VEC>(gi + c, g);
                    vload<VEC>(zj + c, z);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) part = fmaf(g[k], z[k], part);
                    if (c == cw) {                // (the dot's loop passes this lane's output columns once)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[k] = fmaf(alpha, g[k], acc[k]);
                    }
                }
                const float gz = group_sum<LPG>(part);
                dsrc = fmaf(alpha * lr, gz - D[i * H + h], dsrc);
            }
            dsrc = across_groups<LPG>(dsrc);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = across_groups<LPG>(acc[k]);
            if (grp == 0 && active) {
                const float *ah = A + (int64_t)h * 2 * F;
                const float sdj = ds_dst[row * H + h];
                float v[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[k] = acc[k] + dsrc * ah[cw + k] + sdj * ah[F + cw + k];
                vstore<VEC>(dZ + row * lddz + (int64_t)h * F + cw, v);
            }
            if (c0 == 0 && lane == 0) ds_src[row * H + h] = dsrc;
        }
    }
}

// Attention-vector gradient, stage 1: partial[chunk][s][c] = sum over the chunk's rows r of S_s[r, c / F] * Z[r, c]
// (S_0 = ds_src, S_1 = ds_dst); 64 columns x 4 row lanes per workgroup, fixed order
__global__ __launch_bounds__(256) void gat_attn_partial_kernel(const float *__restrict__ Z, int64_t ldz,
                                                               const float *__restrict__ ds_src,
                                                               const float *__restrict__ ds_dst, int64_t n, int H,
                                                               int F, float *__restrict__ partial) {
    __shared__ float red[2][4][64];
    const int HF = H * F;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * kGatStatRows;
    const int64_t r1 = min(r0 + (int64_t)kGatStatRows, n);
    float as = 0.f, ad = 0.f;
    if (c < HF) {
        const int h = c / F;
        for (int64_t r = r0 + rl; r < r1; r += 4) {
            const float z = Z[r * ldz + c];
            as = fmaf(ds_src[r * H + h], z, as);
            ad = fmaf(ds_dst[r * H + h], z, ad);
        }
    }
    red[0][rl][threadIdx.x & 63] = as;
    red[1][rl][threadIdx.x & 63] = ad;
    __syncthreads();
    if (rl < 2 && c < HF) {
        const int t = threadIdx.x & 63;
        const float v = (red[rl][0][t] + red[rl][1][t]) + (red[rl][2][t] + red[rl][3][t]);
        partial[((int64_t)blockIdx.y * 2 + rl) * HF + c] = v;
    }
}

// stage 2: dA[h, s*F + f] = sum over chunks (in order) of partial[chunk][s][h*F + f]
__global__ __launch_bounds__(256) void gat_attn_final_kernel(const float *__restrict__ partial, int64_t chunks,
                                                             int H, int F, float *__restrict__ dA) {
    const int HF = H * F;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * HF) return;
    const int s = t / HF, c = t - s * HF;
    float v = 0.f;
    for (int64_t k = 0; k < chunks; ++k) v += partial[(k * 2 + s) * HF + c];
    const int h = c / F, f = c - h * F;
    dA[(int64_t)h * 2 * F + s * F + f] = v;
}

// Lanes per edge group: enough lanes for a head's F columns at VEC per lane (fewer edge groups for wide heads).
static int gat_lpg(int64_t F, int vec) {
    const int64_t lanes = ceil_div(F, vec);
    return lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64;
}

static bool gat_vec4(int64_t F, std::initializer_list<int64_t> lds, std::initializer_list<const void *> ptrs) {
    if (F % 4) return false;
    for (int64_t ld : lds)
        if (ld % 4) return false;
    for (const void *p : ptrs)
        if (!aligned16(p)) return false;
    return true;
}

#define GAT_DISPATCH(KERNEL, CAT, VEC4, LPG, GRID, ST, ...)                                               \
    do {                                                                                             \
        if (VEC4) {                                                                                  \
            switch (LPG) {                                                                           \
            case 8: hipLaunchKernelGGL((KERNEL<4, 8, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break;   \
            case 16: hipLaunchKernelGGL((KERNEL<4, 16, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break; \
            case 32: hipLaunchKernelGGL((KERNEL<4, 32, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break; \
            default: hipLaunchKernelGGL((KERNEL<4, 64, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break; \
            }                                                                                        \
        } else {                                                                                     \
            switch (LPG) {                                                                           \
            case 8: hipLaunchKernelGGL((KERNEL<1, 8, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break;   \
            case 16: hipLaunchKernelGGL((KERNEL<1, 16, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break; \
            case 32: hipLaunchKernelGGL((KERNEL<1, 32, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break; \
            default: hipLaunchKernelGGL((KERNEL<1, 64, CAT>), GRID, dim3(256), 0, ST, __VA_ARGS__); break; \
            }                                                                                        \
        }                                                                                            \
    } while (0)

static bool gat_sizes_ok(int64_t n, int64_t H, int64_t F) {
    return n >= 0 && n < (int64_t)1 << 31 && H >= 1 && F >= 1 && H * F < (int64_t)1 << 31;
}

}  // namespace gist

using namespace gist;

extern "C" int gist_gat_scores_f32(const float *Z, int64_t ldz, const float *A, int64_t n_rows, int64_t heads,
                                   int64_t out_dim, float *s_src, float *s_dst, gist_stream_t stream) {
    // (every entry point: no pointer is read without rows -- torch hands NULL for a tensor without elements)
    GIST_REQUIRE(gat_sizes_ok(n_rows, heads, out_dim) && ldz >= heads * out_dim, "gist_gat_scores_f32: bad sizes");
    if (n_rows == 0) return GIST_OK;
    GIST_REQUIRE(Z && A && s_src && s_dst, "gist_gat_scores_f32: null pointer");
    hipLaunchKernelGGL(gat_scores_kernel, dim3((unsigned)ceil_div(n_rows, kGatRowsPerBlock)), dim3(256), 0,
                       as_stream(stream), Z, ldz, A, n_rows, (int)heads, (int)out_dim, s_src, s_dst);
    return launch_status("gist_gat_scores_f32");
}

// The three entry points that know how the heads are combined, once for both ways: CAT = false is the head mean
// (gist_gat_*_f32), CAT = true the concatenation (gist_gat_*_cat_f32), where out, d_out and G are heads * out_dim wide.
template <bool CAT>
static int gat_aggregate(const char *who, const int32_t *rowptr, const int32_t *col, const float *Z, int64_t ldz,
                         const float *s_src, const float *s_dst, int64_t n_rows, int64_t heads, int64_t out_dim,
                         int elu, float *out, int64_t ldo, float *M, float *L, gist_stream_t stream) {
    if constexpr (CAT) {      // (one head: nothing to concatenate, and the mean's * 1.0f is exact)
        if (heads == 1)
            return gat_aggregate<false>(who, rowptr, col, Z, ldz, s_src, s_dst, n_rows, heads, out_dim, elu, out, ldo, M,
                                        L, stream);
    }
    GIST_REQUIRE(gat_sizes_ok(n_rows, heads, out_dim) && ldz >= heads * out_dim &&
                     ldo >= (CAT ? heads * out_dim : out_dim),
                 "%s: bad sizes", who);
    if (n_rows == 0) return GIST_OK;
    // (col is read only inside rowptr's ranges: it may be NULL for a graph without edges, as in gist_spmm_csr_f32)
    GIST_REQUIRE(rowptr && Z && s_src && s_dst && out && M && L, "%s: null pointer", who);
    const bool v4 = gat_vec4(out_dim, {ldz, ldo}, {Z, out});
    const int lpg = gat_lpg(out_dim, v4 ? 4 : 1);
    const dim3 grid((unsigned)ceil_div(n_rows, kGatRowsPerBlock));
    GAT_DISPATCH(gat_aggregate_kernel, CAT, v4, lpg, grid, as_stream(stream), rowptr, col, Z, ldz, s_src, s_dst,
                 n_rows, (int)heads, (int)out_dim, elu ? 1 : 0, out, ldo, M, L);
    return launch_status(who);
}

template <bool CAT>
static int gat_backward_dst(const char *who, const int32_t *rowptr, const int32_t *col, const float *Z, int64_t ldz,
                            const float *out, int64_t ldo, const float *d_out, int64_t ldg, const float *s_src,
                            const float *s_dst, const float *M, const float *L, int64_t n_rows, int64_t heads,
                            int64_t out_dim, int elu, float *G, int64_t ldgm, float *ds_dst, float *D,
                            gist_stream_t stream) {
    if constexpr (CAT) {      // (one head: the mean's / 1.0f is exact)
        if (heads == 1)
            return gat_backward_dst<false>(who, rowptr, col, Z, ldz, out, ldo, d_out, ldg, s_src, s_dst, M, L, n_rows,
                                           heads, out_dim, elu, G, ldgm, ds_dst, D, stream);
    }
    const int64_t width = CAT ? heads * out_dim : out_dim;      // of out, d_out and G
    GIST_REQUIRE(gat_sizes_ok(n_rows, heads, out_dim) && ldz >= heads * out_dim && ldg >= width && ldgm >= width &&
                     (!elu || ldo >= width),
                 "%s: bad sizes", who);
    if (n_rows == 0) return GIST_OK;
    GIST_REQUIRE(rowptr && Z && d_out && s_src && s_dst && M && L && G && ds_dst && D && (out || !elu),
                 "%s: null pointer", who);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(gat_grad_in_kernel<CAT>, dim3((unsigned)ceil_div(n_rows * width, 256)), dim3(256), 0, st,
                       d_out, ldg, out, ldo, n_rows, (int)out_dim, (int)heads, elu ? 1 : 0, G, ldgm);
    int rc = launch_status(who);
    if (rc) return rc;
    const bool v4 = gat_vec4(out_dim, {ldz, ldgm}, {Z, G});
    const int lpg = gat_lpg(out_dim, v4 ? 4 : 1);
    const dim3 grid((unsigned)ceil_div(n_rows, kGatRowsPerBlock));
    GAT_DISPATCH(gat_bwd_dst_kernel, CAT, v4, lpg, grid, st, rowptr, col, Z, ldz, G, ldgm, s_src, s_dst, M, L, n_rows,
                 (int)heads, (int)out_dim, ds_dst, D);
    return launch_status(who);
}

template <bool CAT>
static int gat_backward_src(const char *who, const int32_t *t_rowptr, const int32_t *t_col, const float *Z,
                            int64_t ldz, const float *G, int64_t ldgm, const float *A, const float *s_src,
                            const float *s_dst, const float *M, const float *L, const float *D, const float *ds_dst,
                            int64_t n_rows, int64_t heads, int64_t out_dim, float *dZ, int64_t lddz, float *ds_src,
                            gist_stream_t stream) {
    if constexpr (CAT) {
        if (heads == 1)
            return gat_backward_src<false>(who, t_rowptr, t_col, Z, ldz, G, ldgm, A, s_src, s_dst, M, L, D, ds_dst,
                                           n_rows, heads, out_dim, dZ, lddz, ds_src, stream);
    }
    GIST_REQUIRE(gat_sizes_ok(n_rows, heads, out_dim) && ldz >= heads * out_dim && lddz >= heads * out_dim &&
                     ldgm >= (CAT ? heads * out_dim : out_dim),
                 "%s: bad sizes", who);
    if (n_rows == 0) return GIST_OK;
    GIST_REQUIRE(t_rowptr && Z && G && A && s_src && s_dst && M && L && D && ds_dst && dZ && ds_src,
                 "%s: null pointer", who);
    const bool v4 = gat_vec4(out_dim, {ldz, ldgm, lddz}, {Z, G, dZ});
    const int lpg = gat_lpg(out_dim, v4 ? 4 : 1);
    const dim3 grid((unsigned)ceil_div(n_rows, kGatRowsPerBlock));
    GAT_DISPATCH(gat_bwd_src_kernel, CAT, v4, lpg, grid, as_stream(stream), t_rowptr, t_col, Z, ldz, G, ldgm, A,
                 s_src, s_dst, M, L, D, ds_dst, n_rows, (int)heads, (int)out_dim, dZ, lddz, ds_src);
    return launch_status(who);
}

extern "C" int gist_gat_aggregate_f32(const int32_t *rowptr, const int32_t *col, const float *Z, int64_t ldz,
    const float *s_src, const float *s_dst, int64_t n_rows, int64_t heads, int64_t out_dim, int elu, float *out,
    int64_t ldo, float *M, float *L, gist_stream_t stream) {
    return gat_aggregate<false>("gist_gat_aggregate_f32", rowptr, col, Z, ldz, s_src, s_dst, n_rows, heads, out_dim, elu, out,
                              ldo, M, L, stream);
}

extern "C" int gist_gat_aggregate_cat_f32(const int32_t *rowptr, const int32_t *col, const float *Z, int64_t ldz,
    const float *s_src, const float *s_dst, int64_t n_rows, int64_t heads, int64_t out_dim, int elu, float *out,
    int64_t ldo, float *M, float *L, gist_stream_t stream) {
    return gat_aggregate<true>("gist_gat_aggregate_cat_f32", rowptr, col, Z, ldz, s_src, s_dst, n_rows, heads, out_dim, elu, out,
                             ldo, M, L, stream);
}

extern "C" int gist_gat_backward_dst_f32(const int32_t *rowptr, const int32_t *col, const float *Z, int64_t ldz,
    const float *out, int64_t ldo, const float *d_out, int64_t ldg, const float *s_src, const float *s_dst,
    const float *M, const float *L, int64_t n_rows, int64_t heads, int64_t out_dim, int elu, float *G, int64_t ldgm,
    float *ds_dst, float *D, gist_stream_t stream) {
    return gat_backward_dst<false>("gist_gat_backward_dst_f32", rowptr, col, Z, ldz, out, ldo, d_out, ldg, s_src, s_dst, M, L,
                                 n_rows, heads, out_dim, elu, G, ldgm, ds_dst, D, stream);
}

extern "C" int gist_gat_backward_dst_cat_f32(const int32_t *rowptr, const int32_t *col, const float *Z, int64_t ldz,
    const float *out, int64_t ldo, const float *d_out, int64_t ldg, const float *s_src, const float *s_dst,
    const float *M, const float *L, int64_t n_rows, int64_t heads, int64_t out_dim, int elu, float *G, int64_t ldgm,
    float *ds_dst, float *D, gist_stream_t stream) {
    return gat_backward_dst<true>("gist_gat_backward_dst_cat_f32", rowptr, col, Z, ldz, out, ldo, d_out, ldg, s_src, s_dst, M, L,
                                n_rows, heads, out_dim, elu, G, ldgm, ds_dst, D, stream);
}

extern "C" int gist_gat_backward_src_f32(const int32_t *t_rowptr, const int32_t *t_col, const float *Z, int64_t ldz,
    const float *G, int64_t ldgm, const float *A, const float *s_src, const float *s_dst, const float *M, const float *L,
    const float *D, const float *ds_dst, int64_t n_rows, int64_t heads, int64_t out_dim, float *dZ, int64_t lddz,
    float *ds_src, gist_stream_t stream) {
    return gat_backward_src<false>("gist_gat_backward_src_f32", t_rowptr, t_col, Z, ldz, G, ldgm, A, s_src, s_dst, M, L, D,
                                 ds_dst, n_rows, heads, out_dim, dZ, lddz, ds_src, stream);
}

extern "C" int gist_gat_backward_src_cat_f32(const int32_t *t_rowptr, const int32_t *t_col, const float *Z, int64_t ldz,
    const float *G, int64_t ldgm, const float *A, const float *s_src, const float *s_dst, const float *M, const float *L,
    const float *D, const float *ds_dst, int64_t n_rows, int64_t heads, int64_t out_dim, float *dZ, int64_t lddz,
    float *ds_src, gist_stream_t stream) {
    return gat_backward_src<true>("gist_gat_backward_src_cat_f32", t_rowptr, t_col, Z, ldz, G, ldgm, A, s_src, s_dst, M, L, D,
                                ds_dst, n_rows, heads, out_dim, dZ, lddz, ds_src, stream);
}

extern "C" int64_t gist_gat_attn_grad_workspace_floats(int64_t n_rows, int64_t heads, int64_t out_dim) {
    if (n_rows <= 0 || heads <= 0 || out_dim <= 0) return 0;
    return ceil_div(n_rows, kGatStatRows) * 2 * heads * out_dim;
}

extern "C" int gist_gat_attn_grad_f32(const float *Z, int64_t ldz, const float *ds_src, const float *ds_dst,
                                      int64_t n_rows, int64_t heads, int64_t out_dim, float *partials,
                                      int64_t partial_floats, float *dA, gist_stream_t stream) {
    GIST_REQUIRE(gat_sizes_ok(n_rows, heads, out_dim) && ldz >= heads * out_dim, "gist_gat_attn_grad_f32: bad sizes");
    GIST_REQUIRE(dA && (n_rows == 0 || (Z && ds_src && ds_dst)), "gist_gat_attn_grad_f32: null pointer");
    const int64_t need = gist_gat_attn_grad_workspace_floats(n_rows, heads, out_dim);
    if (need > 0 && (!partials || partial_floats < need)) {
        set_error("gist_gat_attn_grad_f32: workspace too small (%lld < %lld floats)", (long long)partial_floats,
                  (long long)need);
        return GIST_ENOSPACE;
    }
    const hipStream_t st = as_stream(stream);
    const int64_t hf = heads * out_dim;
    const int64_t chunks = ceil_div(n_rows, kGatStatRows);
    if (chunks > 0) {
        hipLaunchKernelGGL(gat_attn_partial_kernel, dim3((unsigned)ceil_div(hf, 64), (unsigned)chunks), dim3(256), 0,
                           st, Z, ldz, ds_src, ds_dst, n_rows, (int)heads, (int)out_dim, partials);
        int rc = launch_status("gist_gat_attn_grad_f32 (partials)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(gat_attn_final_kernel, dim3((unsigned)ceil_div(2 * hf, 256)), dim3(256), 0, st, partials,
                       chunks, (int)heads, (int)out_dim, dA);
    return launch_status("gist_gat_attn_grad_f32");
}
