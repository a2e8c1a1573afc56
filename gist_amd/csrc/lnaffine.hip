// The tail of a GraphSAGELayer on gfx950 (cluster_gcn/modules.py:120,144-147): projection bias + LayerNorm WITH affine
// + ReLU in one forward launch, and a backward that leaves dx and the three column sums (d gamma, d beta, d bias of the
// projection) as partials per 16-row chunk, finished in a fixed order by a second launch.  No float atomics.  The
// forward's DROP instantiations (gist_ln_affine_fwd_drop_f32) also fold the NEXT layer's dropout into the store: out
// under gist_dropout_f32's mask, the undropped value to out2.  Its inference instantiations (gist_ln_affine_infer_f32,
// the full-graph evaluator's tail) store out alone.
//
// A row is owned by one wave (d <= 1024) or by one 256-thread workgroup; with up to kE = 16 elements per thread it
// stays in registers (d <= 16 * TPR: every wave row, workgroup rows up to 4096) and is read once; wider rows are
// re-read.  VEC = 4: a thread's elements are quads (16-byte accesses); VEC = 1: single floats, lane-strided.
#include "common.h"

namespace gist {
namespace {

constexpr int kE = 16;
constexpr int kChunkRows = 16;      // gist_row_chunks16

// gamma * yhat + beta as ONE fused multiply-add: the forward's ReLU and the backward's gate call this on the same
// float32 operands, so they see the same bits
__device__ __forceinline__ float affine_pre(float yh, float g, float b) { return fmaf(g, yh, b); }

// column of element e of thread t
template <int TPR, int VEC>
__device__ __forceinline__ int elem_col(int t, int e) {
    if constexpr (VEC == 4) return t * 4 + (e >> 2) * (TPR * 4) + (e & 3);
    else return t + e * TPR;
}

// the thread's kE elements of p[0..d) (0.f past d, or when !live)
template <int TPR, int VEC>
__device__ __forceinline__ void load_elems(float (&v)[kE], const float *p, int t, int d, bool live) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int u = 0; u < kE / 4; ++u) {
            const int c = t * 4 + u * (TPR * 4);
            const float4 q = (live && c < d) ? *reinterpret_cast<const float4 *>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            const int c = t + e * TPR;
            v[e] = (live && c < d) ? p[c] : 0.f;
        }
    }
}

template <int TPR, int VEC>
__device__ __forceinline__ void store_elems(const float (&v)[kE], float *p, int t, int d) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int u = 0; u < kE / 4; ++u) {
            const int c = t * 4 + u * (TPR * 4);
            if (c < d) *reinterpret_cast<float4 *>(p + c) = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            const int c = t + e * TPR;
            if (c < d) p[c] = v[e];
        }
    }
}

// the thread's share of a row sum: quads pairwise, single floats in order
template <int VEC>
__device__ __forceinline__ float sum_elems(const float (&v)[kE]) {
    float s = 0.f;
    if constexpr (VEC == 4) {
#pragma unroll
        for (int u = 0; u < kE / 4; ++u) s += (v[4 * u] + v[4 * u + 1]) + (v[4 * u + 2] + v[4 * u + 3]);
    } else {
#pragma unroll
        for (int e = 0; e < kE; ++e) s += v[e];
    }
    return s;
}

// VEC consecutive floats at p (re-reading path).  Not kernel_kit.h's vload / vstore / vsum on float[VEC]: written
// that way the five TPR = 256 kernels that re-read come out with other address arithmetic and more instructions.
template <int VEC>
struct Pack { float v[VEC]; };
template <int VEC>
__device__ __forceinline__ Pack<VEC> ld(const float *p) {
    Pack<VEC> r;
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void st(float *p, const Pack<VEC> &r) {
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}
template <int VEC>
__device__ __forceinline__ float sum_pack(const Pack<VEC> &r) {
    if constexpr (VEC == 4) return (r.v[0] + r.v[1]) + (r.v[2] + r.v[3]);
    else return r.v[0];
}

// The next layer's dropout folded into the forward's store (gist_ln_affine_fwd_drop_f32): what goes to row r, column c
// of `out` is multiplied by gist_dropout_f32's keep/scale factor of element offset + r * mask_ld + c (m.p = 0: no mask,
// nothing hashed); the value before the mask goes to out2 (NULL: none).  Only the DROP instantiations read it.
struct LnaDrop {
    float *out2; int64_t ldo2;
    DropMask m;
    uint64_t offset;
    int64_t mask_ld;
};

// the mask on the thread's kE elements of the row whose element 0 has index ibase
template <int TPR, int VEC>
__device__ __forceinline__ void mask_elems(float (&v)[kE], uint64_t ibase, int t, int d, const DropMask &m) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int u = 0; u < kE / 4; ++u) {
            const int c = t * 4 + u * (TPR * 4);
            if (c < d) {
                float4 q = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
                drop_f4(q, ibase + (uint64_t)c, m);
                v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            const int c = t + e * TPR;
            if (c < d) v[e] *= drop_keep(ibase + (uint64_t)c, m);
        }
    }
}

// ---------------------------------------------------------------------------
// forward: v = x + lin_bias; yhat = (v - mean) * rstd; out = relu?(gamma * yhat + beta)
// kLnaDrop: out2 = that value, out = it under the next layer's dropout mask (LnaDrop)
// kLnaInfer: the same arithmetic in the same order, but yhat and rstd stay in registers (both pointers NULL): only out is
// stored (gist_ln_affine_infer_f32)
// ---------------------------------------------------------------------------
enum LnaMode { kLnaTrain = 0, kLnaDrop = 1, kLnaInfer = 2 };

template <int TPR, int VEC, int MODE = kLnaTrain>
__global__ __launch_bounds__(256) void ln_affine_fwd_kernel(
    const float *__restrict__ x, int64_t ldx, const float *__restrict__ lin_bias, const float *__restrict__ gamma,
    const float *__restrict__ beta, float *__restrict__ yhat, int64_t ldy, float *__restrict__ out, int64_t ldo,
    float *__restrict__ rstd_out, int n_rows, int d, int relu, float eps, LnaDrop dr) {
    __shared__ float red[4];
    constexpr int RPB = 256 / TPR;
    constexpr bool DROP = MODE == kLnaDrop, SAVE = MODE != kLnaInfer;      // SAVE: yhat and rstd are written
    const int row = blockIdx.x * RPB + threadIdx.x / TPR;
    const int t = threadIdx.x % TPR;
    const bool live = row < n_rows;
    const float *xr = x + (int64_t)(live ? row : 0) * ldx;
    float *yr = nullptr;
    if constexpr (SAVE) yr = yhat + (int64_t)(live ? row : 0) * ldy;
    float *orow = out + (int64_t)(live ? row : 0) * ldo;
    float *o2row = nullptr;
    uint64_t ibase = 0;
    if constexpr (DROP) {
        if (dr.out2 != nullptr) o2row = dr.out2 + (int64_t)(live ? row : 0) * dr.ldo2;
        ibase = dr.offset + (uint64_t)(live ? row : 0) * (uint64_t)dr.mask_ld;
    }
    if (TPR == 64 || d <= kE * TPR) {
        float v[kE];
        load_elems<TPR, VEC>(v, xr, t, d, live);
        if (lin_bias != nullptr) {
            float b[kE];
            load_elems<TPR, VEC>(b, lin_bias, t, d, live);
#pragma unroll
            for (int e = 0; e < kE; ++e) v[e] += b[e];
        }
        const float mean = row_sum<TPR>(sum_elems<VEC>(v), red) / (float)d;
        float sq[kE];
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            v[e] = elem_col<TPR, VEC>(t, e) < d ? v[e] - mean : 0.f;
            sq[e] = v[e] * v[e];
        }
        const float var = row_sum<TPR>(sum_elems<VEC>(sq), red) / (float)d;
        const float rstd = 1.0f / sqrtf(var + eps);
        if (!live) return;
        if constexpr (SAVE) {
            if (t == 0) rstd_out[row] = rstd;
        }
#pragma unroll
        for (int e = 0; e < kE; ++e) v[e] *= rstd;
        if constexpr (SAVE) store_elems<TPR, VEC>(v, yr, t, d);
        float g[kE], b[kE];
        load_elems<TPR, VEC>(g, gamma, t, d, true);
        load_elems<TPR, VEC>(b, beta, t, d, true);
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            v[e] = affine_pre(v[e], g[e], b[e]);
            if (relu) v[e] = fmaxf(v[e], 0.f);
        }
        if constexpr (DROP) {
            if (o2row != nullptr) store_elems<TPR, VEC>(v, o2row, t, d);
            if (dr.m.p > 0.f) mask_elems<TPR, VEC>(v, ibase, t, d, dr.m);
        }
        store_elems<TPR, VEC>(v, orow, t, d);
        return;
    }
    if constexpr (TPR == 256) {      // d > 4096: the row is read three times (the workgroup is the row: live is uniform)
        auto value = [&](int c) {
            Pack<VEC> p = ld<VEC>(xr + c);
            if (lin_bias != nullptr) {
                const Pack<VEC> b = ld<VEC>(lin_bias + c);
#pragma unroll
                for (int k = 0; k < VEC; ++k) p.v[k] += b.v[k];
            }
            return p;
        };
        float s = 0.f;
        for (int c = t * VEC; c < d; c += 256 * VEC) s += sum_pack<VEC>(value(c));
        const float mean = row_sum<TPR>(s, red) / (float)d;
        float q = 0.f;
        for (int c = t * VEC; c < d; c += 256 * VEC) {
            Pack<VEC> p = value(c);
#pragma unroll
            for (int k = 0; k < VEC; ++k) { p.v[k] -= mean; p.v[k] *= p.v[k]; }
            q += sum_pack<VEC>(p);
        }
        const float var = row_sum<TPR>(q, red) / (float)d;
        const float rstd = 1.0f / sqrtf(var + eps);
        if constexpr (SAVE) {
            if (t == 0) rstd_out[row] = rstd;
        }
        for (int c = t * VEC; c < d; c += 256 * VEC) {
            Pack<VEC> p = value(c);
            const Pack<VEC> g = ld<VEC>(gamma + c), b = ld<VEC>(beta + c);
#pragma unroll
            for (int k = 0; k < VEC; ++k) p.v[k] = (p.v[k] - mean) * rstd;
            if constexpr (SAVE) st<VEC>(yr + c, p);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                p.v[k] = affine_pre(p.v[k], g.v[k], b.v[k]);
                if (relu) p.v[k] = fmaxf(p.v[k], 0.f);
            }
            if constexpr (DROP) {
                if (o2row != nullptr) st<VEC>(o2row + c, p);
                if (dr.m.p > 0.f) drop_vec<VEC>(p.v, ibase + (uint64_t)c, dr.m);
            }
            st<VEC>(orow + c, p);
        }
    }
}

// ---------------------------------------------------------------------------
// backward.  g' = d_out * [pre > 0] (strict: no gradient at 0), dyh = g' * gamma,
//   dx = rstd * (dyh - mean(dyh) - yhat * mean(dyh * yhat))
// and, per 16-row chunk (one workgroup), the column sums of g' * yhat, g' and dx:
//   partials[s][chunk][0..d), s = 0 d gamma, 1 d beta, 2 d lin_bias (only when n_sums = 3).
// Order inside a chunk: TPR = 64: wave w adds its rows r0 + w + 4 j in j order, then ((w0 + w1) + w2) + w3 through LDS
// (the order of gist_ln_relu_bwd_colsum_f32); TPR = 256: the owner thread of a column adds the rows in order.
// ---------------------------------------------------------------------------
template <int TPR, int VEC>
__global__ __launch_bounds__(256) void ln_affine_bwd_kernel(
    const float *__restrict__ d_out, int64_t ldg, const float *__restrict__ yhat, int64_t ldy,
    const float *__restrict__ rstd_in, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ dx, int64_t lddx, int n_rows, int d, int relu, float *__restrict__ partials, int n_sums) {
    __shared__ float red[4];
    __shared__ __attribute__((aligned(16))) float part[TPR == 64 ? 3 * 1024 : 4];
    const int t = threadIdx.x % TPR, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * kChunkRows;
    const int64_t plane = (int64_t)gridDim.x * d;
    float *ps = partials + (int64_t)blockIdx.x * d;      // + s * plane
    constexpr int NR = TPR == 64 ? kChunkRows / 4 : kChunkRows;
    auto row_of = [&](int j) { return TPR == 64 ? r0 + wave + 4 * j : r0 + j; };
    if (TPR == 64 || d <= kE * TPR) {
        float ga[kE], be[kE];
        load_elems<TPR, VEC>(ga, gamma, t, d, true);
        load_elems<TPR, VEC>(be, beta, t, d, true);
        float cs[3][kE];
#pragma unroll
        for (int e = 0; e < kE; ++e) cs[0][e] = cs[1][e] = cs[2][e] = 0.f;
        auto load = [&](float (&g)[kE], float (&y)[kE], int j) {
            const int row = row_of(j);
            const bool live = j < NR && row < n_rows;
            load_elems<TPR, VEC>(g, d_out + (int64_t)(live ? row : 0) * ldg, t, d, live);
            load_elems<TPR, VEC>(y, yhat + (int64_t)(live ? row : 0) * ldy, t, d, live);
        };
        auto process = [&](float (&g)[kE], float (&y)[kE], int row) {      // (elements past d: g = y = gamma = 0)
            float a[kE], b[kE];
#pragma unroll
            for (int e = 0; e < kE; ++e) {
                if (relu) g[e] = affine_pre(y[e], ga[e], be[e]) > 0.f ? g[e] : 0.f;
                a[e] = g[e] * ga[e];
                b[e] = a[e] * y[e];
            }
            const float m1 = row_sum<TPR>(sum_elems<VEC>(a), red) / (float)d;
            const float m2 = row_sum<TPR>(sum_elems<VEC>(b), red) / (float)d;
            const float rstd = rstd_in[row];
#pragma unroll
            for (int e = 0; e < kE; ++e) {
                a[e] = elem_col<TPR, VEC>(t, e) < d ? rstd * (a[e] - m1 - y[e] * m2) : 0.f;
                cs[0][e] += g[e] * y[e];
                cs[1][e] += g[e];
                cs[2][e] += a[e];
            }
            store_elems<TPR, VEC>(a, dx + (int64_t)row * lddx, t, d);
        };
        // the next row's loads are issued before the current row's reductions
        float gA[kE], yA[kE], gB[kE], yB[kE];
        load(gA, yA, 0);
        for (int j = 0; j < NR; j += 2) {
            if (row_of(j) >= n_rows) break;
            load(gB, yB, j + 1);
            process(gA, yA, row_of(j));
            if (row_of(j + 1) >= n_rows) break;
            load(gA, yA, j + 2);
            process(gB, yB, row_of(j + 1));
        }
        if constexpr (TPR == 256) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (s < n_sums) store_elems<TPR, VEC>(cs[s], ps + s * plane, t, d);
        } else {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (s >= n_sums) break;                           // uniform
                __syncthreads();                                  // part[] of the previous sum has been read
                if (wave > 0) store_elems<TPR, VEC>(cs[s], part + (wave - 1) * 1024, t, 1024);
                __syncthreads();
                if (wave == 0) {
                    float o[kE];
#pragma unroll
                    for (int e = 0; e < kE; ++e) {
                        const int c = elem_col<TPR, VEC>(t, e);
                        o[e] = ((cs[s][e] + part[c]) + part[1024 + c]) + part[2048 + c];
                    }
                    store_elems<TPR, VEC>(o, ps + s * plane, t, d);
                }
            }
        }
        return;
    }
    if constexpr (TPR == 256) {
        // d > 4096: two reads of a row; a column's sums live in the partials themselves, which only the thread that
        // owns the column touches (written at the chunk's first row, added to in row order after it)
        for (int j = 0; j < kChunkRows; ++j) {
            const int row = r0 + j;
            if (row >= n_rows) break;                             // uniform
            const float *gr = d_out + (int64_t)row * ldg, *yr = yhat + (int64_t)row * ldy;
            float *dr = dx + (int64_t)row * lddx;
            auto gated = [&](int c, Pack<VEC> &g, Pack<VEC> &a, const Pack<VEC> &y) {      // g <- g', a <- g' * gamma
                const Pack<VEC> gm = ld<VEC>(gamma + c), bt = ld<VEC>(beta + c);
                g = ld<VEC>(gr + c);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    if (relu) g.v[k] = affine_pre(y.v[k], gm.v[k], bt.v[k]) > 0.f ? g.v[k] : 0.f;
                    a.v[k] = g.v[k] * gm.v[k];
                }
            };
            float s1 = 0.f, s2 = 0.f;
            for (int c = t * VEC; c < d; c += 256 * VEC) {
                const Pack<VEC> y = ld<VEC>(yr + c);
                Pack<VEC> g, a, b;
                gated(c, g, a, y);
#pragma unroll
                for (int k = 0; k < VEC; ++k) b.v[k] = a.v[k] * y.v[k];
                s1 += sum_pack<VEC>(a);
                s2 += sum_pack<VEC>(b);
            }
            const float m1 = row_sum<TPR>(s1, red) / (float)d;
            const float m2 = row_sum<TPR>(s2, red) / (float)d;
            const float rstd = rstd_in[row];
            for (int c = t * VEC; c < d; c += 256 * VEC) {
                const Pack<VEC> y = ld<VEC>(yr + c);
                Pack<VEC> g, a, sums[3];
                gated(c, g, a, y);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    a.v[k] = rstd * (a.v[k] - m1 - y.v[k] * m2);
                    sums[0].v[k] = g.v[k] * y.v[k];
                    sums[1].v[k] = g.v[k];
                    sums[2].v[k] = a.v[k];
                }
                st<VEC>(dr + c, a);
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (s >= n_sums) break;
                    if (j > 0) {
                        const Pack<VEC> old = ld<VEC>(ps + s * plane + c);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) sums[s].v[k] = old.v[k] + sums[s].v[k];
                    }
                    st<VEC>(ps + s * plane + c, sums[s]);
                }
            }
        }
    }
}

// out[s][c] = the chunks' partials of sum s added in gist_colsum_chunks_f32's order: four partial sums over the chunks
// q, q + 4, ... (ascending), then ((q0 + q1) + q2) + q3.  blockIdx.y = s.
struct LnAffineOuts { float *p[3]; };

__global__ __launch_bounds__(256) void ln_affine_finish_kernel(const float *__restrict__ partials, int chunks, int d,
                                                              LnAffineOuts outs) {
    __shared__ float part[3][64];
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + e;
    const float *ps = partials + (int64_t)blockIdx.y * chunks * d;
    float acc = 0.f;
    if (c < d)
        for (int k = q; k < chunks; k += 4) acc += ps[(int64_t)k * d + c];
    if (q > 0) part[q - 1][e] = acc;
    __syncthreads();
    if (q == 0 && c < d) outs.p[blockIdx.y][c] = ((acc + part[0][e]) + part[1][e]) + part[2][e];
}

}  // namespace
}  // namespace gist

namespace gist {
// drop = NULL, or p = 0 and out2 = NULL: the plain instantiations.  infer (gist_ln_affine_infer_f32; no drop): yhat and
// rstd are NULL and ldy is 0 -- not required, not in the vector predicate, not written; everything else is the same
// decision: a call whose yhat shares out's pitch and alignment class picks the same (regime, VEC) either way
static int ln_affine_fwd_ex(const char *name, const float *x, int64_t ldx, const float *lin_bias, const float *gamma,
                            const float *beta, float *yhat, int64_t ldy, float *out, int64_t ldo, float *rstd,
                            int64_t n_rows, int64_t d, int relu, float eps, const LnaDrop *drop, bool infer,
                            hipStream_t st) {
    GIST_REQUIRE(n_rows >= 0 && d >= 0, "%s: negative size", name);
    if (n_rows == 0 || d == 0) return GIST_OK;
    GIST_REQUIRE(x && gamma && beta && out && (infer || (yhat && rstd)), "%s: null pointer", name);
    GIST_REQUIRE(ldx >= d && (infer || ldy >= d) && ldo >= d, "%s: leading dimension < d", name);
    GIST_REQUIRE(n_rows < (1LL << 31) && d < (1LL << 31), "%s: size >= 2^31", name);
    GIST_REQUIRE(eps >= 0.f, "%s: negative eps", name);
    bool v4 = d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(yhat) &&
              aligned16(out) && aligned16(gamma) && aligned16(beta) && aligned16(lin_bias);
    LnaDrop dr{};
    const bool dropping = !infer && drop != nullptr && (drop->m.p > 0.f || drop->out2 != nullptr);
    if (dropping) {
        dr = *drop;
        if (dr.out2 != nullptr) {
            GIST_REQUIRE(dr.ldo2 >= d, "%s: leading dimension < d", name);
            v4 = v4 && dr.ldo2 % 4 == 0 && aligned16(dr.out2);
        }
    }
    const bool wide = d > 1024;
    const unsigned grid = (unsigned)(wide ? n_rows : ceil_div(n_rows, 4));
#define LM(TPR, V, MODE)                                                                                              \
    hipLaunchKernelGGL((ln_affine_fwd_kernel<TPR, V, MODE>), dim3(grid), dim3(256), 0, st, x, ldx, lin_bias, gamma, beta, \
                       yhat, ldy, out, ldo, rstd, (int)n_rows, (int)d, relu, eps, dr)
#define L(TPR, V)                                                                                                     \
    do {                                                                                                              \
        if (infer) LM(TPR, V, kLnaInfer);                                                                             \
        else if (dropping) LM(TPR, V, kLnaDrop);                                                                      \
        else LM(TPR, V, kLnaTrain);                                                                                   \
    } while (0)
    if (wide) { if (v4) L(256, 4); else L(256, 1); }
    else { if (v4) L(64, 4); else L(64, 1); }
#undef L
#undef LM
    return launch_status(name);
}
}  // namespace gist

extern "C" int gist_ln_affine_fwd_f32(const float *x, int64_t ldx, const float *lin_bias, const float *gamma,
                                      const float *beta, float *yhat, int64_t ldy, float *out, int64_t ldo,
                                      float *rstd, int64_t n_rows, int64_t d, int relu, float eps,
                                      gist_stream_t stream) {
    return gist::ln_affine_fwd_ex("gist_ln_affine_fwd_f32", x, ldx, lin_bias, gamma, beta, yhat, ldy, out, ldo, rstd,
                                  n_rows, d, relu, eps, nullptr, false, gist::as_stream(stream));
}

extern "C" int gist_ln_affine_fwd_drop_f32(const float *x, int64_t ldx, const float *lin_bias, const float *gamma,
                                           const float *beta, float *yhat, int64_t ldy, float *out, int64_t ldo,
                                           float *out2, int64_t ldo2, float *rstd, int64_t n_rows, int64_t d, int relu,
                                           float eps, float p, uint64_t seed, uint64_t offset, int64_t mask_ld,
                                           gist_stream_t stream) {
    GIST_REQUIRE(p >= 0.f && p < 1.f, "gist_ln_affine_fwd_drop_f32: p must be in [0,1)");
    GIST_REQUIRE(mask_ld >= d || p == 0.f, "gist_ln_affine_fwd_drop_f32: mask_ld < d");
    gist::LnaDrop dr{};
    dr.out2 = out2; dr.ldo2 = ldo2;
    dr.m = gist::drop_mask_of(p, seed); dr.offset = offset; dr.mask_ld = mask_ld;
    return gist::ln_affine_fwd_ex("gist_ln_affine_fwd_drop_f32", x, ldx, lin_bias, gamma, beta, yhat, ldy, out, ldo,
                                  rstd, n_rows, d, relu, eps, &dr, false, gist::as_stream(stream));
}

extern "C" int gist_ln_affine_infer_f32(const float *x, int64_t ldx, const float *lin_bias, const float *gamma,
                                        const float *beta, float *out, int64_t ldo, int64_t n_rows, int64_t d, int relu,
                                        float eps, gist_stream_t stream) {
    return gist::ln_affine_fwd_ex("gist_ln_affine_infer_f32", x, ldx, lin_bias, gamma, beta, nullptr, 0, out, ldo, nullptr,
                                  n_rows, d, relu, eps, nullptr, true, gist::as_stream(stream));
}

extern "C" int64_t gist_ln_affine_bwd_workspace_floats(int64_t n_rows, int64_t d) {
    return n_rows <= 0 || d <= 0 ? 0 : 3 * gist_row_chunks16(n_rows) * d;
}

extern "C" int gist_ln_affine_bwd_f32(const float *d_out, int64_t ldg, const float *yhat, int64_t ldy,
                                      const float *rstd, const float *gamma, const float *beta, int relu, float *dx,
                                      int64_t lddx, float *dgamma, float *dbeta, float *dlin_bias, int64_t n_rows,
                                      int64_t d, float *workspace, int64_t workspace_floats, gist_stream_t stream) {
    using namespace gist;
    GIST_REQUIRE(n_rows >= 0 && d >= 0, "gist_ln_affine_bwd_f32: negative size");
    if (n_rows == 0 || d == 0) return GIST_OK;
    GIST_REQUIRE(d_out && yhat && rstd && gamma && beta && dx && dgamma && dbeta, "gist_ln_affine_bwd_f32: null pointer");
    GIST_REQUIRE(ldg >= d && ldy >= d && lddx >= d, "gist_ln_affine_bwd_f32: leading dimension < d");
    GIST_REQUIRE(n_rows < (1LL << 31) - kChunkRows && d < (1LL << 31), "gist_ln_affine_bwd_f32: size >= 2^31");
    GIST_REQUIRE(workspace && workspace_floats >= gist_ln_affine_bwd_workspace_floats(n_rows, d),
                 "gist_ln_affine_bwd_f32: workspace too small (gist_ln_affine_bwd_workspace_floats)");
    const bool v4 = d % 4 == 0 && ldg % 4 == 0 && ldy % 4 == 0 && lddx % 4 == 0 && aligned16(d_out) && aligned16(yhat) &&
                    aligned16(dx) && aligned16(gamma) && aligned16(beta) && aligned16(workspace);
    const int chunks = (int)gist_row_chunks16(n_rows);
    const int n_sums = dlin_bias != nullptr ? 3 : 2;
#define L(TPR, V)                                                                                                  \
    hipLaunchKernelGGL((ln_affine_bwd_kernel<TPR, V>), dim3((unsigned)chunks), dim3(256), 0, as_stream(stream), d_out, \
                       ldg, yhat, ldy, rstd, gamma, beta, dx, lddx, (int)n_rows, (int)d, relu, workspace, n_sums)
    if (d > 1024) { if (v4) L(256, 4); else L(256, 1); }
    else { if (v4) L(64, 4); else L(64, 1); }
#undef L
    const int rc = launch_status("gist_ln_affine_bwd_f32");
    if (rc != GIST_OK) return rc;
    LnAffineOuts outs{{dgamma, dbeta, dlin_bias}};
    hipLaunchKernelGGL(ln_affine_finish_kernel, dim3((unsigned)ceil_div(d, 64), (unsigned)n_sums), dim3(256), 0,
                       as_stream(stream), workspace, chunks, (int)d, outs);
    return launch_status("gist_ln_affine_bwd_f32 (finish)");
}
