// The whole-tensor LayerNorm's geometry, slice partials and merges (lnall.hip's header comment describes the scheme), for
// the two files that run it: lnall.hip on a tensor as it lies in memory, gcntail.hip on relu(x + b) and on d_out under a
// dropout mask, formed while loading.  A kernel hands the slice loops a loader:
//   unit(u, v)        the VEC values of unit u (units of one thread are asked for in ascending order, 256 apart)
//   edge(e)           the value of scalar element e (head and tail of workgroup 0)
// and the backward's loader unit(u, g, y) / edge(e, g, y) both operands.  The arithmetic on the loaded values is stated
// here once, so two kernels whose loaders return the same floats leave the same bits.
#pragma once
#include "common.h"

namespace gist {

constexpr int kLnAllChunk = 4096;      // floats per workgroup below the cap
constexpr int kLnAllCap = 1024;        // workgroups at most

struct LnAllGeom {
    int64_t n, head, units, uper, tail;
    int grid;
};

static LnAllGeom ln_all_geom(int64_t n, int vec, const void *base) {
    LnAllGeom ge;
    ge.n = n;
    const int64_t g = ceil_div(n, kLnAllChunk);
    ge.grid = (int)(g < 1 ? 1 : (g > kLnAllCap ? kLnAllCap : g));
    if (vec == 4) {
        const int64_t off = (int64_t)((reinterpret_cast<uintptr_t>(base) >> 2) & 3u);
        const int64_t head = (4 - off) & 3;
        ge.head = head < n ? head : n;
    } else {
        ge.head = 0;
    }
    ge.units = (n - ge.head) / vec;
    ge.tail = n - ge.head - ge.units * vec;
    ge.uper = ceil_div(ge.units, ge.grid);
    return ge;
}

static inline unsigned ln_all_phase(const void *p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u); }

// two doubles per workgroup, counted in floats (gist_ln_all_partials)
static inline int64_t ln_all_partial_floats(int64_t n) {
    if (n <= 0) return 0;
    const int64_t g = ceil_div(n, kLnAllChunk);
    return 4 * (g > kLnAllCap ? kLnAllCap : g);
}

#ifdef __HIPCC__
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);      // a + b == b + a: the same bits in every lane
    return v;
}

__device__ __forceinline__ double block_sum_f64(double v, double *red) {
    v = wave_sum_f64(v);
    __syncthreads();                       // red[] may still be read from a previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// elements of workgroup b's slice: its units, and for workgroup 0 the scalar head and tail
__device__ __forceinline__ int64_t ln_all_count(const LnAllGeom &ge, int b, int vec) {
    int64_t u0 = (int64_t)b * ge.uper, u1 = u0 + ge.uper;
    if (u0 > ge.units) u0 = ge.units;
    if (u1 > ge.units) u1 = ge.units;
    return (u1 - u0) * vec + (b == 0 ? ge.head + ge.tail : 0);
}

// index of the scalar element thread t of workgroup 0 owns, or -1
__device__ __forceinline__ int64_t ln_all_edge(const LnAllGeom &ge, int vec) {
    if (blockIdx.x != 0) return -1;
    const int64_t t = threadIdx.x;
    if (t < ge.head) return t;
    if (t < ge.head + ge.tail) return ge.head + ge.units * vec + (t - ge.head);
    return -1;
}

// the double sums of the partial array every workgroup of a second launch forms, in one fixed order
template <int VEC, typename F>
__device__ __forceinline__ double ln_all_merge(const LnAllGeom &ge, double *red, F term) {
    double a = 0.0;
    for (int j = threadIdx.x; j < ge.grid; j += 256) a += term(j, (double)ln_all_count(ge, j, VEC));
    return block_sum_f64(a, red);
}

// a product that stays a product: a loader that forms d_out * factor hands the sums below the rounded value a stored
// tensor would hold, never one operand of a fused multiply-add
__device__ __forceinline__ float ln_all_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// the two elementwise formulas
__device__ __forceinline__ float ln_all_norm(float v, float mean, float rstd) { return (v - mean) * rstd; }
__device__ __forceinline__ float ln_all_dx(float g, float y, float m1, float m2, float rstd) {
    return rstd * (g - m1 - y * m2);
}

// forward, launch 1: workgroup blockIdx.x's (mean, M2) -> partials[2 b], partials[2 b + 1]
template <int VEC, typename L>
__device__ __forceinline__ void ln_all_fwd_partials(const LnAllGeom &ge, L &ld, double *red, double *partials) {
    const int b = blockIdx.x;
    const int64_t u0 = (int64_t)b * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
    const int64_t e = ln_all_edge(ge, VEC);
    const int64_t cnt = ln_all_count(ge, b, VEC);
    float s = 0.f;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC];
        ld.unit(u, v);
        s += vsum<VEC>(v);
    }
    if (e >= 0) s += ld.edge(e);
    const double S = block_sum_f64((double)s, red);
    const float m = cnt > 0 ? (float)(S / (double)cnt) : 0.f;
    float q = 0.f, c = 0.f;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC], w[VEC];
        ld.unit(u, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { v[k] -= m; w[k] = v[k] * v[k]; }
        c += vsum<VEC>(v);
        q += vsum<VEC>(w);
    }
    if (e >= 0) { const float a = ld.edge(e) - m; c += a; q += a * a; }
    const double Q = block_sum_f64((double)q, red);
    const double C = block_sum_f64((double)c, red);
    if (threadIdx.x == 0) {
        const double m2 = cnt > 0 ? Q - C * C / (double)cnt : 0.0;
        partials[2 * b] = cnt > 0 ? (double)m + C / (double)cnt : 0.0;
        partials[2 * b + 1] = m2 > 0.0 ? m2 : 0.0;
    }
}

// forward, launch 2: every workgroup's merge of the partial array
template <int VEC>
__device__ __forceinline__ void ln_all_fwd_merge(const LnAllGeom &ge, double *red, const double *__restrict__ partials,
                                                 float eps, float &mf, float &rstd) {
    const double nn = (double)ge.n;
    const double mean = ln_all_merge<VEC>(ge, red, [&](int j, double cnt) { return cnt * partials[2 * j]; }) / nn;
    const double var = ln_all_merge<VEC>(ge, red, [&](int j, double cnt) {
        const double d = partials[2 * j] - mean;
        return partials[2 * j + 1] + cnt * d * d;
    }) / nn;
    mf = (float)mean;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// backward, launch 1: workgroup blockIdx.x's sum g and sum g * yhat
template <int VEC, typename L>
__device__ __forceinline__ void ln_all_bwd_partials(const LnAllGeom &ge, L &ld, double *red, double *partials) {
    const int b = blockIdx.x;
    const int64_t u0 = (int64_t)b * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC], y[VEC];
        ld.unit(u, v, y);
        s1 += vsum<VEC>(v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) y[k] *= v[k];
        s2 += vsum<VEC>(y);
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) {
        float g, y;
        ld.edge(e, g, y);
        s1 += g; s2 += g * y;
    }
    const double S1 = block_sum_f64((double)s1, red);
    const double S2 = block_sum_f64((double)s2, red);
    if (threadIdx.x == 0) { partials[2 * b] = S1; partials[2 * b + 1] = S2; }
}

// backward, launch 2: mean(g) and mean(g * yhat) from the partial array, the same bits in every workgroup of any grid
template <int VEC>
__device__ __forceinline__ void ln_all_bwd_merge(const LnAllGeom &ge, double *red, const double *__restrict__ partials,
                                                 float &m1, float &m2) {
    const double nn = (double)ge.n;
    m1 = (float)(ln_all_merge<VEC>(ge, red, [&](int j, double) { return partials[2 * j]; }) / nn);
    m2 = (float)(ln_all_merge<VEC>(ge, red, [&](int j, double) { return partials[2 * j + 1]; }) / nn);
}
#endif

}  // namespace gist
