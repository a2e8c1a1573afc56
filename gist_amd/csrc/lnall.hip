// Whole-tensor LayerNorm over the grid: ONE mean and variance over all n elements of a tensor (gcn/gcn.py:65-66,
// F.layer_norm(h, h.shape)), spread over the chip instead of walked by the single workgroup that a [1, n] row gets
// from the row kernel (rowops.hip).
//
// Both directions are two launches with the same geometry, a function of n alone:
//   launch 1  every workgroup reduces its slice to two doubles            -> partials[2 * b], partials[2 * b + 1]
//   launch 2  every workgroup sums the whole partial array again, in the same fixed order, and rewrites its slice
// No float atomics, no hand-off between workgroups inside a launch: for a given n and base alignment the result is
// bitwise a function of the values.
//
// Geometry.  A unit is VEC floats (VEC = 4: one 16-byte load; the `head` floats in front of the first 16-byte
// boundary and the `tail` floats behind the last whole unit are scalars of workgroup 0).  VEC = 1 when the tensors of
// a call do not share their alignment.  grid = clamp(ceil(n / 4096), 1, 1024) workgroups of 256 threads; workgroup b
// owns units [b * uper, (b + 1) * uper), uper = ceil(units / grid), thread t every 256th of them: past the cap the
// slices grow and each workgroup loops further.
//
// Forward partials: the slice's (mean, M2), two passes over the slice (the second one hits the cache): m = the fp32
// slice mean as pivot, Q = sum (x - m)^2, C = sum (x - m); mean_b = m + C / cnt, M2_b = Q - C^2 / cnt.  Launch 2
// merges them as mean = sum cnt_b mean_b / n, M2 = sum (M2_b + cnt_b (mean_b - mean)^2): every term of the second sum is
// non-negative, nothing cancels.  The merges run in fp64 (at most 4 partials per thread and a 256-leaf tree).
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

template <int VEC>
__device__ __forceinline__ void ln_all_load(const float *p, int64_t u, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p + 4 * u);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = p[u];
    }
}

template <int VEC>
__device__ __forceinline__ void ln_all_store(float *p, int64_t u, const float (&v)[VEC]) {
    if constexpr (VEC == 4)
        *reinterpret_cast<float4 *>(p + 4 * u) = make_float4(v[0], v[1], v[2], v[3]);
    else
        p[u] = v[0];
}

template <int VEC>
__device__ __forceinline__ float ln_all_add(const float (&v)[VEC]) {
    if constexpr (VEC == 4) return (v[0] + v[1]) + (v[2] + v[3]);
    else return v[0];
}

// the double sums of the partial array every workgroup of a second launch forms, in one fixed order
template <int VEC, typename F>
__device__ __forceinline__ double ln_all_merge(const LnAllGeom &ge, double *red, F term) {
    double a = 0.0;
    for (int j = threadIdx.x; j < ge.grid; j += 256) a += term(j, (double)ln_all_count(ge, j, VEC));
    return block_sum_f64(a, red);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void ln_all_fwd_stats_kernel(const float *x, LnAllGeom ge, double *partials) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const float *xb = x + ge.head;
    const int64_t u0 = (int64_t)b * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
    const int64_t e = ln_all_edge(ge, VEC);
    const int64_t cnt = ln_all_count(ge, b, VEC);
    float s = 0.f;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC];
        ln_all_load<VEC>(xb, u, v);
        s += ln_all_add<VEC>(v);
    }
    if (e >= 0) s += x[e];
    const double S = block_sum_f64((double)s, red);
    const float m = cnt > 0 ? (float)(S / (double)cnt) : 0.f;
    float q = 0.f, c = 0.f;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC], w[VEC];
        ln_all_load<VEC>(xb, u, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { v[k] -= m; w[k] = v[k] * v[k]; }
        c += ln_all_add<VEC>(v);
        q += ln_all_add<VEC>(w);
    }
    if (e >= 0) { const float a = x[e] - m; c += a; q += a * a; }
    const double Q = block_sum_f64((double)q, red);
    const double C = block_sum_f64((double)c, red);
    if (threadIdx.x == 0) {
        const double m2 = cnt > 0 ? Q - C * C / (double)cnt : 0.0;
        partials[2 * b] = cnt > 0 ? (double)m + C / (double)cnt : 0.0;
        partials[2 * b + 1] = m2 > 0.0 ? m2 : 0.0;
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void ln_all_fwd_norm_kernel(const float *x, float *yhat, LnAllGeom ge,
                                                              const double *__restrict__ partials, float eps,
                                                              float *__restrict__ stats) {
    __shared__ double red[4];
    const double nn = (double)ge.n;
    const double mean = ln_all_merge<VEC>(ge, red, [&](int j, double cnt) { return cnt * partials[2 * j]; }) / nn;
    const double var = ln_all_merge<VEC>(ge, red, [&](int j, double cnt) {
        const double d = partials[2 * j] - mean;
        return partials[2 * j + 1] + cnt * d * d;
    }) / nn;
    const float mf = (float)mean;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = mf; stats[1] = rstd; }
    const float *xb = x + ge.head;
    float *yb = yhat + ge.head;
    const int64_t u0 = (int64_t)blockIdx.x * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC];
        ln_all_load<VEC>(xb, u, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = (v[k] - mf) * rstd;
        ln_all_store<VEC>(yb, u, v);
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) yhat[e] = (x[e] - mf) * rstd;
}

// ---------------------------------------------------------------------------
// backward: dx = rstd * (g - mean(g) - yhat * mean(g * yhat))
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void ln_all_bwd_stats_kernel(const float *__restrict__ g,
                                                               const float *__restrict__ yhat, LnAllGeom ge,
                                                               double *partials) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const float *gb = g + ge.head, *yb = yhat + ge.head;
    const int64_t u0 = (int64_t)b * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC], y[VEC];
        ln_all_load<VEC>(gb, u, v);
        ln_all_load<VEC>(yb, u, y);
        s1 += ln_all_add<VEC>(v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) y[k] *= v[k];
        s2 += ln_all_add<VEC>(y);
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) { s1 += g[e]; s2 += g[e] * yhat[e]; }
    const double S1 = block_sum_f64((double)s1, red);
    const double S2 = block_sum_f64((double)s2, red);
    if (threadIdx.x == 0) { partials[2 * b] = S1; partials[2 * b + 1] = S2; }
}

template <int VEC>
__global__ __launch_bounds__(256) void ln_all_bwd_apply_kernel(const float *g, const float *__restrict__ yhat,
                                                               const float *__restrict__ stats, float *dx, LnAllGeom ge,
                                                               const double *__restrict__ partials) {
    __shared__ double red[4];
    const double nn = (double)ge.n;
    const float m1 = (float)(ln_all_merge<VEC>(ge, red, [&](int j, double) { return partials[2 * j]; }) / nn);
    const float m2 = (float)(ln_all_merge<VEC>(ge, red, [&](int j, double) { return partials[2 * j + 1]; }) / nn);
    const float rstd = stats[1];
    const float *gb = g + ge.head, *yb = yhat + ge.head;
    float *db = dx + ge.head;
    const int64_t u0 = (int64_t)blockIdx.x * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC], y[VEC];
        ln_all_load<VEC>(gb, u, v);
        ln_all_load<VEC>(yb, u, y);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = rstd * (v[k] - m1 - y[k] * m2);
        ln_all_store<VEC>(db, u, v);
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) dx[e] = rstd * (g[e] - m1 - yhat[e] * m2);
}

static inline unsigned ln_all_phase(const void *p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u); }

}  // namespace gist

using namespace gist;

extern "C" int64_t gist_ln_all_partials(int64_t n) {
    if (n <= 0) return 0;
    const int64_t g = ceil_div(n, kLnAllChunk);
    return 4 * (g > kLnAllCap ? kLnAllCap : g);       // two doubles per workgroup, counted in floats
}

extern "C" int gist_ln_all_fwd_f32(const float *x, float *yhat, float *stats, int64_t n, float eps, float *partials,
                                   gist_stream_t stream) {
    GIST_REQUIRE(n >= 0, "gist_ln_all_fwd_f32: negative size");
    if (n == 0) return GIST_OK;
    GIST_REQUIRE(x && yhat && stats && partials, "gist_ln_all_fwd_f32: null pointer");
    GIST_REQUIRE(n < (1LL << 33), "gist_ln_all_fwd_f32: size >= 2^31 * 4");
    GIST_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(yhat)) & 3u) == 0 && aligned8(partials),
                 "gist_ln_all_fwd_f32: misaligned buffer");
    double *pp = reinterpret_cast<double *>(partials);
    hipStream_t st = as_stream(stream);
    if (ln_all_phase(x) == ln_all_phase(yhat)) {
        const LnAllGeom ge = ln_all_geom(n, 4, x);
        hipLaunchKernelGGL(ln_all_fwd_stats_kernel<4>, dim3(ge.grid), dim3(256), 0, st, x, ge, pp);
        hipLaunchKernelGGL(ln_all_fwd_norm_kernel<4>, dim3(ge.grid), dim3(256), 0, st, x, yhat, ge, pp, eps, stats);
    } else {
        const LnAllGeom ge = ln_all_geom(n, 1, x);
        hipLaunchKernelGGL(ln_all_fwd_stats_kernel<1>, dim3(ge.grid), dim3(256), 0, st, x, ge, pp);
        hipLaunchKernelGGL(ln_all_fwd_norm_kernel<1>, dim3(ge.grid), dim3(256), 0, st, x, yhat, ge, pp, eps, stats);
    }
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return launch_status("gist_ln_all_fwd_f32");
}

extern "C" int gist_ln_all_bwd_f32(const float *g, const float *yhat, const float *stats, float *dx, int64_t n,
                                   float *partials, gist_stream_t stream) {
    GIST_REQUIRE(n >= 0, "gist_ln_all_bwd_f32: negative size");
    if (n == 0) return GIST_OK;
    GIST_REQUIRE(g && yhat && stats && dx && partials, "gist_ln_all_bwd_f32: null pointer");
    GIST_REQUIRE(n < (1LL << 33), "gist_ln_all_bwd_f32: size >= 2^31 * 4");
    GIST_REQUIRE(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(yhat) | reinterpret_cast<uintptr_t>(dx)) & 3u) == 0 &&
                     aligned8(partials),
                 "gist_ln_all_bwd_f32: misaligned buffer");
    double *pp = reinterpret_cast<double *>(partials);
    hipStream_t st = as_stream(stream);
    if (ln_all_phase(g) == ln_all_phase(yhat) && ln_all_phase(g) == ln_all_phase(dx)) {
        const LnAllGeom ge = ln_all_geom(n, 4, g);
        hipLaunchKernelGGL(ln_all_bwd_stats_kernel<4>, dim3(ge.grid), dim3(256), 0, st, g, yhat, ge, pp);
        hipLaunchKernelGGL(ln_all_bwd_apply_kernel<4>, dim3(ge.grid), dim3(256), 0, st, g, yhat, stats, dx, ge, pp);
    } else {
        const LnAllGeom ge = ln_all_geom(n, 1, g);
        hipLaunchKernelGGL(ln_all_bwd_stats_kernel<1>, dim3(ge.grid), dim3(256), 0, st, g, yhat, ge, pp);
        hipLaunchKernelGGL(ln_all_bwd_apply_kernel<1>, dim3(ge.grid), dim3(256), 0, st, g, yhat, stats, dx, ge, pp);
    }
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return launch_status("gist_ln_all_bwd_f32");
}
