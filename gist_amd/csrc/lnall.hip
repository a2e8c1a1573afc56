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
#include "lnall.h"

namespace gist {

// a tensor as it lies in memory
template <int VEC>
struct LnAllPlain {
    const float *x, *xb;      // element 0, unit 0
    __device__ __forceinline__ void unit(int64_t u, float (&v)[VEC]) const { vload<VEC>(xb, u, v); }
    __device__ __forceinline__ float edge(int64_t e) const { return x[e]; }
};
template <int VEC>
struct LnAllPlain2 {
    const float *g, *gb, *y, *yb;
    __device__ __forceinline__ void unit(int64_t u, float (&v)[VEC], float (&w)[VEC]) const {
        vload<VEC>(gb, u, v);
        vload<VEC>(yb, u, w);
    }
    __device__ __forceinline__ void edge(int64_t e, float &a, float &b) const { a = g[e]; b = y[e]; }
};

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void ln_all_fwd_stats_kernel(const float *x, LnAllGeom ge, double *partials) {
    __shared__ double red[4];
    LnAllPlain<VEC> ld{x, x + ge.head};
    ln_all_fwd_partials<VEC>(ge, ld, red, partials);
}

template <int VEC>
__global__ __launch_bounds__(256) void ln_all_fwd_norm_kernel(const float *x, float *yhat, LnAllGeom ge,
                                                              const double *__restrict__ partials, float eps,
                                                              float *__restrict__ stats) {
    __shared__ double red[4];
    float mf, rstd;
    ln_all_fwd_merge<VEC>(ge, red, partials, eps, mf, rstd);
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = mf; stats[1] = rstd; }
    const float *xb = x + ge.head;
    float *yb = yhat + ge.head;
    const int64_t u0 = (int64_t)blockIdx.x * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC];
        vload<VEC>(xb, u, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = ln_all_norm(v[k], mf, rstd);
        vstore<VEC>(yb, u, v);
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) yhat[e] = ln_all_norm(x[e], mf, rstd);
}

// ---------------------------------------------------------------------------
// backward: dx = rstd * (g - mean(g) - yhat * mean(g * yhat))
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void ln_all_bwd_stats_kernel(const float *__restrict__ g,
                                                               const float *__restrict__ yhat, LnAllGeom ge,
                                                               double *partials) {
    __shared__ double red[4];
    LnAllPlain2<VEC> ld{g, g + ge.head, yhat, yhat + ge.head};
    ln_all_bwd_partials<VEC>(ge, ld, red, partials);
}

template <int VEC>
__global__ __launch_bounds__(256) void ln_all_bwd_apply_kernel(const float *g, const float *__restrict__ yhat,
                                                               const float *__restrict__ stats, float *dx, LnAllGeom ge,
                                                               const double *__restrict__ partials) {
    __shared__ double red[4];
    float m1, m2;
    ln_all_bwd_merge<VEC>(ge, red, partials, m1, m2);
    const float rstd = stats[1];
    const float *gb = g + ge.head, *yb = yhat + ge.head;
    float *db = dx + ge.head;
    const int64_t u0 = (int64_t)blockIdx.x * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
#pragma unroll 4
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC], y[VEC];
        vload<VEC>(gb, u, v);
        vload<VEC>(yb, u, y);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = ln_all_dx(v[k], y[k], m1, m2, rstd);
        vstore<VEC>(db, u, v);
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) dx[e] = ln_all_dx(g[e], yhat[e], m1, m2, rstd);
}

}  // namespace gist

using namespace gist;

extern "C" int64_t gist_ln_all_partials(int64_t n) {
    return ln_all_partial_floats(n);
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
