// The tail of a BaselineGCN layer on gfx950 (cluster_gcn/modules.py:316-349): GraphConv's bias and activation (:346), the
// whole-tensor F.layer_norm(h, h.shape) (:347-348) and the NEXT layer's dropout (:345) on a dense [n_rows, d] tensor,
//   a = relu ? max(x + b, 0) : x + b;   yhat = norm ? (a - mean) * rstd : a;   out = yhat * factor
// with ONE mean and biased variance over all n_rows * d values of a, and factor = gist_dropout_f32's at element index
// offset + r * d + c.
//
// The statistics are lnall.hip's scheme (lnall.h): the same geometry over the flat tensor, the same pivoted (mean, M2)
// slice partials in double, the same fixed-order merge in every workgroup of the second launch; a is formed on load and
// never stored.  No float atomics.
//   forward   norm: slice partials of a; merge + yhat + out.  no norm: the second launch alone.
//   infer     the same two kernels with out alone (out may be x: a thread rewrites the elements it has just read).
//   backward  norm: slice sums of g = d_out * factor and g * yhat (lnall's geometry); then, a workgroup per 16 rows x
//             64 * VEC columns, dx = gate ? da : 0 and the chunk's column sums of dx; then colsum_finish adds the chunks in
//             gist_colsum_chunks_f32's order.  no norm: the last two launches alone.
//
//   scales    GraphConv's two degree vectors 1 / sqrt(max(degree, 1)) from rowptr and t_rowptr, one launch (at the end).
//
// Columns.  A 16-byte unit of the flat walk lies inside a row only when d % 4 == 0 and the tensor starts on a 16-byte
// boundary; otherwise it straddles rows.  The bias column of flat element i is i % d either way: a thread computes the
// column of its first unit with one 64-bit remainder and steps it by (256 * VEC) % d from unit to unit.
#include "lnall.h"

namespace gist {
namespace {

constexpr int kChunkRows = 16;      // gist_row_chunks16

// relu?(x + b) of the flat tensor, as lnall.h's loader.  BV: a unit's four bias values are one aligned float4.
template <int VEC, bool BV>
struct TailLoad {
    const float *x, *xb;            // element 0, unit 0
    const float *__restrict__ b;
    int64_t head;
    int d, step, relu;              // step = (256 * VEC) % d
    int64_t next_u = -1;
    unsigned c = 0;                 // column of the first element of unit next_u (c + step < 2^32)

    // the backward's gate, applied: a closed gate stores +0 whatever the sign of a zero sum
    __device__ __forceinline__ float act(float v) const { return (!relu || v > 0.f) ? v : 0.f; }
    __device__ __forceinline__ int column(int64_t u) {
        if (u != next_u) c = (unsigned)((uint64_t)(head + u * VEC) % (uint64_t)d);
        const int c0 = (int)c;
        next_u = u + 256;
        c += (unsigned)step;
        if (c >= (unsigned)d) c -= (unsigned)d;
        return c0;
    }
    __device__ __forceinline__ void bias(int c0, float (&bb)[VEC]) const {
        if constexpr (BV) {
            const float4 q = *reinterpret_cast<const float4 *>(b + c0);
            bb[0] = q.x; bb[1] = q.y; bb[2] = q.z; bb[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                int ck = c0 + k;
                if (ck >= d) ck -= d;
                if (ck >= d) ck %= d;      // d < 4
                bb[k] = b[ck];
            }
        }
    }
    // the unit's values of a, and its column
    __device__ __forceinline__ void unit(int64_t u, float (&v)[VEC]) {
        float bb[VEC];
        bias(column(u), bb);
        vload<VEC>(xb, u, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = act(v[k] + bb[k]);
    }
    __device__ __forceinline__ float edge(int64_t e) const { return act(x[e] + b[(int)((uint64_t)e % (uint64_t)d)]); }
};

// d_out under the forward's mask, and yhat, of the flat tensor
template <int VEC>
struct TailLoadG {
    const float *g, *gb, *y, *yb;
    int64_t head;
    DropMask m;
    uint64_t offset;
    __device__ __forceinline__ void unit(int64_t u, float (&v)[VEC], float (&w)[VEC]) const {
        vload<VEC>(gb, u, v);
        vload<VEC>(yb, u, w);
        if (m.p > 0.f) {
            const uint64_t i0 = offset + (uint64_t)(head + u * VEC);
            if constexpr (VEC == 4) {
                float f[4];
                drop_factors4(f, i0, m);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = ln_all_mul(v[k], f[k]);
            } else {
                v[0] = ln_all_mul(v[0], drop_keep(i0, m));
            }
        }
    }
    __device__ __forceinline__ void edge(int64_t e, float &a, float &b) const {
        a = m.p > 0.f ? ln_all_mul(g[e], drop_keep(offset + (uint64_t)e, m)) : g[e];
        b = y[e];
    }
};

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int VEC, bool BV>
__global__ __launch_bounds__(256) void gcn_tail_stats_kernel(const float *x, const float *__restrict__ b, LnAllGeom ge,
                                                             int d, int step, int relu, double *partials) {
    __shared__ double red[4];
    TailLoad<VEC, BV> ld{x, x + ge.head, b, ge.head, d, step, relu};
    ln_all_fwd_partials<VEC>(ge, ld, red, partials);
}

// yhat (NULL: not stored) and out (NULL: not stored; under the mask when m.p > 0); x may be out
template <int VEC, bool BV>
__global__ __launch_bounds__(256) void gcn_tail_write_kernel(const float *x, const float *__restrict__ b, float *yhat,
                                                             float *out, LnAllGeom ge, int d, int step, int relu, int norm,
                                                             const double *__restrict__ partials, float eps, float *stats,
                                                             DropMask m, uint64_t offset) {
    __shared__ double red[4];
    float mf = 0.f, rstd = 1.f;
    if (norm) {
        ln_all_fwd_merge<VEC>(ge, red, partials, eps, mf, rstd);
        if (stats != nullptr && blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = mf; stats[1] = rstd; }
    }
    TailLoad<VEC, BV> ld{x, x + ge.head, b, ge.head, d, step, relu};
    const int64_t u0 = (int64_t)blockIdx.x * ge.uper;
    const int64_t u1 = u0 + ge.uper < ge.units ? u0 + ge.uper : ge.units;
#pragma unroll 2
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        float v[VEC];
        ld.unit(u, v);
        if (norm) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = ln_all_norm(v[k], mf, rstd);
        }
        if (yhat != nullptr) vstore<VEC>(yhat + ge.head, u, v);
        if (out != nullptr) {
            if (m.p > 0.f) drop_vec<VEC>(v, offset + (uint64_t)(ge.head + u * VEC), m);
            vstore<VEC>(out + ge.head, u, v);
        }
    }
    const int64_t e = ln_all_edge(ge, VEC);
    if (e >= 0) {
        float v = ld.edge(e);
        if (norm) v = ln_all_norm(v, mf, rstd);
        if (yhat != nullptr) yhat[e] = v;
        if (out != nullptr) out[e] = m.p > 0.f ? v * drop_keep(offset + (uint64_t)e, m) : v;
    }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void gcn_tail_bwd_stats_kernel(const float *__restrict__ d_out,
                                                                 const float *__restrict__ yhat, LnAllGeom ge, DropMask m,
                                                                 uint64_t offset, double *partials) {
    __shared__ double red[4];
    TailLoadG<VEC> ld{d_out, d_out + ge.head, yhat, yhat + ge.head, ge.head, m, offset};
    ln_all_bwd_partials<VEC>(ge, ld, red, partials);
}

// blockIdx.x = 16-row chunk, blockIdx.y = tile of 64 * VEC columns; wave w owns rows r0 + w + 4 j (j ascending), a lane
// VEC columns.  col_sums[chunk][c] = ((w0 + w1) + w2) + w3 of the waves' sums of dx.  `ge` is the geometry the partial
// array was written with (VECP its unit), not this kernel's.
template <int VEC, int VECP>
__global__ __launch_bounds__(256) void gcn_tail_bwd_apply_kernel(
    const float *__restrict__ d_out, const float *__restrict__ x, const float *__restrict__ b,
    const float *__restrict__ yhat, const float *__restrict__ stats, float *__restrict__ dx, int n_rows, int d, int relu,
    int norm, DropMask m, uint64_t offset, LnAllGeom ge, const double *__restrict__ partials,
    float *__restrict__ col_sums) {
    __shared__ double red[4];
    __shared__ float part[3][64 * VEC];
    float m1 = 0.f, m2 = 0.f, rstd = 1.f;
    if (norm) {
        ln_all_bwd_merge<VECP>(ge, red, partials, m1, m2);
        rstd = stats[1];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (blockIdx.y * 64 + lane) * VEC;
    const int r0 = blockIdx.x * kChunkRows;
    const bool live = c < d;
    float bb[VEC], cs[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) cs[k] = 0.f;
    if (live) vload<VEC>(b + c, bb);
    if (live) {
#pragma unroll
        for (int j = 0; j < kChunkRows / 4; ++j) {
            const int row = r0 + wave + 4 * j;
            if (row >= n_rows) break;
            const int64_t i0 = (int64_t)row * d + c;
            float g[VEC], xv[VEC], y[VEC] = {};
            vload<VEC>(d_out + i0, g);
            vload<VEC>(x + i0, xv);
            if (norm) vload<VEC>(yhat + i0, y);
            if (m.p > 0.f) {
                if constexpr (VEC == 4) {
                    float f[4];
                    drop_factors4(f, offset + (uint64_t)i0, m);
#pragma unroll
                    for (int k = 0; k < 4; ++k) g[k] = ln_all_mul(g[k], f[k]);
                } else {
                    g[0] = ln_all_mul(g[0], drop_keep(offset + (uint64_t)i0, m));
                }
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float da = norm ? ln_all_dx(g[k], y[k], m1, m2, rstd) : g[k];
                g[k] = (!relu || xv[k] + bb[k] > 0.f) ? da : 0.f;      // the forward's own add; no gradient at 0
                cs[k] += g[k];
            }
            vstore<VEC>(dx + i0, g);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) part[wave - 1][lane * VEC + k] = cs[k];
    }
    __syncthreads();
    if (wave == 0 && live) {
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            o[k] = ((cs[k] + part[0][lane * VEC + k]) + part[1][lane * VEC + k]) + part[2][lane * VEC + k];
        vstore<VEC>(col_sums + (int64_t)blockIdx.x * d + c, o);
    }
}

int tail_common(const char *name, const float *x, const float *b, int64_t n_rows, int64_t d, int relu, int norm,
                float eps) {
    GIST_REQUIRE(x && b, "%s: null pointer", name);
    GIST_REQUIRE(n_rows < (1LL << 31) - kChunkRows && d < (1LL << 31), "%s: size >= 2^31", name);
    GIST_REQUIRE(n_rows * d < (1LL << 33), "%s: size >= 2^31 * 4", name);
    GIST_REQUIRE(!norm || eps >= 0.f, "%s: negative eps", name);
    GIST_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(b)) & 3u) == 0, "%s: misaligned buffer", name);
    return GIST_OK;
}

// the forward's launches; yhat and out may each be NULL, out may be yhat's or x's address
int tail_fwd_launch(const char *name, const float *x, const float *b, float *yhat, float *out, float *stats, int64_t n_rows,
                    int64_t d, int relu, int norm, float eps, const DropMask &m, uint64_t offset, float *ws,
                    hipStream_t st) {
    const int64_t n = n_rows * d;
    GIST_REQUIRE(((reinterpret_cast<uintptr_t>(yhat) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0 && (!norm || aligned8(ws)),
                 "%s: misaligned buffer", name);
    const bool v4 = (yhat == nullptr || ln_all_phase(yhat) == ln_all_phase(x)) &&
                    (out == nullptr || ln_all_phase(out) == ln_all_phase(x));
    const LnAllGeom ge = ln_all_geom(n, v4 ? 4 : 1, x);
    const bool bv = v4 && d % 4 == 0 && ge.head == 0 && aligned16(b);
    const int step = (int)((v4 ? 1024 : 256) % d);
    double *pp = reinterpret_cast<double *>(ws);
    if (out == yhat) out = nullptr;      // p = 0 (checked by the caller): one store serves both
#define L(V, BV)                                                                                                        \
    do {                                                                                                                \
        if (norm) {                                                                                                     \
            hipLaunchKernelGGL((gcn_tail_stats_kernel<V, BV>), dim3(ge.grid), dim3(256), 0, st, x, b, ge, (int)d, step, \
                               relu, pp);                                                                               \
            g_launches.fetch_add(1, std::memory_order_relaxed);                                                         \
        }                                                                                                               \
        hipLaunchKernelGGL((gcn_tail_write_kernel<V, BV>), dim3(ge.grid), dim3(256), 0, st, x, b, yhat, out, ge, (int)d, \
                           step, relu, norm, pp, eps, stats, m, offset);                                                \
    } while (0)
    if (bv) L(4, true);
    else if (v4) L(4, false);
    else L(1, false);
#undef L
    return launch_status(name);
}

// ---------------------------------------------------------------------------
// the degree scales of GraphConv.forward (dgl_compat/nn/pytorch.py:27-30), both vectors in one launch
// ---------------------------------------------------------------------------
// 1 / sqrt(max(deg, 1)).  The build has no fast-math flag, so hipcc's default for HIP holds (correctly rounded fp32
// divide and square root: the v_sqrt_f32 / v_rcp_f32 results with their fix-up sequences, never v_rsq_f32); the
// __fsqrt_rn / __fdiv_rn spellings would NOT be stronger -- without OCML_BASIC_ROUNDED_OPERATIONS the first is the
// native square root.  The pragma keeps the two operations apart whatever flags a later build adds.
__device__ __forceinline__ float degree_scale(const int32_t *__restrict__ rowptr, int64_t v) {
#pragma clang fp reassociate(off) contract(off) reciprocal(off)
    const int deg = rowptr[v + 1] - rowptr[v];
    const float f = (float)(deg > 1 ? deg : 1);
    return 1.0f / __builtin_sqrtf(f);
}

__global__ __launch_bounds__(256) void gcn_degree_scales_kernel(const int32_t *__restrict__ rowptr,
                                                                const int32_t *__restrict__ t_rowptr, int64_t n_rows,
                                                                float *__restrict__ nd, float *__restrict__ ns) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    nd[v] = degree_scale(rowptr, v);
    ns[v] = degree_scale(t_rowptr, v);
}

}  // namespace
}  // namespace gist

using namespace gist;

extern "C" int gist_gcn_degree_scales_f32(const int32_t *rowptr, const int32_t *t_rowptr, int64_t n_rows, float *nd,
                                          float *ns, gist_stream_t stream) {
    const char *name = "gist_gcn_degree_scales_f32";
    GIST_REQUIRE(n_rows >= 0 && n_rows < (1LL << 31), "%s: n_rows must be in 0 .. 2^31 - 1", name);
    if (n_rows == 0) return GIST_OK;
    GIST_REQUIRE(rowptr && t_rowptr && nd && ns, "%s: null pointer", name);
    GIST_REQUIRE(((reinterpret_cast<uintptr_t>(rowptr) | reinterpret_cast<uintptr_t>(t_rowptr) |
                   reinterpret_cast<uintptr_t>(nd) | reinterpret_cast<uintptr_t>(ns)) & 3u) == 0,
                 "%s: misaligned buffer", name);
    hipLaunchKernelGGL(gcn_degree_scales_kernel, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, as_stream(stream),
                       rowptr, t_rowptr, n_rows, nd, ns);
    return launch_status(name);
}

extern "C" int gist_gcn_tail_fwd_f32(const float *x, const float *b, float *yhat, float *out, float *stats, int64_t n_rows,
                                     int64_t d, int relu, int norm, float eps, float p, uint64_t seed, uint64_t offset,
                                     float *ws, gist_stream_t stream) {
    const char *name = "gist_gcn_tail_fwd_f32";
    GIST_REQUIRE(n_rows >= 0 && d >= 0, "%s: negative size", name);
    GIST_REQUIRE(p >= 0.f && p < 1.f, "%s: p must be in [0,1)", name);
    if (n_rows == 0 || d == 0) return GIST_OK;
    GIST_REQUIRE((yhat || out) && (out || p == 0.f) && (!norm || (stats && ws)), "%s: null pointer", name);
    GIST_REQUIRE(out != yhat || p == 0.f, "%s: out must not be yhat when p > 0", name);
    GIST_REQUIRE(x != yhat && x != out, "%s: x must not be overwritten", name);
    const int rc = tail_common(name, x, b, n_rows, d, relu, norm, eps);
    if (rc != GIST_OK) return rc;
    return tail_fwd_launch(name, x, b, yhat, out, stats, n_rows, d, relu, norm, eps, drop_mask_of(p, seed), offset, ws,
                           as_stream(stream));
}

extern "C" int gist_gcn_tail_infer_f32(const float *x, const float *b, float *out, float *stats, int64_t n_rows, int64_t d,
                                       int relu, int norm, float eps, float *ws, gist_stream_t stream) {
    const char *name = "gist_gcn_tail_infer_f32";
    GIST_REQUIRE(n_rows >= 0 && d >= 0, "%s: negative size", name);
    if (n_rows == 0 || d == 0) return GIST_OK;
    GIST_REQUIRE(out && (!norm || ws), "%s: null pointer", name);
    const int rc = tail_common(name, x, b, n_rows, d, relu, norm, eps);
    if (rc != GIST_OK) return rc;
    return tail_fwd_launch(name, x, b, nullptr, out, stats, n_rows, d, relu, norm, eps, drop_mask_of(0.f, 0), 0, ws,
                           as_stream(stream));
}

extern "C" int64_t gist_gcn_tail_bwd_workspace_floats(int64_t n_rows, int64_t d) {
    return n_rows <= 0 || d <= 0 ? 0 : ln_all_partial_floats(n_rows * d) + gist_row_chunks16(n_rows) * d;
}

extern "C" int gist_gcn_tail_bwd_f32(const float *d_out, const float *x, const float *b, const float *yhat,
                                     const float *stats, float *dx, float *dbias, int64_t n_rows, int64_t d, int relu,
                                     int norm, float p, uint64_t seed, uint64_t offset, float *ws, int64_t ws_floats,
                                     gist_stream_t stream) {
    const char *name = "gist_gcn_tail_bwd_f32";
    GIST_REQUIRE(n_rows >= 0 && d >= 0, "%s: negative size", name);
    GIST_REQUIRE(p >= 0.f && p < 1.f, "%s: p must be in [0,1)", name);
    if (n_rows == 0 || d == 0) return GIST_OK;
    GIST_REQUIRE(d_out && dx && dbias && (!norm || (yhat && stats)), "%s: null pointer", name);
    const int rc = tail_common(name, x, b, n_rows, d, relu, 0, 0.f);
    if (rc != GIST_OK) return rc;
    GIST_REQUIRE(ws && ws_floats >= gist_gcn_tail_bwd_workspace_floats(n_rows, d),
                 "%s: workspace too small (gist_gcn_tail_bwd_workspace_floats)", name);
    GIST_REQUIRE(((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(yhat) | reinterpret_cast<uintptr_t>(dx) |
                   reinterpret_cast<uintptr_t>(dbias)) & 3u) == 0 && aligned8(ws),
                 "%s: misaligned buffer", name);
    const int64_t n = n_rows * d;
    const DropMask m = drop_mask_of(p, seed);
    double *pp = reinterpret_cast<double *>(ws);
    float *col_sums = ws + ln_all_partial_floats(n);
    hipStream_t st = as_stream(stream);
    const int vecp = (norm && ln_all_phase(d_out) == ln_all_phase(yhat)) ? 4 : 1;
    const LnAllGeom ge = ln_all_geom(n, vecp, d_out);
    if (norm) {
        if (vecp == 4) hipLaunchKernelGGL(gcn_tail_bwd_stats_kernel<4>, dim3(ge.grid), dim3(256), 0, st, d_out, yhat, ge, m, offset, pp);
        else hipLaunchKernelGGL(gcn_tail_bwd_stats_kernel<1>, dim3(ge.grid), dim3(256), 0, st, d_out, yhat, ge, m, offset, pp);
        const int rc1 = launch_status(name);
        if (rc1 != GIST_OK) return rc1;
    }
    const bool v4 = d % 4 == 0 && aligned16(d_out) && aligned16(x) && aligned16(b) && aligned16(dx) && aligned16(col_sums) &&
                    (!norm || aligned16(yhat));
    const int chunks = (int)gist_row_chunks16(n_rows);
    const int64_t tiles = ceil_div(d, v4 ? 256 : 64);
    GIST_REQUIRE(tiles <= 65535, "%s: d too large for rows that are not whole aligned float4s", name);
#define L(V, VP)                                                                                                       \
    hipLaunchKernelGGL((gcn_tail_bwd_apply_kernel<V, VP>), dim3((unsigned)chunks, (unsigned)tiles), dim3(256), 0, st, d_out, \
                       x, b, yhat, stats, dx, (int)n_rows, (int)d, relu, norm, m, offset, ge, pp, col_sums)
    if (v4) { if (vecp == 4) L(4, 4); else L(4, 1); }
    else { if (vecp == 4) L(1, 4); else L(1, 1); }
#undef L
    const int rc2 = launch_status(name);
    if (rc2 != GIST_OK) return rc2;
    return colsum_finish(col_sums, chunks, d, dbias, st);
}
