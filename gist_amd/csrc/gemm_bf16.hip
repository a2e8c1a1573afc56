// bf16x1 (GEMM mode 3): ordinary mixed precision.  Every fp32 operand element is rounded ONCE to bf16 (to nearest, ties
// to even: v_cvt_pk_bf16_f32; a NaN stays a NaN, a finite value at or beyond bf16's range becomes +-Inf), the products
// are exact in fp32 and are summed in fp32 on v_mfma_f32_16x16x32_bf16; bias and output are fp32.  One MFMA term and
// 2 bytes per staged operand element where bf16x3 (gemm_b3.hip) has six terms and 6 bytes.
//
// Cast pre-pass (one launch for both operands): reads each fp32 source once and writes it as a k-contiguous bf16 image
// [rows][x1_kpad(k)] into the call's workspace, zeros past k, whatever the source layout: an operand whose k is the slow
// index ([k][rows]: the NN form's W, both TN operands) is transposed here through a 64 x 64 LDS tile, so there is ONE
// main kernel, NT.  16-byte aligned sources with ld % 4 == 0 are read as float4, the rest element by element.
//
// Main kernel: 128 x 128 x 64 block tile, 256 threads = 4 waves in 2 x 2, wave tile 64 x 64 = 4 x 4 MFMA tiles (64
// accumulator registers), two LDS stages of A 16 KiB + B 16 KiB (64 KiB: two workgroups per CU).  The images are padded
// to whole k tiles, so every k tile goes global -> LDS by DMA (the fp32 kernel's scheme, gemm.hip: the next tile's DMA is
// issued, the current tile's MFMAs run, vmcnt(0) and one barrier).  LDS image of an operand = [128 rows][8 chunks of
// 16 B = 8 k]; chunk c of row r sits in slot c ^ ((r >> 1) & 7): the 16 rows a fragment read touches land on 16 different
// 16-byte bank groups.  A lane's fragment of v_mfma_f32_16x16x32_bf16 (row lane & 15, k = 8 (lane >> 4) .. + 7) is one
// ds_read_b128.  k slices (blockIdx.z) write dense fp32 slabs that splitk_reduce sums in slice order (+ bias): no atomics,
// the result is a function of the arguments and the plan alone.
#include <type_traits>

#include "common.h"

namespace gist {

typedef __bf16 x1_bf16x8 __attribute__((ext_vector_type(8)));
typedef float x1_f32x4 __attribute__((ext_vector_type(4)));

constexpr int X1_THREADS = 256;
constexpr int X1_IMG_BYTES = X1_T * X1_BK * 2;             // one operand, one stage: 16 KiB
constexpr int X1_STAGE_BYTES = 2 * X1_IMG_BYTES;
constexpr int X1_LDS_BYTES = 2 * X1_STAGE_BYTES;
constexpr int X1_DMA = X1_IMG_BYTES / 1024 / 4;            // DMA instructions per wave and image: 4

// ---- cast pre-pass -----------------------------------------------------------------------------------
struct X1CastJob {
    const float *src; int64_t ld;     // kc: src[rows][k]; else src[k][rows]
    uint16_t *dst;                    // [rows][kpad] bf16
    int64_t rows, k, kpad;
    int kc, vec4;
    int gx;                           // transposing job: 64-wide k tiles per row of 64 x 64 tiles
    int64_t first;                    // its first block
};
struct X1CastList { X1CastJob job[2]; };

__device__ __forceinline__ uint32_t x1_pack(float lo, float hi) {
    return pack_bf16x2((__bf16)lo, (__bf16)hi);
}

__global__ __launch_bounds__(X1_THREADS) void x1_cast_kernel(X1CastList L) {
    __shared__ float tile[64][65];
    const int64_t bid = blockIdx.x;
    const X1CastJob J = bid >= L.job[1].first ? L.job[1] : L.job[0];      // (job 1 absent: first = total blocks)
    const int64_t lb = bid - J.first;
    const int t = threadIdx.x;
    if (J.kc) {
        // one 16-byte chunk (8 k of one row) per thread, chunks of a row on consecutive threads
        const int64_t cpr = J.kpad / 8, g = lb * X1_THREADS + t;
        if (g >= J.rows * cpr) return;
        const int64_t r = g / cpr, k0 = (g - r * cpr) * 8;
        const float *s = J.src + r * J.ld + k0;
        float v[8];
        if (J.vec4 && k0 + 8 <= J.k) {
            const float4 a = *reinterpret_cast<const float4 *>(s), b = *reinterpret_cast<const float4 *>(s + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = k0 + e < J.k ? s[e] : 0.f;
        }
        *reinterpret_cast<uint4 *>(J.dst + r * J.kpad + k0) =
            make_uint4(x1_pack(v[0], v[1]), x1_pack(v[2], v[3]), x1_pack(v[4], v[5]), x1_pack(v[6], v[7]));
        return;
    }
    // src[k][rows] -> dst[rows][kpad]: a 64 (k) x 64 (rows) tile through LDS
    const int64_t k0 = (lb % J.gx) * 64, r0 = (lb / J.gx) * 64;
    {
        const int cq = t & 15, kr = t >> 4;                // columns (rows of dst) 4 cq .. + 3, k rows kr + 16 i
        const int64_t c = r0 + 4 * cq;
        const bool whole = J.vec4 && r0 + 64 <= J.rows;    // (block-uniform: whole float4s only)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t kk = k0 + kr + 16 * i;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kk < J.k) load4_ragged(J.src + kk * J.ld + c, c, J.rows, whole, q);
            float *d = &tile[kr + 16 * i][4 * cq];
            d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int g = t + X1_THREADS * i, r = g & 63, ch = g >> 6;      // (consecutive lanes: consecutive LDS columns)
        if (r0 + r >= J.rows) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tile[8 * ch + e][r];
        *reinterpret_cast<uint4 *>(J.dst + (r0 + r) * J.kpad + k0 + 8 * ch) =
            make_uint4(x1_pack(v[0], v[1]), x1_pack(v[2], v[3]), x1_pack(v[4], v[5]), x1_pack(v[6], v[7]));
    }
}

// ---- the GEMM ----------------------------------------------------------------------------------------
struct X1Args {
    const uint16_t *a, *b;            // images [m][kpad], [n][kpad]
    const float *bias;
    float *c; int64_t ldc;
    int m, n, kpad;
    int tiles_m, tiles_n;
    int kt_per_split;                 // k tiles per blockIdx.z; slice s writes c + s * split_stride
    int64_t split_stride;
};

// DMA instruction j = 4 wave + jj of an image fills its LDS bytes [1024 j, 1024 (j + 1)): position p = 64 j + lane is row
// p / 8, slot p % 8, which holds k chunk slot ^ ((row >> 1) & 7).  Byte offsets relative to the tile origin: < 128 rows x
// pitch x 2 B < 2^31 for a pitch < 2^22 (the planner's limit).  Rows past the operand's last are clamped to it: what
// they hold only reaches output rows / columns that are never stored.
__device__ __forceinline__ void x1_dma_offsets(int64_t pitch, int rows, int row0, int wave, int lane, uint32_t (&off)[X1_DMA]) {
#pragma unroll
    for (int jj = 0; jj < X1_DMA; ++jj) {
        const int p = 64 * (X1_DMA * wave + jj) + lane;
        const int r = p >> 3, slot = p & 7;
        const int dr = min(r, rows - 1 - row0);
        off[jj] = (uint32_t)(((int64_t)dr * pitch + ((slot ^ ((r >> 1) & 7)) << 3)) * 2);
    }
}

__global__ __launch_bounds__(X1_THREADS, 2) void gemm_bf16x1_kernel(X1Args g) {
    extern __shared__ __attribute__((aligned(16))) char x1_smem[];
    const TileOf tile = tile_of_linear(xcd_linear((int)blockIdx.x, g.tiles_m * g.tiles_n), g.tiles_m, g.tiles_n);
    const int row0 = tile.bm * X1_T, col0 = tile.bn * X1_T;

    const int n_kt_all = g.kpad / X1_BK;
    const int kt_begin = (int)blockIdx.z * g.kt_per_split;
    const int n_kt = min(g.kt_per_split, n_kt_all - kt_begin);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int rr = lane & 15, kg = lane >> 4;

    x1_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = x1_f32x4{0.f, 0.f, 0.f, 0.f};

    uint32_t offA[X1_DMA], offB[X1_DMA];
    x1_dma_offsets(g.kpad, g.m, row0, wave, lane, offA);
    x1_dma_offsets(g.kpad, g.n, col0, wave, lane, offB);
    const uint16_t *originA = g.a + (int64_t)row0 * g.kpad + (int64_t)kt_begin * X1_BK;
    const uint16_t *originB = g.b + (int64_t)col0 * g.kpad + (int64_t)kt_begin * X1_BK;
    auto dma = [&](int buf, int kt) {
        char *sa = x1_smem + buf * X1_STAGE_BYTES;
        lds_dma_image<X1_DMA>(originA + (int64_t)kt * X1_BK, offA, sa, X1_DMA * wave);
        lds_dma_image<X1_DMA>(originB + (int64_t)kt * X1_BK, offB, sa + X1_IMG_BYTES, X1_DMA * wave);
    };
    // fragment byte offsets inside an image: tile i of the wave, k step s (32 k): row, chunk 4 s + kg
    int aoff[4][2], boff[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int ra = wm * 64 + i * 16 + rr, rb = wn * 64 + i * 16 + rr;
            aoff[i][s] = ra * (X1_BK * 2) + (((4 * s + kg) ^ ((ra >> 1) & 7)) << 4);
            boff[i][s] = rb * (X1_BK * 2) + (((4 * s + kg) ^ ((rb >> 1) & 7)) << 4);
        }

    if (n_kt > 0) dma(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0f70);         // vmcnt(0): the DMA has landed in LDS
    __syncthreads();

    auto kstep = [&](auto cur_c, int kt) {
        constexpr int cur = decltype(cur_c)::value;
        if (kt + 1 < n_kt) dma(cur ^ 1, kt + 1);      // buffer cur ^ 1 is free since the last barrier
        __builtin_amdgcn_sched_barrier(0);
        const char *sa = x1_smem + cur * X1_STAGE_BYTES;
        const char *sb = sa + X1_IMG_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            x1_bf16x8 af[4], bf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const x1_bf16x8 *>(sa + aoff[i][s]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const x1_bf16x8 *>(sb + boff[j][s]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0f70);     // vmcnt(0): the next tile has landed
        __syncthreads();
    };
    for (int kt = 0; kt < n_kt; kt += 2) {
        kstep(std::integral_constant<int, 0>{}, kt);
        if (kt + 1 < n_kt) kstep(std::integral_constant<int, 1>{}, kt + 1);
    }

    // ---- epilogue: C/D layout col = lane & 15, row = 4 (lane >> 4) + register.  Raw buffer stores whose resource covers
    // exactly the valid rows of this tile; columns >= n get an out-of-range offset and are dropped by the range check.
    const int rows_valid = min(g.m - row0, X1_T);
    float *cbase = g.c + (int64_t)blockIdx.z * g.split_stride + (int64_t)row0 * g.ldc + col0;
    __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(cbase, 0, (int)((int64_t)rows_valid * g.ldc * 4), 0x00020000);
    const uint32_t ldc_b = (uint32_t)g.ldc * 4;
    uint32_t cvoff[4];
    float bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cl = wn * 64 + j * 16 + rr;
        const bool ok = col0 + cl < g.n;
        cvoff[j] = ok ? (uint32_t)(wm * 64 + 4 * kg) * ldc_b + (uint32_t)cl * 4 : 0x7fffffffu;
        bv[j] = (g.bias != nullptr && ok) ? g.bias[col0 + cl] : 0.f;
    }
    // (the range check covers the vector offset only, so the row advance rides in it)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t roff = (uint32_t)(i * 16 + e) * ldc_b;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = acc[i][j][e] + bv[j];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), crsrc, cvoff[j] + roff, 0, 0);
            }
        }
}

// ---- host side: the plan (gemm_plan.h) says slices and where images and slabs sit -------------------------
static int x1_cast(const char *name, bool a_kc, const float *a, int64_t lda, int64_t m, uint16_t *ia, bool b_kc,
                   const float *b, int64_t ldb, int64_t n, uint16_t *ib, int64_t k, hipStream_t st) {
    X1CastList L{};
    int64_t blocks = 0;
    auto fill = [&](X1CastJob &J, bool kc, const float *src, int64_t ld, int64_t rows, uint16_t *dst) {
        J.src = src; J.ld = ld; J.dst = dst; J.rows = rows; J.k = k; J.kpad = x1_kpad(k);
        J.kc = kc; J.vec4 = aligned16(src) && ld % 4 == 0;
        J.gx = (int)(J.kpad / 64);
        J.first = blocks;
        blocks += kc ? ceil_div(rows * (J.kpad / 8), X1_THREADS) : (int64_t)J.gx * ceil_div(rows, 64);
    };
    fill(L.job[0], a_kc, a, lda, m, ia);
    fill(L.job[1], b_kc, b, ldb, n, ib);
    if (blocks >= (1LL << 31)) { set_error("%s: %lld blocks in the bf16 cast", name, (long long)blocks); return GIST_EINVAL; }
    hipLaunchKernelGGL(x1_cast_kernel, dim3((unsigned)blocks), dim3(X1_THREADS), 0, st, L);
    return launch_status(name);
}

// A gist_gemm_* call on this path.  A: a_kc ? [m][k] : [k][m];  B: b_kc ? [n][k] : [k][n].
int x1_gemm(const char *name, const GemmPlan &pl, bool a_kc, bool b_kc, const float *a, int64_t lda, const float *b,
            int64_t ldb, const float *bias, float *c, int64_t ldc, int64_t m, int64_t n, int64_t k, void *ws, hipStream_t st) {
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_bf16x1_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, X1_LDS_BYTES);
        if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e)); return GIST_ELAUNCH; }
        once.done(dev);
    }
    const int64_t kpad = x1_kpad(k);
    uint16_t *ia = reinterpret_cast<uint16_t *>(static_cast<char *>(ws) + pl.operand_offset);
    uint16_t *ib = ia + m * kpad;
    float *slabs = reinterpret_cast<float *>(static_cast<char *>(ws) + pl.scratch_offset);
    int rc = x1_cast(name, a_kc, a, lda, m, ia, b_kc, b, ldb, n, ib, k, st);
    if (rc != GIST_OK) return rc;
    X1Args g;
    g.a = ia; g.b = ib; g.bias = bias; g.c = c; g.ldc = ldc;
    g.m = (int)m; g.n = (int)n; g.kpad = (int)kpad;
    g.tiles_m = (int)ceil_div(m, X1_T); g.tiles_n = (int)ceil_div(n, X1_T);
    g.kt_per_split = (int)(pl.k_per_split / X1_BK);
    g.split_stride = 0;
    if (pl.splits > 1) { g.c = slabs; g.ldc = n; g.split_stride = m * n; g.bias = nullptr; }
    const int64_t slot = timer_begin(tl_timer, 2, m, n, k, st);      // kind 2: the main kernel (+ slab sum)
    hipLaunchKernelGGL(gemm_bf16x1_kernel, dim3((unsigned)(g.tiles_m * g.tiles_n), 1, (unsigned)pl.splits), dim3(X1_THREADS),
                       X1_LDS_BYTES, st, g);
    rc = launch_status(name);
    if (rc == GIST_OK && pl.splits > 1) rc = splitk_reduce(name, slabs, m * n, pl.splits, bias, c, ldc, m, n, st);
    timer_end(tl_timer, slot, st);
    return rc;
}

}  // namespace gist
