// fp32 GEMM on the bf16 matrix cores with ALL 24 operand bits: every fp32 operand x is split once
// into three bf16 pieces, x = b1 + b2 + b3 exactly (b1 = bf16(x), b2 = bf16(x - b1),
// b3 = bf16(x - b1 - b2): 3 x 8 significant bits, round-to-nearest at every step, bf16 has fp32's
// exponent range so there is no scale and no row maximum), and
//     (A.B^T)[i][j] = sum_k ( a1.b3 + a3.b1 + a2.b2 + a1.b2 + a2.b1 + a1.b1 )      (fp32 accumulation)
// on v_mfma_f32_16x16x32_bf16: the six cross terms down to 2^-16 of a product.  What is dropped
// (a2.b3, a3.b2, a3.b3) is below 2^-23 of |a||b| per product, the size of ONE fp32 rounding of that
// product; every bf16 x bf16 product is exact in fp32, and a k tile of 32 products is rounded into the
// accumulator 6 times instead of 16 times on v_mfma_f32_32x32x2_f32.  Measured against float64 the
// result is at the fp32-MFMA kernel's error level on every tested operand class, adversarial ones
// included (rms within 1.25x, max over 10^6 outputs within 3x: a few ulp of sum |a||b| either way;
// tests/test_gemm_b3_gpu.py).  Six bf16 MFMAs (16 cycles each) replace sixteen
// fp32-rate MFMA slots: 2.7x less matrix-core time per tile than the fp32 kernel.
//
// Pre-pass (HBM-bound, per operand): one kernel reads the fp32 source once and writes the operand
// k-contiguous whatever its source layout (the transposed form of NN/TN operands is produced here,
// so there is ONE GEMM kernel, NT), rows padded with zeros to a multiple of 64 k (an even number of k tiles), in the layout
//     row r : [k0..7 b1 (16 B)] [k0..7 b2] [k0..7 b3] [k8..15 b1] ...       (6 bytes per element)
// A lane's MFMA fragment (8 consecutive k of one row, one piece) is one 16-byte chunk.
//
// Main kernel: 256 x 128 x 32 block tile (A 48 KiB + B 24 KiB per stage, two stages = 144 KiB, one
// 512-thread workgroup per CU), 8 waves in 4 x 2, wave tile 64 x 64 = 4 x 4 MFMA tiles x 6 terms =
// 96 MFMAs per k tile, LDS-DMA staging issued a full k step ahead (below: one barrier per step, in
// its middle).  The tile is this large because at 6 bytes
// per element the L2 -> LDS traffic bounds smaller ones: 128 x 64 tiles with two workgroups per CU
// (9.4 GB staged for 2046 x 4096 x 8192) ran at 31 % matrix-pipe occupancy, this one (4.7 GB) at
// 45 %; a one-stage 128 x 128 variant with two workgroups per CU (fragment reads of one under the
// MFMAs of the other) was slower than either two-stage kernel (1.05 vs 0.95 ms per call).
// LDS image = [16-row slab][row][chunk] x 16 B, row-major like the operand: slot L of a slab
// (L = 12 row + position) holds chunk position ^ (2 if row >= 8), and a slab is three 1 KiB DMA
// instructions of 64 consecutive slots.  The four lanes of a DMA quad therefore read ONE aligned
// 64-byte piece of one row: the texture addresser handles a quad per cycle when it lies in one
// cache line, and the earlier image ([chunk][row]: a quad = 16 bytes from each of four rows, four
// lines) made the staging address-bound -- 1.08 -> 0.77 ms per 2046 x 4096 x 8192 call for the
// change of image alone.  The pair swap of rows 8-15 keeps the fragment reads conflict free: a
// ds_read_b128 lane group is rows {0-3, 12-15} of k group g with rows 4-11 of k group g + 1, i.e.
// chunks c and c + 3, and 16 B slot index mod 16 = (12 row + (c ^ swap)) mod 16 takes 16 different
// values over such a group (exhaustive check over the 3 pieces x 2 group kinds; no rotation by whole
// 64-byte pieces can do it, the slot index mod 4 would repeat).
// Outputs with at least 256 tiles of 256 x 256 that run as one k slice take a 256 x 256 x 32 sibling
// (gemm_b3_wide_kernel, below): same image, a third less staged traffic per flop, fewer rounds;
// bit for bit the same C.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "common.h"

namespace gist {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float b3_f32x4 __attribute__((ext_vector_type(4)));

// (the tile B3_TM x B3_TN = 256 x 128 and k per tile B3_BK = 32: gemm_plan.h)
constexpr int B3_THREADS = 512;
constexpr int B3_STAGES = 2;
constexpr int B3_SKEW = 16;      // MFMAs by which waves 4-7 run behind waves 0-3 inside a k step
constexpr int B3_KT_BYTES = B3_BK * 6;                 // 192 B of one row per k tile (12 chunks)
constexpr int B3_A_BYTES = B3_TM * B3_KT_BYTES;        // 24 KiB
constexpr int B3_B_BYTES = B3_TN * B3_KT_BYTES;        // 12 KiB
constexpr int B3_BUF_BYTES = B3_A_BYTES + B3_B_BYTES;

// ---- pre-pass ---------------------------------------------------------------------------------
// One read of src[rows, cols] -> the split operand with k = columns (dst_r: [rows][kpad(cols)]) and/or
// the one with k = rows (dst_t: [cols][kpad(rows)]), one 64 x 64 tile of src per 128-thread block; pitches
// in k elements (6 bytes each).  Dropout is applied on the fly with gist_dropout_f32's generator (element
// index offset + r * cols + c), so the fp32 dropped tensor never has to exist.
//
// A thread loads 8 rows x 4 columns (float4 per row: a wave instruction reads four whole 256-byte row
// segments) and splits each element ONCE.  In registers those pieces already form 12 transposed chunks
// (one column, 8 rows, one piece) and 24 half chunks of the row layout (one row, 4 columns, one piece).
// Each layout goes through an LDS image [output row][24 chunks + 1 pad] of 16 B, from which the block
// writes its 64 output rows x 384 B: consecutive lanes store consecutive 16-byte chunks, so a lane quad is
// one aligned 64-byte piece and a wave instruction covers whole row segments (the previous kernel split
// every element twice and stored 48 bytes per lane at a 48-byte lane stride: 24 partial lines per
// instruction).  One 25.6 KiB image is reused by the two layouts: six blocks per CU.
constexpr int B3S_THREADS = 128;
constexpr int B3S_PITCH = 25;                          // 16-B chunks per image row (24 + 1: fewer bank conflicts)

struct B3SplitJob {
    B3Dual d;
    int64_t ldd_r, ldd_t;
    DropMask mask;                    // drop_mask_of(d.p, d.seed): what the kernel reads; d.p and d.seed it does not
    int gx, gy;                       // 64 x 64 tiles of this job
    int first;                        // its first block
};
struct B3SplitList {
    B3SplitJob job[B3_SPLIT_MAX_JOBS];
    int n;
};

// x -> RNE bf16(x), bf16(x - b1), bf16(x - b1 - b2) (both differences exact)
__device__ __forceinline__ void b3_pieces(float x, __bf16 (&p)[3]) {
    p[0] = (__bf16)x;
    const float r1 = x - (float)p[0];
    p[1] = (__bf16)r1;
    const float r2 = r1 - (float)p[1];
    p[2] = (__bf16)r2;
}

// the image's 64 rows x 384 B -> dst rows out0 .. out0 + n_out - 1 at k offset k0; nt: non-temporal stores (the
// transposed layout: read by a backward projection after hundreds of MB of other traffic, while the row layout of W
// and Z is read by the forward projection right away -- nt on both cost that projection more than it saved here)
template <bool NT>
__device__ __forceinline__ void b3_store_image(const uint4 *img, uint16_t *__restrict__ dst, int64_t ldd,
                                               int64_t out0, int64_t n_out, int64_t k0, int t) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int s = 0; s < 64 * 24 / B3S_THREADS; ++s) {
        const int g = s * B3S_THREADS + t;
        const int o = g / 24, w = g - o * 24;
        if (o >= n_out) continue;
        const uint4 v = img[o * B3S_PITCH + w];
        u32x4 *p = reinterpret_cast<u32x4 *>(dst + ((out0 + o) * ldd + k0) * 3 + w * 8);
        const u32x4 vv = {v.x, v.y, v.z, v.w};
        if (NT) __builtin_nontemporal_store(vv, p);
        else *p = vv;
    }
}

__global__ __launch_bounds__(B3S_THREADS) void b3_split_kernel(B3SplitList L) {
    __shared__ uint4 img[64 * B3S_PITCH];                  // (also the fp32 tile of the column sums)
    static_assert(64 * B3S_PITCH * 16 >= 64 * 65 * 4, "image too small for the column-sum tile");
    const int bid = blockIdx.x;
    B3SplitJob J = L.job[0];                               // (copies: fields in SGPRs, not loads by index)
#pragma unroll
    for (int q = 1; q < B3_SPLIT_MAX_JOBS; ++q)
        if (q < L.n && bid >= L.job[q].first) J = L.job[q];
    const B3Dual &d = J.d;
    const int lb = bid - J.first;
    const int c0 = (lb % J.gx) * 64, r0 = (lb / J.gx) * 64;      // (row tiles outer: measured against both other orders)
    const int t = threadIdx.x;
    const int cq = t & 15, rg = t >> 4;                    // columns 4 cq .. 4 cq + 3, rows 8 rg .. 8 rg + 7
    const int c = c0 + 4 * cq;

    float v[8][4];
    if (d.vec4 && c0 + 64 <= d.cols) {                     // (block-uniform: whole float4s only)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t r = r0 + 8 * rg + i;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < d.rows) q = *reinterpret_cast<const float4 *>(d.src + r * d.ld + c);
            v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t r = r0 + 8 * rg + i;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[i][e] = r < d.rows && c + e < d.cols ? d.src[r * d.ld + c + e] : 0.f;
        }
    }
    if (J.mask.p > 0.f) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t r = r0 + 8 * rg + i;
            if (r >= d.rows) continue;
            float f[4];
            drop_factors4_flat(f, d.offset + (uint64_t)r * (uint64_t)d.cols + (uint64_t)c, J.mask);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] *= f[e];
        }
    }
    if (d.col_partials != nullptr) {      // column sums of this 64-row chunk, in the order gist_colsum_f32 uses
        float(*tile)[65] = reinterpret_cast<float(*)[65]>(img);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[8 * rg + i][4 * cq + e] = v[i][e];
        __syncthreads();
        if (t < 64 && c0 + t < d.cols && r0 < d.rows) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int r = 0; r < 64; r += 4) {
                s0 += tile[r][t]; s1 += tile[r + 1][t]; s2 += tile[r + 2][t]; s3 += tile[r + 3][t];
            }
            d.col_partials[(int64_t)(r0 / 64) * d.cols + c0 + t] = (s0 + s1) + (s2 + s3);
        }
        __syncthreads();
    }

    // the pieces, once per element
    uint32_t tw[4][3][4];                                  // transposed: column e, piece q, rows (2m, 2m + 1)
    uint2 rw[8][3];                                        // rows: row i, piece q, columns (0, 1), (2, 3)
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            __bf16 a[3], b[3];
            b3_pieces(v[i][e], a);
            b3_pieces(v[i + 1][e], b);
#pragma unroll
            for (int q = 0; q < 3; ++q) tw[e][q][i >> 1] = pack_bf16x2(a[q], b[q]);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint32_t w0 = tw[0][q][i >> 1], w1 = tw[1][q][i >> 1], w2 = tw[2][q][i >> 1], w3 = tw[3][q][i >> 1];
            rw[i][q] = (i & 1) ? make_uint2((w0 >> 16) | (w1 & 0xFFFF0000u), (w2 >> 16) | (w3 & 0xFFFF0000u))
                               : make_uint2((w0 & 0xFFFFu) | (w1 << 16), (w2 & 0xFFFFu) | (w3 << 16));
        }

    const bool rows_on = d.dst_r != nullptr && r0 < d.rows && c0 < J.ldd_r;
    const bool trans_on = d.dst_t != nullptr && c0 < d.cols && r0 < J.ldd_t;
    if (rows_on) {
        char *base = reinterpret_cast<char *>(img);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                *reinterpret_cast<uint2 *>(base + (8 * rg + i) * (B3S_PITCH * 16) + (cq >> 1) * 48 + q * 16 +
                                           (cq & 1) * 8) = rw[i][q];
        __syncthreads();
        b3_store_image<false>(img, d.dst_r, J.ldd_r, r0, d.rows - r0, c0, t);
    }
    if (trans_on) {
        if (rows_on) __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                img[(4 * cq + e) * B3S_PITCH + rg * 3 + q] = make_uint4(tw[e][q][0], tw[e][q][1], tw[e][q][2], tw[e][q][3]);
        __syncthreads();
        b3_store_image<true>(img, d.dst_t, J.ldd_t, c0, d.cols - c0, r0, t);
    }
}

// ---- the GEMM -----------------------------------------------------------------------------------
struct B3Args {
    const uint16_t *a; int64_t lda;      // split operands, [rows][kpad] elements of 6 bytes
    const uint16_t *b; int64_t ldb;
    const float *bias;
    float *c; int64_t ldc;
    int m, n, kpad;
    int tiles_m, tiles_n;
    int kt_per_split;                    // k tiles per blockIdx.y (even); split s writes c + s * split_stride
    int64_t split_stride;
    // Tail units (one k slice, tiles > one per CU): the first dp_tiles logical tiles run whole, one workgroup
    // each; every remaining tile is cut into tail_splits k slices of tail_kt k tiles (even), one workgroup
    // each (blockIdx.x = dp_tiles + tile * tail_splits + slice), which leave their accumulators at
    // tail_partials[unit][16 registers][512 threads] x 16 B; gemm_b3_tail_sum_kernel, the next launch,
    // sums a tile's partials in slice order and stores C (+ bias).
    int dp_tiles, tail_splits, tail_kt;
    float *tail_partials;
};

// DMA instruction `inst` of an image: slot L = 64 (inst % 3) + lane of 16-row slab inst / 3; slot
// L holds row L / 12, chunk (L % 12) ^ (2 if row >= 8): the four lanes of a quad read one aligned
// 64-byte piece of one row
template <int NI>
__device__ __forceinline__ void b3_dma_offsets(int64_t ld, int rows, int row0, int first, int lane,
                                                uint32_t (&off)[NI]) {
#pragma unroll
    for (int jj = 0; jj < NI; ++jj) {
        const int inst = first + jj;
        const int slot = (inst % 3) * 64 + lane;
        const int rs = slot / 12;
        const int chunk = (slot % 12) ^ ((rs >> 3) << 1);
        const int r = (inst / 3) * 16 + rs;
        const int dr = min(r, rows - 1 - row0);
        off[jj] = (uint32_t)((int64_t)dr * ld * 6 + chunk * 16);
    }
}

// acc += a . b in place.  (Written as asm with a tied accumulator: left to itself the register
// allocator gives many of the 96 MFMAs of a k step a destination different from their addend,
// rotates the 64 accumulator registers through a pool it does not have, and spills accumulators to
// scratch inside the k loop -- 113 VGPRs with the fragments live across the loop edge.)
__device__ __forceinline__ void b3_mfma(b3_f32x4 &acc, const bf16x8 &a, const bf16x8 &b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

__global__ __launch_bounds__(B3_THREADS, 2) void gemm_b3_kernel(B3Args g) {
    extern __shared__ __attribute__((aligned(16))) char b3_smem[];
    constexpr int NI = 4, NJ = 4;                 // 16-row slabs per wave: 64 x 64 wave tile
    const int nwg = g.dp_tiles;
    const int orig = blockIdx.x;
    const bool tail = orig >= nwg;       // a k slice of one of the tiles past the last full round
    const int tail_tile = tail ? (orig - nwg) / g.tail_splits : 0;
    const int tail_slice = tail ? (orig - nwg) % g.tail_splits : 0;
    const TileOf tile = tile_of_linear(tail ? nwg + tail_tile : xcd_linear(orig, nwg), g.tiles_m, g.tiles_n);
    const int row0 = tile.bm * B3_TM, col0 = tile.bn * B3_TN;
    // split-K: this workgroup's k tiles
    const int kt0 = tail ? tail_slice * g.tail_kt : (int)blockIdx.y * g.kt_per_split;
    const int n_kt = min(g.kpad / B3_BK - kt0, tail ? g.tail_kt : g.kt_per_split);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int rr = lane & 15, kg = lane >> 4;

    b3_f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

    // DMA instructions of 1 KiB: 3 per 16 rows of an image, dealt evenly to the waves
    constexpr int NWAVES = B3_THREADS / 64;
    constexpr int DA = B3_TM / 16 * 3 / NWAVES, DB = B3_TN / 16 * 3 / NWAVES;
    uint32_t offA[DA], offB[DB];
    b3_dma_offsets<DA>(g.lda, g.m, row0, DA * wave, lane, offA);
    b3_dma_offsets<DB>(g.ldb, g.n, col0, DB * wave, lane, offB);
    const char *originA = reinterpret_cast<const char *>(g.a) + (int64_t)row0 * g.lda * 6 + (int64_t)kt0 * B3_KT_BYTES;
    const char *originB = reinterpret_cast<const char *>(g.b) + (int64_t)col0 * g.ldb * 6 + (int64_t)kt0 * B3_KT_BYTES;
    auto dma = [&](int buf, int kt) {
        char *sa = b3_smem + buf * B3_BUF_BYTES;
        lds_dma_image<DA>(originA + (int64_t)kt * B3_KT_BYTES, offA, sa, DA * wave);
        lds_dma_image<DB>(originB + (int64_t)kt * B3_KT_BYTES, offB, sa + B3_A_BYTES, DB * wave);
    };

    // fragment addresses: chunk c = 3 kg + piece of row rr of slab s sits at slot
    // 192 s + 12 rr + (c ^ (2 if rr >= 8)) of its image.  One lane-dependent LDS address per (stage,
    // image, piece) = 12 VGPRs; the slab (3 KiB apart) goes into the ds_read offset field.
    const char *fa[B3_STAGES][3], *fb[B3_STAGES][3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int c = 3 * kg + p;
        const int in_slab = (rr * 12 + (c ^ ((rr >> 3) << 1))) * 16;
#pragma unroll
        for (int st = 0; st < B3_STAGES; ++st) {
            fa[st][p] = b3_smem + st * B3_BUF_BYTES + wm * NI * 3072 + in_slab;
            fb[st][p] = b3_smem + st * B3_BUF_BYTES + B3_A_BYTES + wn * NJ * 3072 + in_slab;
        }
    }

    // One barrier per k step, in the MIDDLE of the step.  Terms in the order
    //   a2.b1  a3.b1 | a2.b2  a1.b1 | a1.b2  a1.b3        (16 MFMAs each; pieces 1-based as above)
    // so that after the first four (64 MFMAs) the registers of a2, a3 and b1 are dead, and by then
    // every fragment read of the current image has been consumed.  At that point: wait for the own
    // pieces of the next tile's DMA (issued a whole step earlier), barrier -- next image complete AND
    // current image free --, issue the DMA of the tile after next into the current image, read the
    // a2 / a3 / b1 fragments of the next tile, and only then issue the last 32 MFMAs, which need
    // none of these.  The matrix pipe never waits on a post-barrier LDS round trip (with the barrier
    // at the end of the step all eight waves start the next one with 8 KiB of fragment reads each and
    // nothing to issue), and the DMA has a full step to land instead of 80 MFMA slots.
    // In-kernel stamps (2046 x 4096 x 8192 / 4096 x 8192 x 2046): MFMA
    // cycles are 0.79 / 0.84 of the k loop's cycles at 1.95 / 1.93 GHz, against 0.71 / 0.80 at
    // 2.08 / 1.96 GHz with the barrier at the end of the step -- the chip gives back in clock most of
    // what the pipe share gains (power), the loop itself is 2-4 % shorter (508 vs 531 us)
    // (probe removed; `git show 4165530:scripts/b3_clock_probe.py`).
    // A wave whose 64 rows all lie past the end of C (the last row tile of a batch a few rows over a multiple of 256)
    // stages its share of the images and meets the barriers, nothing else: its SIMD's other wave has the pipe alone.
    const bool live = __builtin_amdgcn_readfirstlane(row0 + wm * (16 * NI) < g.m);
    bf16x8 a[NI][3], b[NJ][3];
    auto read_head = [&](auto st_c) {
        constexpr int st = decltype(st_c)::value;
        if (!live) return;
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j][0] = *reinterpret_cast<const bf16x8 *>(fb[st][0] + j * 3072);
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i][1] = *reinterpret_cast<const bf16x8 *>(fa[st][1] + i * 3072);
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i][2] = *reinterpret_cast<const bf16x8 *>(fa[st][2] + i * 3072);
    };
    auto read_rest = [&](auto st_c) {
        constexpr int st = decltype(st_c)::value;
        if (!live) return;
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j][1] = *reinterpret_cast<const bf16x8 *>(fb[st][1] + j * 3072);
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i][0] = *reinterpret_cast<const bf16x8 *>(fa[st][0] + i * 3072);
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j][2] = *reinterpret_cast<const bf16x8 *>(fb[st][2] + j * 3072);
    };
    constexpr int pa[6] = {1, 2, 1, 0, 0, 0};
    constexpr int pb[6] = {0, 0, 1, 0, 1, 2};
    constexpr int B3_MID = 4 * NI * NJ;           // MFMAs before the barrier

    dma(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0f70);
    __syncthreads();
    dma(1, 1);                                       // n_kt is even and >= 2
    read_head(std::integral_constant<int, 0>{});

    // The two waves of a SIMD (w and w + 4) run the step half a term apart, so that one of them has
    // MFMAs to issue while the other issues its fragment reads and DMA instructions: waves 4-7
    // (`late`) issue 16 MFMAs before each of the two non-MFMA blocks of the step.
    auto mfmas = [&](auto t0_c, auto t1_c) {
        constexpr int t0 = decltype(t0_c)::value, t1 = decltype(t1_c)::value;
        if (!live) return;
#pragma unroll
        for (int t = t0; t < t1; ++t) {
            const int term = t / (NI * NJ), i = (t % (NI * NJ)) / NJ, j = t % NJ;
            b3_mfma(acc[i][j], a[i][pa[term]], b[j][pb[term]]);
        }
    };
    // Every step is the same straight-line code: k is padded to an EVEN number of tiles (zeros), the
    // DMA of a tile past the end re-reads the last one into an image nobody consumes, and the last
    // step's barrier and fragment prefetch are simply wasted.  (Variants per remaining-tile count
    // made the compiler merge accumulator registers across branches with hundreds of v_mov.)
    const int last_kt = n_kt - 1;
    auto kstep = [&](auto cur_c, auto late_c, int kt) {
        constexpr int cur = decltype(cur_c)::value;
        constexpr int skew = decltype(late_c)::value * B3_SKEW;
        using I = std::integral_constant<int, 0>;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        mfmas(I{}, std::integral_constant<int, skew>{});
        __builtin_amdgcn_sched_barrier(0);
        read_rest(cur_c);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(std::integral_constant<int, skew>{}, std::integral_constant<int, B3_MID>{});
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0070);          // vmcnt(0) lgkmcnt(0)
        __syncthreads();
        mfmas(std::integral_constant<int, B3_MID>{}, std::integral_constant<int, B3_MID + skew>{});
        __builtin_amdgcn_sched_barrier(0);
        dma(cur, min(kt + 2, last_kt));
        read_head(std::integral_constant<int, cur ^ 1>{});
        __builtin_amdgcn_sched_barrier(0);
        mfmas(std::integral_constant<int, B3_MID + skew>{}, std::integral_constant<int, 6 * NI * NJ>{});
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto run = [&](auto late_c) {
        using C0 = std::integral_constant<int, 0>;
        using C1 = std::integral_constant<int, 1>;
        for (int kt = 0; kt < n_kt; kt += 2) {
            kstep(C0{}, late_c, kt);
            kstep(C1{}, late_c, kt + 1);
        }
    };
    if (wave >= 4) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
    __builtin_amdgcn_s_waitcnt(0x0070);              // the wasted DMA and reads of the last step

    // the MFMAs above are opaque to the compiler's hazard recognizer: let the last ones retire
    // before the accumulators are read (4 passes + write-back)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    const int rows_valid = min(g.m - row0, B3_TM);
    if (tail) {
        // A wave whose 64 rows lie past the end of C has nothing to exchange (the usual tail tile is the
        // few rows a batch has beyond a multiple of 256).
        const bool rows_live = wm * (16 * NI) < rows_valid;
        b3_f32x4 *mine = reinterpret_cast<b3_f32x4 *>(g.tail_partials) +
                         (int64_t)(tail_tile * g.tail_splits + tail_slice) * (NI * NJ * B3_THREADS) + threadIdx.x;
        if (rows_live) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) mine[(i * NJ + j) * B3_THREADS] = acc[i][j];
        }
        return;                                      // gemm_b3_tail_sum_kernel, the next launch, finishes these tiles
    }
    // ---- epilogue: C/D of 16x16x32: col = lane & 15, row = 4 (lane >> 4) + e ----
    float *cbase = g.c + (int64_t)blockIdx.y * g.split_stride + (int64_t)row0 * g.ldc + col0;
    __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(
        cbase, 0, (int)((int64_t)rows_valid * g.ldc * 4), 0x00020000);
    const uint32_t ldc_b = (uint32_t)g.ldc * 4;
    uint32_t cvoff[NJ];
    float bv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cl = wn * (16 * NJ) + j * 16 + rr;
        const bool ok = col0 + cl < g.n;
        cvoff[j] = ok ? (uint32_t)(wm * (16 * NI) + 4 * kg) * ldc_b + (uint32_t)cl * 4 : 0x7fffffffu;
        bv[j] = (g.bias != nullptr && ok) ? g.bias[col0 + cl] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t roff = (uint32_t)(i * 16 + e) * ldc_b;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float v = acc[i][j][e] + bv[j];
                if (rows_valid == B3_TM)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), crsrc, cvoff[j], roff, 0);
                else
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), crsrc, cvoff[j] + roff, 0, 0);
            }
        }
}

// ---- the 256 x 256 x 32 tile ----------------------------------------------------------------------
// For outputs of at least 256 such tiles that run as one k slice (the backward projections of a
// 4096-wide hidden layer).  Same split operands, same DMA image, same 8 waves in 4 x 2 and the same
// one workgroup per CU; the wave tile is 64 x 128 (4 x 8 MFMA tiles, 128 accumulator registers), so
// a full fragment set (48 + 96 registers) no longer fits next to the accumulators.  The wave keeps
// its A fragments (a1, a2, a3 of 4 slabs) and streams B two 16-column slabs at a time: per slab pair,
// the six terms in the narrow kernel's order, 8 MFMAs each (an accumulator every 8th MFMA), and each
// B piece is re-read for the next pair right after the term that last uses it (b1 after a1.b1, b2
// after a1.b2, b3 after a1.b3).  Every fragment is read once per k tile: 36 ds_read_b128 per 192
// MFMAs instead of 24 per 96.  Every accumulator still sees k tiles in ascending order and the six
// terms in the same order, so C is bit for bit the narrow kernel's.
// LDS: two B images do fit with ONE A image (48 + 2 x 48 = 144 KiB), and A is read early: all of
// A_t is in registers once the k step's third term has been issued.  Two barriers per k step:
//   P (after the first slab pair's third term): A_t and B_{t-1} are free -> DMA A_{t+1}, B_{t+1}
//   Q (after the last slab pair's third term):  A_{t+1}, B_{t+1} complete -> read a2, a3 of A_{t+1}
//     (dead after a2.b2), then the first slab pair of B_{t+1} piece by piece, then a1 of A_{t+1}
// The DMA has the 144 MFMAs between P and Q to land.
// (B3W_TN = 256: gemm_plan.h)
constexpr int B3W_B_BYTES = B3W_TN * B3_KT_BYTES;                // 48 KiB
constexpr int B3W_LDS_BYTES = B3_A_BYTES + 2 * B3W_B_BYTES;      // 144 KiB

__global__ __launch_bounds__(B3_THREADS, 1) void gemm_b3_wide_kernel(B3Args g) {
    extern __shared__ __attribute__((aligned(16))) char b3_smem[];
    constexpr int NI = 4, NJ = 8;                 // 16-row slabs per wave: 64 x 128 wave tile
    const int nwg = g.dp_tiles;
    const int orig = blockIdx.x;
    const TileOf tile = tile_of_linear(xcd_linear(orig, nwg), g.tiles_m, g.tiles_n);
    const int row0 = tile.bm * B3_TM, col0 = tile.bn * B3W_TN;
    const int n_kt = g.kpad / B3_BK;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int rr = lane & 15, kg = lane >> 4;

    b3_f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

    constexpr int NWAVES = B3_THREADS / 64;
    constexpr int DA = B3_TM / 16 * 3 / NWAVES, DB = B3W_TN / 16 * 3 / NWAVES;
    uint32_t offA[DA], offB[DB];
    b3_dma_offsets<DA>(g.lda, g.m, row0, DA * wave, lane, offA);
    b3_dma_offsets<DB>(g.ldb, g.n, col0, DB * wave, lane, offB);
    const char *originA = reinterpret_cast<const char *>(g.a) + (int64_t)row0 * g.lda * 6;
    const char *originB = reinterpret_cast<const char *>(g.b) + (int64_t)col0 * g.ldb * 6;
    auto dma = [&](int bbuf, int kt) {
        lds_dma_image<DA>(originA + (int64_t)kt * B3_KT_BYTES, offA, b3_smem, DA * wave);
        lds_dma_image<DB>(originB + (int64_t)kt * B3_KT_BYTES, offB, b3_smem + B3_A_BYTES + bbuf * B3W_B_BYTES,
                         DB * wave);
    };

    // fragment addresses as in gemm_b3_kernel: one per (image, piece), the slab in the offset field
    const char *fa[3], *fb[2][3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int c = 3 * kg + p;
        const int in_slab = (rr * 12 + (c ^ ((rr >> 3) << 1))) * 16;
        fa[p] = b3_smem + wm * NI * 3072 + in_slab;
#pragma unroll
        for (int st = 0; st < 2; ++st) fb[st][p] = b3_smem + B3_A_BYTES + st * B3W_B_BYTES + wn * NJ * 3072 + in_slab;
    }

    // A wave whose 64 rows all lie past the end of C stages its share of the images and meets the
    // barriers, nothing else.  The loop is compiled once per kind of wave: with a run-time test around
    // each block the compiler's wait counts at the top of the k step turn conservative (lgkmcnt(0)
    // on the a1 reads just issued).
    auto body = [&](auto live_c) {
        constexpr bool live = decltype(live_c)::value;
        bf16x8 a[NI][3], b[2][3];                     // b: piece p of the two slabs of the current pair
        auto read_a = [&](auto p_c) {
            constexpr int p = decltype(p_c)::value;
            if constexpr (!live) return;
#pragma unroll
            for (int i = 0; i < NI; ++i) a[i][p] = *reinterpret_cast<const bf16x8 *>(fa[p] + i * 3072);
        };
        auto read_b = [&](auto st_c, auto pair_c, auto p_c) {
            constexpr int st = decltype(st_c)::value, pair = decltype(pair_c)::value, p = decltype(p_c)::value;
            if constexpr (!live) return;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) b[jj][p] = *reinterpret_cast<const bf16x8 *>(fb[st][p] + (2 * pair + jj) * 3072);
        };
        constexpr int pa[6] = {1, 2, 1, 0, 0, 0};
        constexpr int pb[6] = {0, 0, 1, 0, 1, 2};
        auto mfmas = [&](auto pair_c, auto t0_c, auto t1_c) {
            constexpr int pair = decltype(pair_c)::value, t0 = decltype(t0_c)::value, t1 = decltype(t1_c)::value;
            if constexpr (!live) return;
#pragma unroll
            for (int term = t0; term < t1; ++term)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int i = 0; i < NI; ++i) b3_mfma(acc[i][2 * pair + jj], a[i][pa[term]], b[jj][pb[term]]);
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;

        dma(0, 0);
        __builtin_amdgcn_s_waitcnt(0x0f70);
        __syncthreads();
        read_a(I1{}); read_a(I2{});                  // in the order the end of a k step issues them
        read_b(I0{}, I0{}, I0{}); read_b(I0{}, I0{}, I1{}); read_b(I0{}, I0{}, I2{});
        read_a(I0{});
        __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0) (see the lgkmcnt(2) in the k step)

        // As in gemm_b3_kernel every step is the same straight-line code (k padded to an even number of
        // tiles; the last step's DMA re-reads the last tile, its reads after Q are wasted).
        const int last_kt = n_kt - 1;
        auto kstep = [&](auto cur_c, int kt) {
            constexpr int cur = decltype(cur_c)::value;
            auto pair_block = [&](auto pair_c) {
                constexpr int pair = decltype(pair_c)::value;
                // where the next pieces come from: the next slab pair of this image, or pair 0 of the next
                using S = std::integral_constant<int, pair < 3 ? cur : (cur ^ 1)>;
                using P = std::integral_constant<int, pair < 3 ? pair + 1 : 0>;
                __builtin_amdgcn_sched_barrier(0);
                mfmas(pair_c, I0{}, I3{});               // a2.b1  a3.b1  a2.b2
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (pair == 0) {
                    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's reads of A_t are in
                    __syncthreads();
                    dma(cur ^ 1, min(kt + 1, last_kt));
                }
                if constexpr (pair == 3) {
                    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
                    __syncthreads();
                    read_a(I1{}); read_a(I2{});
                }
                __builtin_amdgcn_sched_barrier(0);
                mfmas(pair_c, I3{}, std::integral_constant<int, 4>{});      // a1.b1
                __builtin_amdgcn_sched_barrier(0);
                read_b(S{}, P{}, I0{});
                __builtin_amdgcn_sched_barrier(0);
                mfmas(pair_c, std::integral_constant<int, 4>{}, std::integral_constant<int, 5>{});   // a1.b2
                // (the a2 / a3 reads after Q are in by now; said explicitly, it keeps the compiler's count of
                // reads in flight across the loop edge below 16, else it waits for all of them at the top)
                if constexpr (pair == 3) __builtin_amdgcn_s_waitcnt(0xc27f);      // lgkmcnt(2)
                __builtin_amdgcn_sched_barrier(0);
                read_b(S{}, P{}, I1{});
                __builtin_amdgcn_sched_barrier(0);
                mfmas(pair_c, std::integral_constant<int, 5>{}, std::integral_constant<int, 6>{});   // a1.b3
                __builtin_amdgcn_sched_barrier(0);
                read_b(S{}, P{}, I2{});
                if constexpr (pair == 3) read_a(I0{});
            };
            __builtin_amdgcn_s_setprio(1);
            pair_block(I0{});
            pair_block(I1{});
            pair_block(I2{});
            pair_block(I3{});
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
        };
        for (int kt = 0; kt < n_kt; kt += 2) {
            kstep(I0{}, kt);
            kstep(I1{}, kt + 1);
        }
    };
    if (__builtin_amdgcn_readfirstlane(row0 + wm * (16 * NI) < g.m)) body(std::true_type{});
    else body(std::false_type{});
    __builtin_amdgcn_s_waitcnt(0x0070);              // the wasted DMA and reads of the last step

    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    const int rows_valid = min(g.m - row0, B3_TM);
    float *cbase = g.c + (int64_t)row0 * g.ldc + col0;
    __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(
        cbase, 0, (int)((int64_t)rows_valid * g.ldc * 4), 0x00020000);
    const uint32_t ldc_b = (uint32_t)g.ldc * 4;
    uint32_t cvoff[NJ];
    float bv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cl = wn * (16 * NJ) + j * 16 + rr;
        const bool ok = col0 + cl < g.n;
        cvoff[j] = ok ? (uint32_t)(wm * (16 * NI) + 4 * kg) * ldc_b + (uint32_t)cl * 4 : 0x7fffffffu;
        bv[j] = (g.bias != nullptr && ok) ? g.bias[col0 + cl] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t roff = (uint32_t)(i * 16 + e) * ldc_b;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float v = acc[i][j][e] + bv[j];
                if (rows_valid == B3_TM)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), crsrc, cvoff[j], roff, 0);
                else
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), crsrc, cvoff[j] + roff, 0, 0);
            }
        }
}

// The tiles the tail units computed: C tile = sum over its k slices of the partials, in slice order (+ bias).
// Grid (tile, accumulator register 0..15); a thread holds the element(s) its twin in gemm_b3_kernel held.
__global__ __launch_bounds__(B3_THREADS) void gemm_b3_tail_sum_kernel(B3Args g) {
    constexpr int NI = 4, NJ = 4;
    const TileOf tile = tile_of_linear(g.dp_tiles + (int)blockIdx.x, g.tiles_m, g.tiles_n);
    const int row0 = tile.bm * B3_TM, col0 = tile.bn * B3_TN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, rr = lane & 15, kg = lane >> 4;
    const int reg = blockIdx.y, i = reg / NJ, j = reg % NJ;
    const int row = row0 + wm * (16 * NI) + i * 16 + 4 * kg, col = col0 + wn * (16 * NJ) + j * 16 + rr;
    if (row0 + wm * (16 * NI) >= g.m || col >= g.n) return;      // (the first test is the one the producer made)
    const b3_f32x4 *part = reinterpret_cast<const b3_f32x4 *>(g.tail_partials) +
                           ((int64_t)blockIdx.x * g.tail_splits * (NI * NJ) + reg) * B3_THREADS + threadIdx.x;
    b3_f32x4 sum = part[0];
    for (int q = 1; q < g.tail_splits; ++q) sum += part[(int64_t)q * (NI * NJ) * B3_THREADS];
    const float bv = g.bias != nullptr ? g.bias[col] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (row + e < g.m) g.c[(int64_t)(row + e) * g.ldc + col] = sum[e] + bv;
}

// ---- host side: the plan (gemm_plan.h) says slices, tail units, tile and where the scratch sits ------------
// One launch for up to B3_SPLIT_MAX_JOBS splits: the grid is partitioned over the jobs, in list order.
int b3_split_jobs(const B3Dual *jobs, int n_jobs, hipStream_t st) {
    if (n_jobs < 1 || n_jobs > B3_SPLIT_MAX_JOBS) {
        set_error("b3_split_jobs: %d jobs (1 .. %d)", n_jobs, B3_SPLIT_MAX_JOBS);
        return GIST_EINVAL;
    }
    B3SplitList L{};
    int64_t blocks = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const B3Dual &d = jobs[i];
        if (d.rows <= 0 || d.cols <= 0) continue;
        B3SplitJob &J = L.job[L.n++];
        J.d = d;
        J.d.vec4 = aligned16(d.src) && d.ld % 4 == 0;
        J.ldd_r = b3_kpad(d.cols); J.ldd_t = b3_kpad(d.rows);
        J.mask = drop_mask_of(d.p, d.seed);
        J.gx = (int)ceil_div(d.dst_r ? J.ldd_r : d.cols, 64);
        J.gy = (int)ceil_div(d.dst_t ? J.ldd_t : d.rows, 64);
        J.first = (int)blocks;
        blocks += (int64_t)J.gx * J.gy;
    }
    if (L.n == 0) return GIST_OK;
    if (blocks >= (1LL << 31)) {
        set_error("b3_split_jobs: %lld blocks", (long long)blocks);
        return GIST_EINVAL;
    }
    hipLaunchKernelGGL(b3_split_kernel, dim3((unsigned)blocks), dim3(B3S_THREADS), 0, st, L);
    return launch_status("b3_dual_split");
}
int b3_dual_split(const B3Dual &d, hipStream_t st) { return b3_split_jobs(&d, 1, st); }

// slabs: the plan's scratch (fp32 slabs of the k slices, or the tail units' partials).  deferred != NULL: the caller's
// consumer sums the slabs (slab s at slabs + s m n, in slab order; bias must be null), *deferred = their number.
static int b3_launch(const char *name, const GemmPlan &pl, const uint16_t *sa, const uint16_t *sb, const float *bias,
                     float *c, int64_t ldc, int64_t m, int64_t n, int64_t k, float *slabs, hipStream_t st, int *deferred) {
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_b3_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, B3_STAGES * B3_BUF_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_b3_wide_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, B3W_LDS_BYTES);
        if (e != hipSuccess) {
            set_error("%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
            return GIST_ELAUNCH;
        }
        once.done(dev);
    }
    B3Args g;
    const int64_t kpad = b3_kpad(k);
    g.a = sa; g.lda = kpad; g.b = sb; g.ldb = kpad; g.bias = bias; g.c = c; g.ldc = ldc;
    g.m = (int)m; g.n = (int)n; g.kpad = (int)kpad;
    g.tiles_m = (int)ceil_div(m, pl.tile_m);
    g.tiles_n = (int)ceil_div(n, pl.tile_n);
    g.kt_per_split = (int)(pl.k_per_split / B3_BK);
    g.split_stride = 0;
    if (pl.splits > 1) { g.c = slabs; g.ldc = n; g.split_stride = m * n; g.bias = nullptr; }
    const int tail_tiles = g.tiles_m * g.tiles_n - pl.whole_tiles;
    g.dp_tiles = pl.whole_tiles; g.tail_splits = pl.tail_splits; g.tail_kt = (int)(pl.tail_k / B3_BK);
    g.tail_partials = pl.tail_splits > 1 ? slabs : nullptr;
    const int64_t slot = timer_begin(tl_timer, 2, m, n, k, st);      // kind 2: the main kernel (+ slab sum)
    if (pl.tile_n == B3W_TN)
        hipLaunchKernelGGL(gemm_b3_wide_kernel, dim3((unsigned)g.dp_tiles), dim3(B3_THREADS), B3W_LDS_BYTES, st, g);
    else
        hipLaunchKernelGGL(gemm_b3_kernel, dim3((unsigned)(pl.whole_tiles + tail_tiles * pl.tail_splits), (unsigned)pl.splits),
                           dim3(B3_THREADS), B3_STAGES * B3_BUF_BYTES, st, g);
    int rc = launch_status(name);
    if (rc == GIST_OK && pl.tail_splits > 1) {
        hipLaunchKernelGGL(gemm_b3_tail_sum_kernel, dim3((unsigned)tail_tiles, 16), dim3(B3_THREADS), 0, st, g);
        rc = launch_status(name);
    }
    if (deferred) *deferred = pl.splits;
    else if (rc == GIST_OK && pl.splits > 1) rc = splitk_reduce(name, slabs, m * n, pl.splits, bias, c, ldc, m, n, st);
    timer_end(tl_timer, slot, st);
    return rc;
}

// operands split once and kept by the caller (the step); slabs: its scratch for k slices or tail units
int b3_gemm_presplit(const char *name, const uint16_t *sa, const uint16_t *sb, const float *bias, float *c,
                     int64_t ldc, int64_t m, int64_t n, int64_t k, float *slabs, int64_t slab_bytes,
                     hipStream_t st, int *deferred) {
    if (ldc * B3_TM * 4 >= (1LL << 31)) {      // the store epilogue's 32-bit byte offsets: 256 rows x ldc
        set_error("%s: leading dimension of the output >= 2^21 elements on the bf16x3 path", name);
        return GIST_EINVAL;
    }
    const GemmPlan pl = plan_gemm(GemmQuery{true, true, m, n, k, 2, true, ldc, GEMM_CALL_KEPT, deferred != nullptr,
                                            slabs != nullptr && slab_bytes > 0 ? slab_bytes : 0, aligned16(slabs)});
    return b3_launch(name, pl, sa, sb, bias, c, ldc, m, n, k, slabs, st, deferred);
}

// A gist_gemm_* call on this path.  A: a_kc ? [m][k] : [k][m];  B: b_kc ? [n][k] : [k][n].
int b3_gemm(const char *name, const GemmPlan &pl, bool a_kc, bool b_kc, const float *a, int64_t lda, const float *b,
            int64_t ldb, const float *bias, float *c, int64_t ldc, int64_t m, int64_t n, int64_t k, void *ws, hipStream_t st) {
    const int64_t kpad = b3_kpad(k);
    uint16_t *sa = reinterpret_cast<uint16_t *>(static_cast<char *>(ws) + pl.operand_offset);
    uint16_t *sb = sa + m * kpad * 3;
    float *slabs = reinterpret_cast<float *>(static_cast<char *>(ws) + pl.scratch_offset);
    auto split = [&](bool kc, const float *src, int64_t ld, int64_t rows, uint16_t *dst) {
        B3Dual d{};
        d.src = src; d.ld = ld;
        if (kc) { d.rows = rows; d.cols = k; d.dst_r = dst; }      // [rows][k]
        else { d.rows = k; d.cols = rows; d.dst_t = dst; }         // [k][rows] -> transposed
        return b3_dual_split(d, st);
    };
    int rc = split(a_kc, a, lda, m, sa);
    if (rc == GIST_OK) rc = split(b_kc, b, ldb, n, sb);
    if (rc != GIST_OK) return rc;
    return b3_launch(name, pl, sa, sb, bias, c, ldc, m, n, k, slabs, st, nullptr);
}

}  // namespace gist
