// The device primitives more than one kernel file uses, each stated once (gfx950; wave = 64 lanes).  common.h includes
// this header; it holds device code only.
//
// Deliberately NOT merged here, because a merge would change results or instruction streams:
//   - the xor-butterfly sums (adam_wave_sum, wave_sum_f64, the block counts of subgraph.hip, group_sum / across_groups of
//     gat.hip) are not wave_sum: they add in another order, and tests compare those kernels bit for bit with their twins;
//   - ln_affine_finish_kernel and colsum_chunks_kernel add in the same order but load differently;
//   - mf_image_to_lds (spmm_mfma.hip) has a bounded resource and offsets of its own, so it is not lds_dma_image;
//   - the C-tile stores of the GEMM kernels (raw buffer stores, gemm.hip's epilogue has the comment): gemm_h3_kernel,
//     gemm_b3_kernel, gemm_b3_wide_kernel and gemm_bf16x1_kernel store the same 16x16x32 accumulator layout, but as one
//     function over a value functor the store changed the register allocation of three of the four, k loop included (the
//     per-lane column of the store is the same value as a fragment row of the k loop, and only next to each other are the
//     two computed once), so each kernel keeps its own;
//   - b3_split_kernel's ragged load covers 8 rows per thread and tests rows and columns per element: not load4_ragged;
//   - "8 consecutive k of a row, zero past k" stays h3_load8 in gemm_h3.hip and inline in x1_cast_kernel: as a call, the
//     loop inside it is unrolled before it is inlined, and x1_cast_kernel's two branches are then laid out the other way;
//   - for the same reason the two row maxima at the end of ln_relu_bwd_kernel (rowops.hip) keep wave_max open-coded;
//   - lnaffine.hip's re-reading path (d > 4096) keeps its Pack<VEC> / ld / st / sum_pack: on vload / vstore / vsum over
//     float[VEC] its five TPR = 256 kernels come out with other address arithmetic and more instructions;
//   - the LN + ReLU kernels of rowops.hip and the affine ones of lnaffine.hip stay two kernel families.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gist {

// ---- reductions ---------------------------------------------------------------------------------------------------
// Sum over the 64 lanes of a wave, the same bits in every lane.  Within a row of 16 lanes on the DPP path of the vector unit
// (lane ^ 1, lane ^ 2 as quad permutes; the other quad of the half row and the other half row as mirrors -- every lane of a
// quad / half row holds the same partial sum by then), the four rows through the scalar unit: 4 + 4 + 3 instructions, none of
// them on the LDS pipe (the __shfl_xor butterfly is six dependent ds_bpermute round trips).
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_move<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v += dpp_move<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v += dpp_move<0x141>(v);      // row_half_mirror
    v += dpp_move<0x140>(v);      // row_mirror
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return (r0 + r1) + (r2 + r3);
}

// Maximum over the 64 lanes of a wave, the same value in every lane.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// Sum over the TPR threads that own one row (TPR = 64: a wave; TPR = 256: the block, red = 4 floats of LDS).
template <int TPR>
__device__ __forceinline__ float row_sum(float v, float *red) {
    v = wave_sum(v);
    if constexpr (TPR == 64) {
        return v;
    } else {
        const int w = threadIdx.x >> 6;
        __syncthreads();                      // red[] may still be read from a previous call
        if ((threadIdx.x & 63) == 0) red[w] = v;
        __syncthreads();
        return red[0] + red[1] + red[2] + red[3];
    }
}

// ---- VEC consecutive floats <-> registers (VEC = 1, 2, 4: one 4-, 8- or 16-byte access) -----------------------------
template <int VEC> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<2> { using T = float2; };
template <> struct Vec<4> { using T = float4; };

template <int VEC>
__device__ __forceinline__ void vload(const float *p, float (&v)[VEC]) {
    using T = typename Vec<VEC>::T;
    T t = *reinterpret_cast<const T *>(p);
    if constexpr (VEC == 1) { v[0] = t; }
    if constexpr (VEC == 2) { v[0] = t.x; v[1] = t.y; }
    if constexpr (VEC == 4) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
}

template <int VEC>
__device__ __forceinline__ void vstore(float *p, const float (&v)[VEC]) {
    using T = typename Vec<VEC>::T;
    T t;
    if constexpr (VEC == 1) { t = v[0]; }
    if constexpr (VEC == 2) { t.x = v[0]; t.y = v[1]; }
    if constexpr (VEC == 4) { t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; }
    *reinterpret_cast<T *>(p) = t;
}

// unit u of p: the VEC floats at p + VEC u.  (Not spelt vload<VEC>(p + VEC * u, v) at the call sites: with the address
// formed by the caller, the whole-tensor LayerNorm kernels come out with other registers.)
template <int VEC>
__device__ __forceinline__ void vload(const float *p, int64_t u, float (&v)[VEC]) { vload<VEC>(p + VEC * u, v); }
template <int VEC>
__device__ __forceinline__ void vstore(float *p, int64_t u, const float (&v)[VEC]) { vstore<VEC>(p + VEC * u, v); }

// their sum, pairwise: (v0 + v1) + (v2 + v3)
template <int VEC>
__device__ __forceinline__ float vsum(const float (&v)[VEC]) {
    if constexpr (VEC == 4) return (v[0] + v[1]) + (v[2] + v[3]);
    else if constexpr (VEC == 2) return v[0] + v[1];
    else return v[0];
}

// two bf16 -> one 32-bit word, lo in the low half
__device__ __forceinline__ uint32_t pack_bf16x2(__bf16 lo, __bf16 hi) {
    return (uint32_t)__builtin_bit_cast(unsigned short, lo) |
           ((uint32_t)__builtin_bit_cast(unsigned short, hi) << 16);
}

// ---- ragged load of the pre-passes ----------------------------------------------------------------------------------
// columns c .. c + 3 of a row with `cols` columns (p points at column c) into v: one float4 if `whole`, else the
// columns that exist one by one; a component past the right edge keeps what the caller put there (0.f)
template <typename I>
__device__ __forceinline__ void load4_ragged(const float *p, I c, I cols, bool whole, float4 &v) {
    if (whole) {
        v = *reinterpret_cast<const float4 *>(p);
    } else {
        if (c + 0 < cols) v.x = p[0];
        if (c + 1 < cols) v.y = p[1];
        if (c + 2 < cols) v.z = p[2];
        if (c + 3 < cols) v.w = p[3];
    }
}
// (rows that are 16-byte aligned at every c: the float4 whenever all four columns exist)
template <typename I>
__device__ __forceinline__ void load4_ragged(const float *p, I c, I cols, float4 &v) {
    load4_ragged(p, c, cols, c + 3 < cols, v);
}

// ---- block index -> output tile ---------------------------------------------------------------------------------------
// XCDs of the device the library runs on (gfx950: 8); blockIdx -> tile maps deal work round-robin to XCDs the way the
// hardware dispatches consecutive workgroups.
constexpr int kXcds = 8;
// tile rows of a super-tile: the tiles one XCD's L2 works on at a time are kTileGroupRows tile rows deep
constexpr int kTileGroupRows = 8;

// Workgroup `orig` of nwg runs on XCD orig % kXcds; the XCDs get consecutive ranges of the linear tile order.
__device__ __forceinline__ int xcd_linear(int orig, int nwg) {
    const int qd = nwg / kXcds, rm = nwg % kXcds, xcd = orig % kXcds;
    return (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + orig / kXcds;
}

// Linear index L -> tile (bm, bn): super-tiles of kTileGroupRows tile rows (fewer in the last), column by column inside.
struct TileOf { int bm, bn; };
__device__ __forceinline__ TileOf tile_of_linear(int L, int tiles_m, int tiles_n) {
    constexpr int GM = kTileGroupRows;
    const int width = GM * tiles_n;
    const int group = L / width;
    const int first_m = group * GM;
    const int gsz = min(tiles_m - first_m, GM);
    const int bm = first_m + (L % width) % gsz;
    const int bn = (L % width) / gsz;
    return {bm, bn};
}

// ---- global -> LDS by DMA ---------------------------------------------------------------------------------------------
// DMA instructions first .. first + NI - 1 of an operand image: instruction j fills LDS bytes [1024 j, 1024 (j + 1)) of
// `image`, a lane's 16 bytes from byte off[j - first] (off[0 .. NI)) behind `base` (uniform).  The resource has no bound
// of its own (range 0x7fffffff): the offsets are clamped by the kernel's *_dma_offsets, which encode each image's swizzle.
template <int NI, typename E>
__device__ __forceinline__ void lds_dma_image(const E *base, const uint32_t *off, char *image, int first) {
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<E *>(base), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int jj = 0; jj < NI; ++jj)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(image + (first + jj) * 1024),
                                                 16, off[jj], 0, 0, 0);
}

}  // namespace gist
#endif
