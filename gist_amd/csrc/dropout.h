// The dropout mask: THE definition of gist_dropout_f32's generator, for every kernel that applies or folds a mask.
// No mask is ever stored: forward and backward agree because every site computes the same bits from (seed, element index):
//   one splitmix64 of (index >> 1) + sm per element PAIR, sm = seed * golden ratio;
//   an even index takes the low 32-bit word of the hash, an odd index the high word;
//   factor = (word >> 8) * 2^-24 >= p ? 1 / (1 - p) : 0.
// A masked value is v * factor -- a multiply by 0.f, never a select: NaN and infinity survive a dropped element as NaN,
// a dropped negative value (and -0) becomes -0.  A site that skips the mask for p = 0 stores v itself.
// (partition.hip's Rng is a different generator that shares the constant.)
#pragma once
#include <stdint.h>

namespace gist {

struct DropMask {
    float p, scale;      // drop probability, 1 / (1 - p)
    uint64_t sm;         // seed * golden ratio
};

// One guard: every entry point admits p in [0, 1) only, where `p > 0` and `p > 0 && p < 1` agree; p = 0 gives scale 1
// (and a factor of 1 everywhere: 0 is never above a word's fraction).
static inline float drop_scale_of(float p) { return p > 0.f ? 1.0f / (1.0f - p) : 1.f; }
static inline DropMask drop_mask_of(float p, uint64_t seed) {
    DropMask m;
    m.p = p; m.scale = drop_scale_of(p);
    m.sm = seed * 0x9E3779B97F4A7C15ULL;
    return m;
}

#ifdef __HIPCC__
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// the hash of pair index `pair` (= element index >> 1), the word of an element index, the factor of a word
__device__ __forceinline__ uint64_t drop_hash(uint64_t pair, const DropMask &m) { return splitmix64(pair + m.sm); }
__device__ __forceinline__ uint32_t drop_word(uint64_t idx, const DropMask &m) {
    const uint64_t h = drop_hash(idx >> 1, m);
    return (idx & 1) ? (uint32_t)(h >> 32) : (uint32_t)h;
}
__device__ __forceinline__ float drop_factor(uint32_t w, const DropMask &m) {
    return ((float)(w >> 8) * (1.0f / 16777216.0f) >= m.p) ? m.scale : 0.f;
}
__device__ __forceinline__ float drop_keep(uint64_t idx, const DropMask &m) { return drop_factor(drop_word(idx, m), m); }

// The factors of the four consecutive indices idx0 .. idx0 + 3: two hashes when idx0 is even, three when it is odd.
// THE quad form: every site but one uses it, through drop_f4 / drop_vec<4>.  (A site whose launcher admits even indices
// only says so with __builtin_assume and gets the two-hash code alone: dropout_vec4_kernel and narrow_nn_drop_kernel in
// rowops.hip.  The assume is a promise -- an odd index there is undefined behaviour -- so it stands or falls with the
// launcher's condition, marked at both launchers.)
__device__ __forceinline__ void drop_factors4(float (&f)[4], uint64_t idx0, const DropMask &m) {
    const uint64_t pair = idx0 >> 1;
    const uint64_t h0 = drop_hash(pair, m), h1 = drop_hash(pair + 1, m);
    uint32_t w0 = (uint32_t)h0, w1 = (uint32_t)(h0 >> 32), w2 = (uint32_t)h1, w3 = (uint32_t)(h1 >> 32);
    if (idx0 & 1) {
        w0 = w1; w1 = w2; w2 = w3; w3 = (uint32_t)drop_hash(pair + 2, m);
    }
    f[0] = drop_factor(w0, m); f[1] = drop_factor(w1, m); f[2] = drop_factor(w2, m); f[3] = drop_factor(w3, m);
}
// The same factors without a branch: three hashes always, then a word select.  Used by b3_split_kernel (gemm_b3.hip)
// alone: eight quads per thread between a load phase and two LDS phases, where the branch of the form above cost
// 0.5 us of 44.4 (1.1 us with an odd offset) on the 2046 x 8192 split -- profiles/dropout_one_generator.md.
__device__ __forceinline__ void drop_factors4_flat(float (&f)[4], uint64_t idx0, const DropMask &m) {
    const uint64_t pair = idx0 >> 1;
    const uint64_t h0 = drop_hash(pair, m), h1 = drop_hash(pair + 1, m), h2 = drop_hash(pair + 2, m);
    const bool odd = (idx0 & 1) != 0;
    f[0] = drop_factor(odd ? (uint32_t)(h0 >> 32) : (uint32_t)h0, m);
    f[1] = drop_factor(odd ? (uint32_t)h1 : (uint32_t)(h0 >> 32), m);
    f[2] = drop_factor(odd ? (uint32_t)(h1 >> 32) : (uint32_t)h1, m);
    f[3] = drop_factor(odd ? (uint32_t)h2 : (uint32_t)(h1 >> 32), m);
}
__device__ __forceinline__ void drop_f4(float4 &v, uint64_t idx0, const DropMask &m) {
    float f[4];
    drop_factors4(f, idx0, m);
    v.x *= f[0]; v.y *= f[1]; v.z *= f[2]; v.w *= f[3];
}
// VEC consecutive elements from idx0 (VEC = 4: the quad form)
template <int VEC>
__device__ __forceinline__ void drop_vec(float (&v)[VEC], uint64_t idx0, const DropMask &m) {
    if constexpr (VEC == 4) {
        float f[4];
        drop_factors4(f, idx0, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= f[k];
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] *= drop_keep(idx0 + k, m);
    }
}
#endif

}  // namespace gist
