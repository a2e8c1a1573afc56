// The mean over n_src sources of one element, shared by mean_rows_kernel (subgraph.hip) and the grouped mover's MEAN
// moves (arena_moves.hip): both give the same bits.
#pragma once
#include <stdint.h>

namespace gist {

// Pairwise (tree) summation over the sources: for identical copies and a power-of-two
// count every partial sum is exact, so "dispatch -> sync without training" leaves the shared
// bias bit-identical (a sequential sum rounds at 3x).  Deterministic for any count.
// src points at source 0's element; source k's is src[k * stride].
__device__ __forceinline__ float mean_tree(const float *__restrict__ src, int64_t stride, int n_src) {
    constexpr int kMax = 64;
    float v[kMax];
    float tail = 0.f;
    const int m = n_src < kMax ? n_src : kMax;
    for (int k = 0; k < kMax; ++k) v[k] = k < m ? src[(int64_t)k * stride] : 0.f;
    for (int k = kMax; k < n_src; ++k) tail += src[(int64_t)k * stride];
#pragma unroll
    for (int w = 1; w < kMax; w <<= 1)
#pragma unroll
        for (int k = 0; k + w < kMax; k += 2 * w) v[k] += v[k + w];
    return (v[0] + tail) / (float)n_src;
}

}  // namespace gist
