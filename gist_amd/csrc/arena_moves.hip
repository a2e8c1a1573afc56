// Grouped block mover (gfx950): every block of a GIST dispatch or sync between two flat arenas in ONE launch
// (include/gist_hip.h, gist_arena_moves_*).
//
// The per-tensor movers (subgraph.hip: block_move_kernel, mean_rows_kernel) cost one launch -- and, from Python, one
// call -- per (site, layer, tensor); the blocks are small, so a sync is bound by the host's issue rate.  Here the
// host packs a table once: per move a 64-byte descriptor, then a prefix of tile counts.  The grid is 1-D over the tiles
// of all moves; a workgroup finds its move by a binary search of the prefix (uniform: scalar loads), then moves one
// tile:
//   GATHER / SCATTER   kTileRows x kTileCols cells, its threads sweeping the columns of one row after the other, so the
//                      contiguous side (dst of a gather, src of a scatter) is accessed in full lines, as in
//                      block_move_kernel; 16-byte accesses where the move's columns are identity-indexed and both
//                      bases, both pitches and the width are multiples of four floats, scalar ones otherwise (a block
//                      may start at ANY float offset);
//   MEAN               256 columns, one per thread, through mean_tree (mean_tree.h): gist_mean_rows_f32's bits.
// All offsets are 64-bit.  No atomics: the moves of one call never write the same cell, and the two arenas do not
// overlap (src is read through a __restrict__ pointer): the caller's contract.
// Bound: HBM, the bytes of the blocks.
#include "common.h"
#include "mean_tree.h"

namespace gist {

constexpr int kTileRows = 8;
constexpr int kTileCols = 1024;
constexpr int kMeanCols = 256;
constexpr int kMoveVec4 = 1;          // ArenaMoveDev::flags: offsets, pitches and width allow 16-byte accesses

struct ArenaMoveDev {                 // the device format of a gist_arena_move: 64 bytes
    int64_t src_off, dst_off, lds, ldd, row_idx, col_idx;
    int32_t n_rows, n_cols;
    int32_t kind, flags;
};
static_assert(sizeof(ArenaMoveDev) == 64, "packed table layout");

static inline int64_t moves_prefix_offset(int64_t n_moves) { return n_moves * (int64_t)sizeof(ArenaMoveDev); }
static inline int64_t moves_packed_bytes(int64_t n_moves) {
    return (moves_prefix_offset(n_moves) + (n_moves + 1) * (int64_t)sizeof(int32_t) + 15) / 16 * 16;
}

template <bool SCATTER, bool VEC>
__device__ __forceinline__ void move_tile(const ArenaMoveDev &m, int lt, const int32_t *__restrict__ idx,
                                          const float *__restrict__ src, float *__restrict__ dst) {
    const int col_chunks = (m.n_cols + kTileCols - 1) / kTileCols;
    const int r0 = (lt / col_chunks) * kTileRows;
    const int c0 = (lt % col_chunks) * kTileCols;
    const int rows = m.n_rows - r0 < kTileRows ? m.n_rows - r0 : kTileRows;
    const int cw = m.n_cols - c0 < kTileCols ? m.n_cols - c0 : kTileCols;
    const int32_t *row = m.row_idx >= 0 ? idx + m.row_idx : nullptr;
    const int32_t *col = m.col_idx >= 0 ? idx + m.col_idx : nullptr;
    const float *s = src + m.src_off;
    float *d = dst + m.dst_off;
    constexpr int W = VEC ? 4 : 1;
    const int per_row = cw / W;                         // (VEC: n_cols % 4 == 0, so every chunk is whole float4s)
    // Thread t takes cells t, t + 256, ... of the tile in row-major order (a narrow block still fills its waves).  The
    // cell's (row, column) is divided out once and then stepped: 256 = dr * per_row + dc, uniform per tile.
    const int dr = (int)blockDim.x / per_row, dc = (int)blockDim.x % per_row;
    int r = (int)threadIdx.x / per_row, c = (int)threadIdx.x % per_row;
    for (; r < rows; r += dr, c += dc) {
        if (c >= per_row) {
            c -= per_row;
            if (++r >= rows) break;
        }
        const int i = r0 + r;
        const int j = c0 + c * W;
        const int64_t ri = row ? row[i] : i;
        if constexpr (VEC) {                            // (identity columns)
            if constexpr (SCATTER)
                *reinterpret_cast<float4 *>(d + ri * m.ldd + j) = *reinterpret_cast<const float4 *>(s + (int64_t)i * m.lds + j);
            else
                *reinterpret_cast<float4 *>(d + (int64_t)i * m.ldd + j) = *reinterpret_cast<const float4 *>(s + ri * m.lds + j);
        } else {
            const int64_t cj = col ? col[j] : j;
            if constexpr (SCATTER) d[ri * m.ldd + cj] = s[(int64_t)i * m.lds + j];
            else d[(int64_t)i * m.ldd + j] = s[ri * m.lds + cj];
        }
    }
}

__global__ __launch_bounds__(256) void arena_moves_kernel(const ArenaMoveDev *__restrict__ moves,
                                                          const int32_t *__restrict__ tile_begin, int n_moves,
                                                          const int32_t *__restrict__ idx,
                                                          const float *__restrict__ src, float *__restrict__ dst,
                                                          int bases16) {
    const int t = blockIdx.x;
    // tile_begin[lo] <= t < tile_begin[hi]: a move without tiles is an empty interval and is never found
    int lo = 0, hi = n_moves;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_begin[mid] <= t) lo = mid;
        else hi = mid;
    }
    const ArenaMoveDev m = moves[lo];
    const int lt = t - tile_begin[lo];
    if (m.kind == GIST_MOVE_MEAN) {
        const int64_t j = (int64_t)lt * kMeanCols + threadIdx.x;
        if (j < m.n_cols) dst[m.dst_off + j] = mean_tree(src + m.src_off + j, m.lds, m.n_rows);
        return;
    }
    const bool vec = bases16 && (m.flags & kMoveVec4);
    if (m.kind == GIST_MOVE_SCATTER) {
        if (vec) move_tile<true, true>(m, lt, idx, src, dst);
        else move_tile<true, false>(m, lt, idx, src, dst);
    } else {
        if (vec) move_tile<false, true>(m, lt, idx, src, dst);
        else move_tile<false, false>(m, lt, idx, src, dst);
    }
}

// off + (rows - 1) * ld + cols <= numel, without overflow (every term >= 0)
static bool extent_fits(int64_t off, int64_t rows, int64_t ld, int64_t cols, int64_t numel) {
    __int128 end = (__int128)off + (__int128)(rows - 1) * ld + cols;
    return end <= (__int128)numel;
}

}  // namespace gist

using namespace gist;

extern "C" int64_t gist_arena_moves_packed_bytes(int64_t n_moves) {
    if (n_moves < 0 || n_moves >= (1LL << 31)) return -1;
    return moves_packed_bytes(n_moves);
}

extern "C" int gist_arena_moves_pack(const struct gist_arena_move *moves, int64_t n_moves, int64_t src_numel,
                                     int64_t dst_numel, int64_t idx_len, void *out_host, int64_t out_bytes,
                                     int64_t *n_tiles) {
    const char *me = "gist_arena_moves_pack";
    GIST_REQUIRE(n_moves >= 0 && n_moves < (1LL << 31), "%s: bad n_moves", me);
    GIST_REQUIRE(src_numel >= 0 && dst_numel >= 0 && idx_len >= 0, "%s: negative arena or index pool size", me);
    GIST_REQUIRE(out_host && n_tiles && (moves || n_moves == 0), "%s: null pointer", me);
    if (out_bytes < moves_packed_bytes(n_moves)) {
        set_error("%s: out_bytes %lld < %lld for %lld moves", me, (long long)out_bytes,
                  (long long)moves_packed_bytes(n_moves), (long long)n_moves);
        return GIST_ENOSPACE;
    }
    ArenaMoveDev *dev = static_cast<ArenaMoveDev *>(out_host);
    int32_t *prefix = reinterpret_cast<int32_t *>(static_cast<char *>(out_host) + moves_prefix_offset(n_moves));
    int64_t tiles = 0;
    for (int64_t k = 0; k < n_moves; ++k) {
        const gist_arena_move &m = moves[k];
        const long long kk = (long long)k;
        GIST_REQUIRE(m.n_rows >= 0 && m.n_cols >= 0, "%s: move %lld: negative size", me, kk);
        GIST_REQUIRE(m.n_rows < (1LL << 31) && m.n_cols < (1LL << 31), "%s: move %lld: size >= 2^31", me, kk);
        GIST_REQUIRE(m.kind == GIST_MOVE_GATHER || m.kind == GIST_MOVE_SCATTER || m.kind == GIST_MOVE_MEAN,
                     "%s: move %lld: unknown kind %d", me, kk, (int)m.kind);
        GIST_REQUIRE(m.src_off >= 0 && m.dst_off >= 0, "%s: move %lld: negative offset", me, kk);
        GIST_REQUIRE(m.lds >= 0 && m.ldd >= 0, "%s: move %lld: negative pitch", me, kk);
        GIST_REQUIRE(m.row_idx >= -1 && m.col_idx >= -1, "%s: move %lld: an index start below -1", me, kk);
        const bool empty = m.n_rows == 0 || m.n_cols == 0;
        int64_t n = 0;
        int flags = 0;
        if (m.kind == GIST_MOVE_MEAN) {
            GIST_REQUIRE(m.row_idx < 0 && m.col_idx < 0, "%s: move %lld: a MEAN takes no index lists", me, kk);
            GIST_REQUIRE(m.n_rows > 0 || m.n_cols == 0, "%s: move %lld: a MEAN of no sources", me, kk);
            if (!empty) {
                GIST_REQUIRE(extent_fits(m.src_off, m.n_rows, m.lds, m.n_cols, src_numel),
                             "%s: move %lld: the sources end past src_numel", me, kk);
                GIST_REQUIRE(extent_fits(m.dst_off, 1, 0, m.n_cols, dst_numel),
                             "%s: move %lld: the block ends past dst_numel", me, kk);
                n = ceil_div(m.n_cols, kMeanCols);
            }
        } else if (!empty) {
            const bool sc = m.kind == GIST_MOVE_SCATTER;
            // the dense side (dst of a gather, src of a scatter) is identity-indexed in both directions
            const int64_t dense_off = sc ? m.src_off : m.dst_off, dense_ld = sc ? m.lds : m.ldd;
            const int64_t dense_numel = sc ? src_numel : dst_numel;
            const int64_t ix_off = sc ? m.dst_off : m.src_off, ix_ld = sc ? m.ldd : m.lds;
            const int64_t ix_numel = sc ? dst_numel : src_numel;
            const char *dense = sc ? "src" : "dst", *ix = sc ? "dst" : "src";
            GIST_REQUIRE(dense_ld >= m.n_cols, "%s: move %lld: %s pitch %lld < n_cols %lld", me, kk, dense,
                         (long long)dense_ld, (long long)m.n_cols);
            GIST_REQUIRE(extent_fits(dense_off, m.n_rows, dense_ld, m.n_cols, dense_numel),
                         "%s: move %lld: the block ends past %s_numel", me, kk, dense);
            GIST_REQUIRE(m.col_idx >= 0 || ix_ld >= m.n_cols, "%s: move %lld: %s pitch %lld < n_cols %lld", me, kk, ix,
                         (long long)ix_ld, (long long)m.n_cols);
            // the indexed side as far as its identity directions reach: rows, columns or, with two lists, its first cell
            GIST_REQUIRE(extent_fits(ix_off, m.row_idx < 0 ? m.n_rows : 1, ix_ld, m.col_idx < 0 ? m.n_cols : 1, ix_numel),
                         "%s: move %lld: the block ends past %s_numel", me, kk, ix);
            GIST_REQUIRE(m.row_idx < 0 || (m.row_idx <= idx_len && m.n_rows <= idx_len - m.row_idx),
                         "%s: move %lld: row index list ends past idx_len", me, kk);
            GIST_REQUIRE(m.col_idx < 0 || (m.col_idx <= idx_len && m.n_cols <= idx_len - m.col_idx),
                         "%s: move %lld: column index list ends past idx_len", me, kk);
            n = ceil_div(m.n_rows, kTileRows) * ceil_div(m.n_cols, kTileCols);
            if (m.col_idx < 0 && ((m.src_off | m.dst_off | m.lds | m.ldd | m.n_cols) & 3) == 0) flags |= kMoveVec4;
        }
        GIST_REQUIRE(tiles + n < (1LL << 31), "%s: more than 2^31 - 1 tiles", me);
        ArenaMoveDev &d = dev[k];
        d.src_off = m.src_off; d.dst_off = m.dst_off; d.lds = m.lds; d.ldd = m.ldd;
        d.row_idx = m.row_idx; d.col_idx = m.col_idx;
        d.n_rows = (int32_t)m.n_rows; d.n_cols = (int32_t)m.n_cols;
        d.kind = m.kind; d.flags = flags;
        prefix[k] = (int32_t)tiles;
        tiles += n;
    }
    prefix[n_moves] = (int32_t)tiles;
    *n_tiles = tiles;
    return GIST_OK;
}

extern "C" int gist_arena_moves_f32(const void *packed_dev, int64_t n_moves, int64_t n_tiles, const int32_t *idx_dev,
                                    const float *src, float *dst, gist_stream_t stream) {
    GIST_REQUIRE(n_moves >= 0 && n_moves < (1LL << 31) && n_tiles >= 0 && n_tiles < (1LL << 31),
                 "gist_arena_moves_f32: bad n_moves or n_tiles");
    if (n_tiles == 0) return GIST_OK;
    GIST_REQUIRE(n_moves > 0, "gist_arena_moves_f32: tiles without moves");
    GIST_REQUIRE(packed_dev && src && dst, "gist_arena_moves_f32: null pointer");
    GIST_REQUIRE(aligned16(packed_dev), "gist_arena_moves_f32: packed_dev must be 16-byte aligned");
    const ArenaMoveDev *moves = static_cast<const ArenaMoveDev *>(packed_dev);
    const int32_t *prefix =
        reinterpret_cast<const int32_t *>(static_cast<const char *>(packed_dev) + moves_prefix_offset(n_moves));
    hipLaunchKernelGGL(arena_moves_kernel, dim3((unsigned)n_tiles), dim3(256), 0, as_stream(stream), moves, prefix,
                       (int)n_moves, idx_dev, src, dst, (int)(aligned16(src) && aligned16(dst)));
    return launch_status("gist_arena_moves_f32");
}
