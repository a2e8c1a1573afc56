// The prepared block structure of a batch: what gist_spmm_blocks_prepare (spmm_mfma.hip) writes and the
// block-dense aggregations of spmm_mfma.hip and spmm_dense32.hip read.
//
// One record of MF_PREP_STRIDE bytes per block:
//   the count image       [k chunk 16][row 128][8 k] bf16: the block's edge counts (<= 256, exact in bf16)
//   int rem_cnt[128]      rem_cnt[r] >= 0: bits 0-7 = listed outside neighbours, bit 8 (MF_PAIR_FLAG) = the row has
//                         edges in a pair image; -1: gather the row in full; -2: walk the edge list for the neighbours
//                         outside the block and its pairs.  Every reader that does not apply the pair images treats a
//                         flagged row as -1, so a structure prepared with or without pairs is correct for any reader
//                         (the caller's pairs choice is speed only)
//   int rem_col[128][8]   the listed outside neighbours, CSR order
//   int pair[2][2]        (first source row, source rows) of the block's pairs
// When the batch is small enough to look for pairs (spmm_mfma.hip), MF_PAIRS count images per block, the pair
// images, follow the records of all blocks (gist_spmm_blocks_bytes).
#pragma once

namespace gist {

constexpr int MF_ROWS = 128;                       // rows of a block = k extent of its product
constexpr int MF_REM = 8;                          // outside neighbours listed per row
constexpr int MF_IMG_BYTES = 16 * MF_ROWS * 16;    // one count image
constexpr int MF_PREP_REMC = MF_IMG_BYTES;                           // byte offset of rem_cnt in a record
constexpr int MF_PREP_REMCOL = MF_PREP_REMC + MF_ROWS * 4;           // ... of rem_col
constexpr int MF_PREP_PINFO = MF_PREP_REMCOL + MF_ROWS * MF_REM * 4; // ... of pair
constexpr int MF_PREP_STRIDE = MF_PREP_PINFO + 16;
constexpr int MF_PAIRS = 2;                        // pair images per block
constexpr int MF_PAIR_FLAG = 0x100;                // rem_cnt: the row has edges in a pair image
static_assert(MF_PREP_STRIDE % 16 == 0, "records stay 16-byte aligned");
static_assert(MF_REM < MF_PAIR_FLAG, "the count bits of rem_cnt hold the list length");

}  // namespace gist
