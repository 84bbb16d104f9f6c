// patterns.h -- the block-pattern table of the row-gather SpMV (patterns.hip builds it, spmv.hip reads it).
#pragma once
#include "common.h"

namespace hpcla {

constexpr int PAT_RPB = 256;                 // rows per block (== RPB of spmv.hip, asserted there)
// One pattern in the table, in 16-bit entries from a 16-byte aligned start:
//   [0 .. 256]   row bounds relative to the block's first entry (rows past the block's last repeat the last bound)
//   [257], [258] the block's row count and the position of its first entry modulo 8 (its "phase")
//   [260 .. 269] five 32-bit bounds of the block's four waves (the bounds of rows 0, 64, 128, 192 and 256 once more: the
//                kernel reads a wave's range with scalar loads)
//   [272 ...]    the block-relative columns, entry j of the block at 272 + phase + j: the kernel's 16-byte loads, which
//                start at (first entry & ~7), read it directly; rounded up to a whole vector of 8
constexpr int PAT_HEAD = 272;
constexpr int PAT_NR = 257, PAT_PHASE = 258, PAT_WAVE = 260;
constexpr int64_t PAT_TABLE_CAP_BYTES = 256 * 1024;   // a small share of one XCD's 4 MiB L2, next to the x lines
constexpr int64_t PAT_MAX_LEN = 65535;                // 16-bit bounds

// per row block: first stored entry (0-based) and the pattern's place in the table in 16-byte units (< 0: not in the table)
struct alignas(8) PatRec {
    int32_t first;
    int32_t id;
};

// what a launch of the pattern form reads (null rec: the launch has no table)
struct PatArgs {
    const PatRec *rec;
    const int16_t *table;
};

}  // namespace hpcla

struct hpcla_block_patterns {
    int64_t nrows = 0, nnz = 0, all_blocks = 0;
    int index_base = 0;
    hpcla::PatRec *rec = nullptr;        // all_blocks records
    int16_t *table = nullptr;
    int64_t table_bytes = 0, n_patterns = 0, n_candidates = 0, n_patterned = 0;
};
