// alga_amd/csrc/seed_index.h -- the k-mer index over a packed column array that the placement, the grow and the merge stage seed from, and
// how it is built (seed_index.hip).  The device side of a look-up is seed_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct alga_engine;

namespace alga {

constexpr int SEED_BLOCK = 256, SEED_WAVES = SEED_BLOCK / 64;
constexpr int SEED_DIR_BITS_MAX = 26;

// n items laid one after the other in a column space: item i is the columns off[i] .. off[i] + len[i] (off[i + 1] may lie further on: padding);
// position q of item i is indexed where q + k <= len[i]
struct SeedSpace {
    const uint32_t *off;              // n + 1
    const int32_t *len;               // n
    uint32_t n;
    uint64_t columns;                 // off[n]
    const uint32_t *cols;             // column g in word g >> 4; two zero words behind the last
};
struct SeedIndex {
    const unsigned long long *keys;   // sorted; the first n are k-mers
    const uint32_t *vals;             // their columns
    const uint32_t *dir;
    int32_t shift;                    // bucket = k-mer >> shift
    uint32_t n;
};
// the reads as node rows: read r is row 2r + 1, its reverse complement row 2r
struct SeedReads {
    const uint32_t *rows;
    int32_t stride;
    const int32_t *len;               // 2R
    uint64_t R;
};

// the grid of a kernel that gives every query a wave: 8 blocks per CU (the look-ups are dependent random reads: occupancy is what hides them)
int    seed_blocks(uint64_t queries, int n_cu);
// words of the per-wave scratch (usable-seed masks of a query with more than 64 seeds): blocks * waves a block * ceil(max seeds / 64)
size_t seed_scratch_words(int blocks, int64_t max_query_len, int32_t k);

}  // namespace alga

// The index of sp's n_index indexed positions, in the engine's one index workspace (seed_keys / seed_vals / seed_dir: no call reads the index
// of an earlier one).  keys[g] = the k-mer at column g where it is an indexed position, 2^(2k) elsewhere (above every k-mer: sorted by
// sort_u64_u32 on 2k + 1 bits, the indexed positions are the head of the sorted keys, no compaction), vals[g] = g; dir[b] = the first of the
// n_index sorted keys with (key >> shift) >= b, b = 0 .. 2^bits (about two positions per bucket, or option "place_dir_bits"; at most 2k bits);
// *d_distinct += the distinct k-mers where d_distinct is not null.  ALGA_OK or the error code, the message set.
int alga_seed_index(alga_engine *e, const alga::SeedSpace &sp, int32_t k, uint64_t n_index, unsigned long long *d_distinct, hipStream_t s, alga::SeedIndex *out);
