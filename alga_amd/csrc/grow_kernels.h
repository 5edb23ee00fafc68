// alga_amd/csrc/grow_kernels.h -- launchers of grow_kernels.hip: contig ends grown with the reads that hang over them
// (include/alga_amd.h: alga_grow_placed_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seed_index.h"

namespace alga {

// counters[] (unsigned long long): the refusal flags, then what the kernels count
enum { GR_BAD = 0, GR_BAD_TWIN /* a 32-bit flag of k_cr_twin */, GR_MAX_LEN, GR_INDEX_POS, GR_OVERHANGING, GR_VOTING, GR_SATURATED, GR_SEEDS, GR_SEEDS_OVER,
       GR_ENDS_VOTERS, GR_ENDS_GROWN, GR_ADDED, GR_LONGEST_GROWTH, GR_STOPS_COVER, GR_STOPS_PERCENT, GR_STOPS_MAX, GR_COLUMNS_AFTER, GR_LONGEST, GR_BAD_NEWLEN, GR_END_COLUMNS,
       GR_COUNTERS };
constexpr uint32_t GR_BAD_LEN = 1, GR_BAD_COLUMNS = 2;                 // bits of counters[GR_BAD]
constexpr uint8_t  GR_ST_OVERHANGS = 1, GR_ST_VOTES = 2, GR_ST_MINUS = 4;   // ALGA_GROW_* of include/alga_amd.h

// the placed targets in the placement's column space
struct GrTargets {
    const uint32_t *col_off;          // T + 1
    uint32_t T;
    uint64_t columns;                 // col_off[T]
    const uint32_t *cols;             // their bases: the placement's column array or the polish's
    uint32_t max_blocks;              // the cap of every grid here that a loop strides over (8192; option "grow_max_blocks")
};
// the 2T end sequences in a column space of their own, the space their index is built over (alga_seed_index): end e is the columns
// off[e] .. off[e] + len[e] (len[e] = W_e), the contig end at the right; n = 2T
typedef SeedSpace GrEnds;
struct GrOut {
    int32_t *end, *over;
    uint8_t *mm, *hits, *state;
};

// every len <= 16 * stride, columns == col_off[T] (the flags of counters[GR_BAD]); counters[GR_MAX_LEN] = the longest node
void launch_gr_check(const SeedReads &r, const GrTargets &t, unsigned long long *counters, hipStream_t s);
// flag[r] = 1 where read r lacks PLACED and has len >= min_anchor + 1 (R + 1 entries, the last 0)
void launch_gr_candidates(const SeedReads &r, const uint8_t *pl_state, int32_t min_anchor, uint32_t *flag, uint32_t max_blocks, hipStream_t s);
// the candidates' ids at the places the scan of flag[] gives
void launch_gr_compact(const uint32_t *flag, const uint32_t *pos, uint64_t R, uint32_t *cand, uint32_t max_blocks, hipStream_t s);
// elen[e] = W_e (2T + 1 entries, the last 0); counters[GR_END_COLUMNS] += W_e, [GR_INDEX_POS] += max(0, W_e - k + 1)
void launch_gr_end_lens(const GrTargets &t, int32_t max_len, int32_t k, int32_t *elen, unsigned long long *counters, hipStream_t s);
// the end sequences, one thread per word: the right ends copied, the left ones complemented and mirrored
void launch_gr_ends(const GrTargets &t, const GrEnds &e, uint32_t *ecols, hipStream_t s);
// one wave per candidate, both nodes (blocks: seed_blocks(n_cand) under the cap, the scratch: seed_scratch_words of that count)
void launch_gr_place(const SeedReads &r, const uint32_t *cand, uint64_t n_cand, const GrEnds &e, const SeedIndex &x, int32_t k, int32_t max_mm, int32_t max_occ,
                     int32_t min_anchor, const GrOut &o, unsigned long long *scratch, uint32_t scratch_words_per_wave, int blocks, unsigned long long *counters,
                     hipStream_t s);
// one wave per candidate that votes: count[(e * max_grow + i) * 4 + base]++, voters[e]++
void launch_gr_vote(const SeedReads &r, const uint32_t *cand, uint64_t n_cand, const GrOut &o, int32_t max_grow, uint32_t *count, uint32_t *voters, uint32_t max_blocks,
                    hipStream_t s);
// one thread per end: x[e] = the leading passing columns, g[e * max_grow + i] their bases, stop[e]; the counters of the ends
void launch_gr_decide(const uint32_t *count, const uint32_t *voters, uint32_t E, int32_t max_grow, int32_t min_cover, int32_t min_percent, uint32_t *x, uint8_t *g,
                      uint8_t *stop, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// left / right / new length per target (T + 1 entries of newlen, the last 0); counters[GR_COLUMNS_AFTER], [GR_LONGEST], [GR_BAD_NEWLEN]
void launch_gr_lens(const GrTargets &t, const uint32_t *x, uint32_t *left, uint32_t *right, int32_t *newlen, unsigned long long *counters, hipStream_t s);
// the grown targets' column array, one thread per word; begin[t] = new_off[t]
void launch_gr_build(const GrTargets &t, const uint32_t *new_off, uint64_t new_columns, const uint32_t *left, const uint8_t *g, int32_t max_grow, uint32_t *words,
                     unsigned long long *begin, hipStream_t s);

// `>contig_id=<t>_length=<len>_left=<xl>_right=<xr>\n<target>\n`, one record per target with a length
struct GrFasta {
    const uint32_t *words, *col_off;
    const int32_t *len;
    const uint32_t *left, *right;
    uint64_t n;
    uint32_t max_blocks;              // the cap of the write grid (16384 unless option "grow_max_blocks" lowers it)
};
void launch_gr_fasta_sizes(const GrFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_gr_fasta_write(const GrFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
