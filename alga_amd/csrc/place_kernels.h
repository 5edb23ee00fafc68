// alga_amd/csrc/place_kernels.h -- launchers of place_kernels.hip: reads placed on sequences, depth, pairs (include/alga_amd.h:
// alga_place_reads_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seed_index.h"

namespace alga {

// counters[] (unsigned long long): the refusal flags and what the checks measure, then what the kernels count
enum { PL_BAD_TWIN = 0, PL_BAD_PAIR, PL_BAD_LEN, PL_COLUMNS, PL_INDEX_POS, PL_MAX_READ_LEN, PL_DISTINCT, PL_PLACED, PL_UNIQUE, PL_SATURATED, PL_SEEDS,
       PL_SEEDS_OVER, PL_PAIRS, PL_PROPER, PL_IMPROPER, PL_SPLIT, PL_NOT_UNIQUE, PL_INSERT_SUM, PL_COUNTERS };

// pair_off (may be null): values <= 2, equal on a node and its twin, the mate in range and pointing back (*bad_pair = 1 otherwise);
// counters[PL_MAX_READ_LEN] = the longest node
void launch_pl_node_check(const uint8_t *pair_off, const int32_t *len, uint64_t n, unsigned long long *counters, hipStream_t s);
// target lengths >= 0 (PL_BAD_LEN), their 64-bit sum (PL_COLUMNS), the indexed positions sum of max(0, len - k + 1) (PL_INDEX_POS)
void launch_pl_target_check(const int32_t *tlen, uint64_t T, int32_t k, unsigned long long *counters, hipStream_t s);
// begin / len of the targets of a final result: target j = the window of the pair order[j]
void launch_pl_final_targets(const unsigned long long *word_off, const uint8_t *verdict, const int32_t *order, const int32_t *begin, const int32_t *len, uint64_t n,
                             unsigned long long *tbegin, int32_t *tlen, hipStream_t s);

// the targets in column space, the space their index is built over (alga_seed_index): off = col_off (T + 1), len = the target lengths, n = T
typedef SeedSpace PlTargets;
// cols: the ragged targets repacked (the buffer is zeroed by the caller)
void launch_pl_gather(const uint32_t *words, const unsigned long long *begin, const PlTargets &t, uint32_t *cols, hipStream_t s);

struct PlOut {
    int32_t *target, *pos;
    uint8_t *mm, *hits, *state;
};
// the placement itself: one wave per read, both strands (blocks: seed_blocks(R), the scratch: seed_scratch_words)
void launch_pl_place(const SeedReads &r, const PlTargets &t, const SeedIndex &x, int32_t k, int32_t max_mm, int32_t max_occ, const PlOut &o, unsigned long long *scratch,
                     uint32_t scratch_words_per_wave, int blocks, unsigned long long *counters, hipStream_t s);

// +1 / -1 of every counting read into diff[] (columns + 1 entries, zeroed), the per-target sums into tstat[4][T] (reads, bases, mismatches, uncovered)
void launch_pl_depth_add(const SeedReads &r, const PlTargets &t, const PlOut &o, int multi, uint32_t *diff, unsigned long long *tstat, hipStream_t s);
// tstat[3][t] += columns of t with cover 0
void launch_pl_uncovered(const PlTargets &t, const uint32_t *cover, unsigned long long *tstat, hipStream_t s);
// the pairs: counters[PL_PAIRS ..], hist[max_insert + 1] (zeroed)
void launch_pl_pairs(const SeedReads &r, const uint8_t *pair_off, const PlOut &o, int32_t max_insert, unsigned long long *hist, unsigned long long *counters, hipStream_t s);

// the FASTA of a final result with depth headers: record j is the accepted pair of id j = target j
struct PlFasta {
    const uint32_t *words;
    const unsigned long long *word_off;
    const uint8_t *verdict;
    const int32_t *order, *begin, *len;
    const unsigned long long *t_reads, *t_bases;
    uint64_t n;
};
void launch_pl_fasta_sizes(const PlFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_pl_fasta_write(const PlFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
