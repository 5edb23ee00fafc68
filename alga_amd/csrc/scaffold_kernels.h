// alga_amd/csrc/scaffold_kernels.h -- launchers of scaffold_kernels.hip: scaffolds from the pairs the placement split over two targets
// (include/alga_amd.h: alga_scaffold_placed_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_kernels.h"

namespace alga {

// counters[] (unsigned long long): the refusal flags, then what the kernels count
enum { SC_BAD = 0, SC_SPLIT, SC_LINKS, SC_TOO_FAR, SC_BUNDLES, SC_SUPPORTED, SC_AMBIGUOUS, SC_JOINS, SC_DROPPED, SC_SCAFFOLDS, SC_MULTI, SC_MEMBERS, SC_LONGEST,
       SC_COUNTERS };
constexpr uint32_t SC_BAD_PAIR = 1, SC_BAD_LEN = 2, SC_BAD_PLACE = 4;       // bits of counters[SC_BAD]
constexpr uint32_t SC_NONE = 0xFFFFFFFFu;                                  // no choice (no partner: CHAIN_NONE, a memset of 0xFF)
constexpr uint8_t  SC_B_SUPPORTED = 1, SC_B_JOIN = 2, SC_B_DROPPED = 4;    // ALGA_SCAFFOLD_BUNDLE_* (bits of d_b_state)
constexpr uint8_t  SC_E_SUPPORTED = 1, SC_E_AMBIGUOUS = 2, SC_E_JOINED = 4; // ALGA_SCAFFOLD_END_* (bits of d_end_state)

// the placed reads: read r is node 2r + 1, its length len[2r + 1]
struct ScReads {
    const int32_t *len;
    int32_t stride;
    uint64_t R;
    const uint8_t *pair_off;          // 2R bytes, or null
    const int32_t *target, *pos;
    const uint8_t *state;
};
struct ScTargets {
    const uint32_t *col_off;          // T + 1
    uint32_t T;
};

// max_blocks: the cap of the launch's grid (8192, the check min(4096, max_blocks); option "scaffold_max_blocks")
// pair_off well formed (as the placement checks it), every UNIQUE read inside its target (as the polish checks it)
void launch_sc_check(const ScReads &r, const ScTargets &t, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// keys[r] = a << 32 | b of the link read r judges, `sentinel` (above every real key) for every other read; vals[r] = r; span[r]
void launch_sc_links(const ScReads &r, const ScTargets &t, int32_t max_insert, unsigned long long sentinel, unsigned long long *keys, uint32_t *vals, uint32_t *span,
                     unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// heads[i] = 1 where sorted key i differs from key i - 1; counters[SC_BUNDLES] += heads
void launch_sc_heads(const unsigned long long *keys, uint64_t n_links, uint32_t *heads, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// b_start[bundle] = its first link (b_start[n_bundles] = n_links), b_span[bundle] (zeroed) += the spans of its links
void launch_sc_bundle_fill(const uint32_t *vals, const uint32_t *span, const uint32_t *heads, const uint32_t *pos, uint64_t n_links, uint64_t n_bundles, uint32_t *b_start,
                           unsigned long long *b_span, uint32_t max_blocks, hipStream_t s);

struct ScBundles {
    uint64_t n;
    uint32_t *a, *b, *links;
    const unsigned long long *span;
    int32_t *gap;
    uint8_t *state;
};
struct ScParams { int32_t insert, min_links, max_second_percent, min_gap; };
// a, b, links, gap, SUPPORTED of every bundle; best[end] (zeroed) = max over its supported bundles of links << 32 | ~partner
void launch_sc_bundles(const unsigned long long *keys, const uint32_t *b_start, const ScBundles &b, const ScParams &p, unsigned long long *best, unsigned long long *counters,
                       uint32_t max_blocks, hipStream_t s);
// second[end] (zeroed) = the same maximum without the best
void launch_sc_second(const ScBundles &b, const unsigned long long *best, unsigned long long *second, uint32_t max_blocks, hipStream_t s);
// choice[end], end_state[end] (HAS_SUPPORTED, AMBIGUOUS)
void launch_sc_choice(const unsigned long long *best, const unsigned long long *second, uint64_t n_ends, int32_t max_second_percent, uint32_t *choice, uint8_t *end_state,
                      unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// JOIN of every bundle both of whose ends chose the other; partner[end] (0xFF-filled) and join_bundle[end] of the joined ends
void launch_sc_joins(const ScBundles &b, const uint32_t *choice, uint32_t *partner, uint32_t *join_bundle, uint32_t max_blocks, hipStream_t s);

// The joins into paths: the chain core (chain_kernels.h) with partner[] as its join[].  A state that still has a successor after the cycle phase
// lies on a cycle: the join at end 2c of its smallest contig c is dropped, DROPPED into its bundle's state
void launch_sc_cycle_drop(const ChainLists &l, uint32_t T, uint32_t *partner, const uint32_t *join_bundle, uint8_t *b_state, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// the rank phase's init: the weight of a state is its contig's length and the gap behind it
void launch_sc_rank_init(const ScTargets &t, const uint32_t *partner, const uint32_t *join_bundle, const int32_t *b_gap, int32_t min_gap, const ChainLists &l, uint32_t max_blocks, hipStream_t s);

struct ScLayout {
    int32_t *scaffold, *rank;
    uint8_t *orient;
    unsigned long long *start;
    int32_t *gap_after;
    uint32_t *join_links;
    uint32_t *s_off;
    int32_t *s_members;
    unsigned long long *s_len;
    uint8_t *end_state;
};
// per contig: rank, orientation, start, gap_after, join_links in the direction item 7 chooses; head[c] = the first contig of its scaffold,
// first[c] = 1 and members[c] = the scaffold's contigs where c is that contig, else 0 (T + 1 entries each, the last 0); JOINED of its two ends
void launch_sc_place(const ScTargets &t, const ChainLists &l, const uint32_t *partner, const uint32_t *join_bundle, const int32_t *b_gap, const uint32_t *b_links, int32_t min_gap,
                     const ScLayout &o, uint32_t *head, uint32_t *first, uint32_t *members, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// scaffold ids and member lists from the exclusive scans of first[] and members[] (T + 1 entries: the totals are entry T)
void launch_sc_layout(const ScTargets &t, const ChainLists &l, const uint32_t *head, const uint32_t *first_scan, const uint32_t *members_scan, const ScLayout &o,
                      unsigned long long *counters, uint32_t max_blocks, hipStream_t s);

// `>scaffold_id=<j>_length=<s_len>_contigs=<m>\n<sequence>\n`, one record per scaffold, the sequence from a column array
struct ScFasta {
    const uint32_t *words, *col_off;
    const uint32_t *s_off;
    const int32_t *s_members;
    const unsigned long long *s_len, *start;
    const uint8_t *orient;
    uint64_t n;
    uint32_t max_blocks;              // the cap of the write grid (16384; option "scaffold_max_blocks" lowers it)
};
void launch_sc_fasta_sizes(const ScFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_sc_fasta_write(const ScFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
