// alga_amd/csrc/merge_kernels.h -- launchers of merge_kernels.hip: contigs whose ends overlap merged into one sequence
// (include/alga_amd.h: alga_merge_targets_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "chain_kernels.h"
#include "seed_index.h"

namespace alga {

// counters[] (unsigned long long): the refusal flags and the sizes, then what the kernels count
enum { MG_BAD = 0, MG_COLUMNS, MG_END_COLUMNS, MG_INDEX_POS, MG_ENDS, MG_SEEDS, MG_SEEDS_OVER, MG_WITH_OVERLAP, MG_AMBIGUOUS, MG_SATURATED, MG_JOINS, MG_DROPPED, MG_JOIN_MM,
       MG_REMOVED, MG_LONGEST_OVERLAP, MG_MERGED, MG_MULTI, MG_MEMBERS, MG_LONGEST, MG_COLUMNS_AFTER, MG_BAD_MERGED_LEN, MG_COUNTERS };
constexpr uint32_t MG_BAD_LEN = 1;                                       // bit of counters[MG_BAD]
constexpr uint8_t  MG_E_HAS_OVERLAP = 1, MG_E_AMBIGUOUS = 2, MG_E_JOINED = 4, MG_E_DROPPED_CYCLE = 8;   // ALGA_MERGE_END_* of include/alga_amd.h
constexpr int32_t  MG_MAX_OVERLAP = 4096;

// a ragged target set as the placement takes it
struct MgTargets {
    const uint32_t *words;
    const unsigned long long *begin;  // T: base index of the first base
    const int32_t *len;               // T
    uint32_t T;
    uint32_t max_blocks;              // the cap of every grid here but k_mg_overlap's and the FASTA kernels' (8192; option "merge_max_blocks")
};
// the 2T end sequences in a column space of their own, the space their index is built over (alga_seed_index): end x is the columns
// off[x] .. off[x] + len[x] (len[x] = W_x), off[x] a multiple of 16; cols holds E_x, the contig end at the right; n = 2T
struct MgEnds : SeedSpace {
    const uint32_t *pcols;            // P_x = the reverse complement of E_x, at the same columns
};
struct MgEndOut {
    int32_t *partner, *olen;
    uint8_t *mm, *hits, *state;
};
struct MgLayout {
    int32_t *merged, *rank;
    uint8_t *orient;
    uint32_t *start;
    int32_t *overlap_after;
    uint32_t *m_off;                  // n_merged + 1
    int32_t *m_members;               // n_members
    int32_t *m_len;                   // n_merged (+ 1: a 0 for the scan)
};

// a negative length -> counters[MG_BAD]; counters[MG_COLUMNS] += len
void launch_mg_check(const MgTargets &t, unsigned long long *counters, hipStream_t s);
// elen[x] = W_x, epad[x] = W_x rounded up to 16 (2T + 1 entries each, the last 0); counters[MG_END_COLUMNS], [MG_INDEX_POS], [MG_ENDS]
void launch_mg_end_lens(const MgTargets &t, int32_t max_overlap, int32_t min_overlap, int32_t k, int32_t *elen, uint32_t *epad, unsigned long long *counters, hipStream_t s);
// E_x and P_x, one thread per word: the left ends complemented and mirrored
void launch_mg_ends(const MgTargets &t, const MgEnds &e, uint32_t *ecols, uint32_t *pcols, hipStream_t s);
// one wave per end (blocks: seed_blocks(2T))
void launch_mg_overlap(const MgEnds &e, const SeedIndex &x, int32_t k, int32_t max_mm, int32_t max_occ, int32_t min_overlap, const MgEndOut &o, int blocks,
                       unsigned long long *counters, hipStream_t s);
// one thread per end: join[x] = the end x is joined with, CHAIN_NONE without; JOINED into the end's state
void launch_mg_joins(const MgEndOut &o, uint32_t E, uint32_t *join, uint32_t max_blocks, hipStream_t s);
// The joins into paths: the chain core (chain_kernels.h).  A state that still has a successor after the cycle phase lies on a cycle: the join at
// end 2c of its smallest contig c is dropped, both ends lose JOINED and get DROPPED_CYCLE
void launch_mg_cycle_drop(const ChainLists &l, uint32_t T, uint32_t *join, uint8_t *end_state, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// the rank phase's init: the weight of a state is len - overlap at the end it is left at
void launch_mg_rank_init(const MgTargets &t, const uint32_t *join, const int32_t *olen, const ChainLists &l, hipStream_t s);
// per contig: rank, orientation, start, overlap_after; head / first / members (T + 1 entries of the last two) for the scans; the join counters
void launch_mg_place(const MgTargets &t, const ChainLists &l, const uint32_t *join, const MgEndOut &o, const MgLayout &lo, uint32_t *head, uint32_t *first, uint32_t *members,
                     unsigned long long *counters, hipStream_t s);
// merged ids, the member lists, the merged lengths; counters[MG_MERGED], [MG_MULTI], [MG_MEMBERS], [MG_LONGEST], [MG_COLUMNS_AFTER], [MG_BAD_MERGED_LEN]
void launch_mg_layout(const MgTargets &t, const ChainLists &l, const uint32_t *head, const uint32_t *first_scan, const uint32_t *members_scan, const MgLayout &lo,
                      unsigned long long *counters, hipStream_t s);
// the merged contigs' column array, one thread per word; begin[j] = col_off[j]
void launch_mg_build(const MgTargets &t, const MgLayout &lo, const uint32_t *col_off, uint32_t n_merged, uint64_t columns, uint32_t *words, unsigned long long *begin,
                     hipStream_t s);

// `>contig_id=<j>_length=<len>_contigs=<m>\n<merged contig>\n`, one record per merged contig
struct MgFasta {
    const uint32_t *words, *col_off, *m_off;
    const int32_t *len;
    uint64_t n;
};
void launch_mg_fasta_sizes(const MgFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_mg_fasta_write(const MgFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga

// engine_merge.hip, shared with engine_stitch.hip: from the joins (w.join and the per-end arrays, as k_mg_joins leaves them) to the built sequences:
// cycles, drop, `after_drop` where the caller has a step there, ranks, places, scans, layout, the read-back of n_counters words of cnt into
// e->h_counters with the refusal of a contig above 2^31 - 1, `words` at its size, the length scan, the build.  stage / noun word the refusal.
struct DevBuf;
int alga_merge_tail(alga_engine *e, const alga::MgTargets &tg, const alga::MgEndOut &eo, const alga::ChainWork &w, const alga::MgLayout &lo, uint32_t *col_off, DevBuf &words,
                    unsigned long long *begin, unsigned long long *cnt, size_t n_counters, const char *stage, const char *noun, const std::function<int()> &after_drop,
                    hipStream_t s);
