// alga_amd/csrc/polish_kernels.h -- launchers of polish_kernels.hip: the placed targets re-voted by every placed read (include/alga_amd.h:
// alga_polish_placed_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

// counters[] (unsigned long long): the refusal flag and what the check measures, then what the vote counts
enum { PO_BAD = 0, PO_VOTERS, PO_VOTES, PO_MAX_LEN, PO_VOTED, PO_CHANGED, PO_AMBIGUOUS, PO_MAX_COVER, PO_WIDE, PO_COUNTERS };
constexpr uint32_t PO_BAD_LEN = 1, PO_BAD_PLACE = 2, PO_BAD_COLUMNS = 4;    // bits of counters[PO_BAD]
constexpr uint32_t PO_NARROW_DEPTH = 255;                                   // covering voters the bit-sliced counters of k_po_vote hold
constexpr uint32_t PO_WIDE_MARK = 0xFFFFFFFFu;                              // pop[w] between the two vote kernels: the word is left to k_po_vote_wide

// the voters: read r votes iff state[r] & vote_bit, as node 2r (MINUS) or 2r + 1, from column col_off[target[r]] + pos[r] on
struct PoReads {
    const uint32_t *rows;
    int32_t stride;
    const int32_t *len;
    uint64_t R;
    const int32_t *target, *pos;
    const uint8_t *state;
    uint8_t vote_bit;
};
struct PoTargets {
    const uint32_t *col_off;          // T + 1
    uint32_t T;
    uint64_t columns;
    const uint32_t *cols;             // the placement's column array: `cur`
};

// the refusals (counters[PO_BAD]), the voters, the sum of their lengths and the longest
void launch_po_check(const PoReads &r, const PoTargets &t, unsigned long long *counters, hipStream_t s);
// keys[r] = the voter's first column, 0xFFFFFFFF for a read that does not vote; vals[r] = its voting node
void launch_po_keys(const PoReads &r, const PoTargets &t, uint32_t *keys, uint32_t *vals, hipStream_t s);

struct PoVote {
    const uint32_t *keys, *vals;      // sorted by key; the first n_voters are voters
    uint32_t n_voters, longest;
    int32_t min_cover, min_percent;
    uint32_t *words;                  // out: the polished column array
    uint32_t *marks;                  // out: changed mask | ambiguous mask << 16
    uint32_t *pop;                    // out: changed columns of the word (PO_WIDE_MARK between the two vote kernels)
    uint32_t *counts;                 // out or null: 4 per column
    unsigned long long *t_changed, *t_ambiguous;
};
void launch_po_vote(const PoReads &r, const PoTargets &t, const PoVote &v, unsigned long long *counters, hipStream_t s);
void launch_po_vote_wide(const PoReads &r, const PoTargets &t, const PoVote &v, unsigned long long *counters, hipStream_t s);
// the change list from the masks and the exclusive scan of pop[]: ascending columns, bases old | new << 2
void launch_po_changes(const PoTargets &t, const uint32_t *words, const uint32_t *marks, const uint32_t *pos, uint32_t *cols_out, uint8_t *bases_out, hipStream_t s);

// the FASTA of a final result with the sequences of a polished column array: record j = target j, header with or without the depth
struct PoFasta {
    const uint32_t *words, *col_off;
    const uint8_t *verdict;
    const int32_t *order;
    const unsigned long long *t_reads, *t_bases;
    uint64_t n;
    int32_t depth;
};
void launch_po_fasta_sizes(const PoFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_po_fasta_write(const PoFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
