// alga_amd/csrc/ipolish_kernels.h -- launchers of ipolish_kernels.hip: the placed targets voted by the Hamming-placed and the gapped reads together,
// columns that change or leave, strings that enter between two columns (include/alga_amd.h: alga_polish_indels_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

constexpr int IP_MAX_RUNS = 31;      // runs a G voter's script may have
constexpr int IP_MAX_INS = 13;       // the longest string that votes: 2 * 13 bits below the length in a 30-bit key

// counters[] (unsigned long long): the refusal flags and what the check measures, then what the vote, the decision and the build count
enum { IP_BAD_TWIN = 0, IP_BAD, IP_VOTERS_G, IP_VOTES_G, IP_DEL_VOTES, IP_INS_VOTES, IP_INS_LONG, IP_INS_EDGE, IP_SHIFTED_RUNS, IP_SHIFTED_BASES, IP_INS_CURSOR,
       IP_VOTED, IP_SUBST, IP_DELETED, IP_INS_SLOTS, IP_INS_BASES, IP_AMB_COLS, IP_AMB_SLOTS, IP_MAX_COVER, IP_LONGEST, IP_COUNTERS };
constexpr uint32_t IP_BAD_READ_LEN = 1, IP_BAD_COL_LEN = 2, IP_BAD_PLACE = 4, IP_BAD_RUNS = 8;     // bits of counters[IP_BAD]

// bits of code[g], the verdict on old column g and on the slot before it
constexpr uint32_t IP_C_BASE = 3, IP_C_DELETED = 4, IP_C_SUBST = 8, IP_C_INSERTED = 16, IP_C_AMB_COL = 32, IP_C_AMB_SLOT = 64;

// the G voters: read r votes iff state[r] & ALGA_GAPPED_UNIQUE, as node 2r (MINUS) or 2r + 1, by its script from column col_off[target[r]] + pos[r] on
struct IpReads {
    const uint32_t *rows;
    int32_t stride;
    const int32_t *len;
    uint64_t R;
    const int32_t *target, *pos, *end;
    const uint8_t *state;
    const uint32_t *cigar_off, *cigar;
    uint64_t n_cigar;
};
struct IpTargets {
    const uint32_t *col_off;          // T + 1
    uint32_t T;
    uint64_t columns;
    const uint32_t *cols;             // the placement's column array: `cur`
    uint32_t max_blocks;              // the cap of every grid here (8192; option "ipolish_max_blocks")
};

// rule 8 on every G voter, and what its normalised script will vote (so that the insertion keys are allocated at their number)
void launch_ip_check(const IpReads &r, const IpTargets &t, int32_t max_ins, unsigned long long *counters, hipStream_t s);
// the votes of the G voters on top of the H voters' counts: counts4[4 g + b] and del[g] by atomic adds, an insertion key (n << 26 | string, slot) per
// inner I run of at most max_ins bases at the place counters[IP_INS_CURSOR] gives, long_ins into ins_all[slot]
void launch_ip_vote_gapped(const IpReads &r, const IpTargets &t, int32_t max_ins, uint32_t *counts4, uint32_t *del, unsigned long long *ins_key, unsigned long long *ins_slot,
                           uint32_t *ins_all, unsigned long long *counters, hipStream_t s);
// +1 at p + 1, -1 at e of every voter [p, e), H (pl_*: state & ALGA_PLACE_UNIQUE) and G, into diff[] (columns + 1 entries, zeroed)
void launch_ip_span(const IpReads &r, const IpTargets &t, const int32_t *pl_target, const int32_t *pl_pos, const uint8_t *pl_state, uint32_t *diff, hipStream_t s);
// over the n insertion votes sorted by (slot, key): the winner of every slot into win_key / win_votes, all its votes added to ins_all
void launch_ip_ins_pick(const unsigned long long *slot, const unsigned long long *key, uint64_t n, uint32_t *win_key, uint32_t *win_votes, uint32_t *ins_all, uint32_t max_blocks,
                        hipStream_t s);

struct IpDecide {
    const uint32_t *counts4, *del;    // 4 per column; 1 per column
    const uint32_t *span_scan;        // the exclusive scan of diff: entry c + 1 is span[c]
    const uint32_t *win_key, *win_votes, *ins_all;
    int32_t min_cover, min_percent;
    uint32_t *width, *evn;            // out, columns + 1 entries (the last 0): new columns of the old column with its slot; its events
    uint8_t *code;                    // out
    uint32_t *counts5, *span;         // out or null
    unsigned long long *t_subs, *t_dels, *t_ins, *t_amb;
};
void launch_ip_decide(const IpTargets &t, const IpDecide &d, unsigned long long *counters, hipStream_t s);

struct IpBuild {
    const uint32_t *new_col;          // columns + 1: the exclusive scan of width
    const uint32_t *ev_off;           // columns + 1: the exclusive scan of evn
    const uint8_t *code;
    const uint32_t *counts4, *del, *span_scan, *win_key, *win_votes;
    uint64_t new_columns;
};
// every word of the new column array, one lane a word (the two padding words included)
void launch_ip_words(const IpTargets &t, const IpBuild &b, uint32_t *words, hipStream_t s);
struct IpEvents {
    uint32_t *col; uint8_t *kind, *len; uint32_t *bases, *votes, *cover;
};
void launch_ip_events(const IpTargets &t, const IpBuild &b, const IpEvents &ev, hipStream_t s);
// the new col_off (T + 1), len and begin of every target; counters[IP_LONGEST]
void launch_ip_targets(const IpTargets &t, const uint32_t *new_col, uint32_t *col_off, int32_t *len, unsigned long long *begin, unsigned long long *counters, hipStream_t s);

// the FASTA of the new targets and the TSV of the events
struct IpFasta {
    const uint32_t *words, *col_off;
    const int32_t *len;
    const unsigned long long *t_subs, *t_ins, *t_dels;
    uint64_t n;
};
void launch_ip_fasta_sizes(const IpFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_ip_fasta_write(const IpFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);
struct IpTsv {
    const uint32_t *old_col_off;      // the col_off of the targets that were polished
    uint32_t T;
    const uint32_t *col; const uint8_t *kind, *len; const uint32_t *bases, *votes, *cover;
    uint64_t n;
};
void launch_ip_tsv_sizes(const IpTsv &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s);
void launch_ip_tsv_write(const IpTsv &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
