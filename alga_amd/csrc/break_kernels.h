// alga_amd/csrc/break_kernels.h -- launchers of break_kernels.hip: contigs broken where no proper pair spans them
// (include/alga_amd.h: alga_break_placed_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

// counters[] (unsigned long long): the refusal flags, then what the kernels count
enum { BR_BAD = 0, BR_PROPER, BR_SPANNING, BR_CANDIDATES, BR_WEAK, BR_RUNS, BR_CUTS, BR_TARGETS_CUT, BR_MAX_SPAN, BR_LONGEST, BR_COUNTERS };
constexpr uint32_t BR_BAD_PAIR = 1, BR_BAD_LEN = 2, BR_BAD_PLACE = 4, BR_BAD_COLUMNS = 8;   // bits of counters[BR_BAD]
// marks[g] of a column: a run starts / ends here; the column before the start / behind the end is a candidate of the same target
constexpr uint8_t  BR_M_START = 1, BR_M_END = 2, BR_M_LEFT = 4, BR_M_RIGHT = 8;

// the placed reads: read r is node 2r + 1, its length len[2r + 1]
struct BrReads {
    const int32_t *len;
    int32_t stride;
    uint64_t R;
    const uint8_t *pair_off;          // 2R bytes, or null
    const int32_t *target, *pos;
    const uint8_t *state;
};
struct BrTargets {
    const uint32_t *col_off;          // T + 1
    uint32_t T;
    uint64_t columns;                 // col_off[T]
};

// pair_off well formed (as the placement checks it), every UNIQUE read inside its target (as the polish checks a voter), columns == col_off[T]
void launch_br_check(const BrReads &r, const BrTargets &t, unsigned long long *counters, hipStream_t s);
// the judging mate of every proper pair: diff[first spanned column] += 1, diff[behind the last] -= 1 (columns + 1 zeroed entries)
void launch_br_pairs(const BrReads &r, const BrTargets &t, int32_t max_insert, int32_t inset, uint32_t *diff, unsigned long long *counters, hipStream_t s);
// per column: starts[g] = 1 where a run starts (columns + 1 entries, the last 0), marks[g]; the counters of the columns and runs
void launch_br_flags(const BrTargets &t, const uint32_t *span, uint32_t min_span, uint32_t margin, uint32_t *starts, uint8_t *marks, unsigned long long *counters,
                     hipStream_t s);
// run i (the i-th start, the i-th end: run_pos is the exclusive scan of starts): its first and last column
void launch_br_runs(const BrTargets &t, const uint32_t *run_pos, const uint8_t *marks, uint64_t n_runs, uint32_t *run_first, uint32_t *run_last, hipStream_t s);
// closed[i] = both neighbours of run i are candidates (n_runs + 1 entries, the last 0); counters[BR_CUTS] += closed
void launch_br_closed(const uint32_t *run_first, const uint32_t *run_last, const uint8_t *marks, uint64_t n_runs, uint32_t *closed, unsigned long long *counters,
                      hipStream_t s);

struct BrCuts {
    uint64_t n;
    uint32_t *cols, *first, *last;    // n
    uint32_t *t_cuts;                 // T (zeroed)
};
// every closed run at the place the scan of closed[] gives: the cut column, the run; t_cuts[its target]++
void launch_br_cuts(const BrTargets &t, const uint32_t *run_first, const uint32_t *run_last, const uint32_t *closed, const uint32_t *cut_pos, uint64_t n_runs, const BrCuts &c,
                    hipStream_t s);

struct BrPieces {
    uint32_t *piece_off;              // n_pieces + 1
    unsigned long long *begin;        // n_pieces
    int32_t *len;
    int32_t *piece_target;
    uint32_t *piece_start;
};
// T + n_cuts items: target starts and cuts find their piece id by bisection over the other list
void launch_br_pieces(const BrTargets &t, const BrCuts &c, const BrPieces &p, unsigned long long *counters, hipStream_t s);
// the column array copied, the bits past the last column zero
void launch_br_copy(const uint32_t *src, uint64_t columns, uint32_t *dst, hipStream_t s);

// `>contig_id=<j>_length=<len>_from=<t>_start=<s>\n<piece>\n`, one record per piece with a length
struct BrFasta {
    const uint32_t *words, *piece_off;
    const int32_t *len, *piece_target;
    const uint32_t *piece_start;
    uint64_t n;
};
void launch_br_fasta_sizes(const BrFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_br_fasta_write(const BrFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
