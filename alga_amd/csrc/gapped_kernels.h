// alga_amd/csrc/gapped_kernels.h -- launchers of gapped_kernels.hip: the reads the Hamming placement left unplaced laid onto the same targets
// by edit distance, their CIGARs, their cover (include/alga_amd.h: alga_place_gapped_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seed_index.h"

namespace alga {

constexpr int GP_MAX_READ = 1024;    // ALGA_GAPPED_MAX_READ
constexpr int GP_MAX_EDITS = 15;     // the band has 2 E + 1 <= 31 diagonals: one half of a wave
constexpr int GP_MAX_RUNS = 2 * GP_MAX_EDITS + 1;   // words a participating read has in the CIGAR scratch

// counters[] (unsigned long long): the refusal flags and what the checks measure, then what the kernels count
enum { GP_BAD_TWIN = 0, GP_BAD_TARGETS, GP_INDEX_POS, GP_TRIED, GP_SKIPPED_LONG, GP_PLACED, GP_UNIQUE, GP_WITH_INDEL, GP_EDITS, GP_INSERTIONS, GP_DELETIONS,
       GP_CANDIDATES, GP_SEEDS, GP_SEEDS_OVER, GP_COUNTERS };

// the targets are the placement's: len[t] == col_off[t + 1] - col_off[t] >= 0 and col_off[T] == columns (GP_BAD_TARGETS otherwise); the indexed
// positions sum of max(0, len - k + 1) (GP_INDEX_POS)
void launch_gp_target_check(const int32_t *tlen, const uint32_t *col_off, uint64_t T, uint64_t columns, int32_t k, unsigned long long *counters, hipStream_t s);
// flag[r] = read r takes part (flag[R] = 0); GP_TRIED, GP_SKIPPED_LONG
void launch_gp_flag(const SeedReads &r, const uint8_t *pl_state, int32_t k, uint32_t *flag, unsigned long long *counters, hipStream_t s);
// list[pos[r]] = r where flag[r]
void launch_gp_scatter(const uint32_t *flag, const uint32_t *pos, uint64_t R, uint32_t *list, hipStream_t s);

struct GpOut {
    int32_t *target, *pos, *end;
    uint8_t *edits, *state;
};
// one wave per participating read, both strands; best[i] = the key of the best candidate of list[i] (all ones: none)
void launch_gp_score(const SeedReads &r, const SeedSpace &t, const SeedIndex &x, int32_t k, int32_t E, int32_t max_occ, const uint32_t *list, uint64_t n_list, const GpOut &o,
                     unsigned long long *best, int blocks, unsigned long long *counters, hipStream_t s);
// one wave per participating read that is placed: its script as runs (len << 2 | op) in runs[i * GP_MAX_RUNS ..], their number in n_runs[list[i]] (zeroed)
void launch_gp_trace(const SeedReads &r, const SeedSpace &t, int32_t k, int32_t E, const uint32_t *list, uint64_t n_list, const unsigned long long *best, uint8_t *state,
                     uint32_t *runs, uint32_t *n_runs, unsigned long long *counters, hipStream_t s);
// cigar[cigar_off[list[i]] ..] = the runs of list[i]
void launch_gp_cigar(const uint32_t *list, uint64_t n_list, const uint32_t *runs, const uint32_t *cigar_off, uint32_t *cigar, hipStream_t s);
// +1 / -1 of every UNIQUE gapped read into diff[] (columns + 1 entries, zeroed), the per-target sums into tstat[3][T] (reads, bases, edits)
void launch_gp_depth_add(const SeedSpace &t, const uint32_t *list, uint64_t n_list, const GpOut &o, uint32_t *diff, unsigned long long *tstat, hipStream_t s);
// cover[g] = pl_cover[g] + scan[g + 1]
void launch_gp_cover(const uint32_t *pl_cover, const uint32_t *scan, uint64_t columns, uint32_t *cover, hipStream_t s);

// the TSV: one line per gapped-placed read
struct GpTsv {
    const int32_t *target, *pos, *end;
    const uint8_t *edits, *state;
    const uint32_t *cigar_off, *cigar;
    uint64_t n;
};
void launch_gp_tsv_sizes(const GpTsv &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_gp_tsv_write(const GpTsv &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
