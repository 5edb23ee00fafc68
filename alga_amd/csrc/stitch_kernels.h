// alga_amd/csrc/stitch_kernels.h -- launchers of stitch_kernels.hip: scaffold joins whose contig ends overlap stitched into one sequence
// (include/alga_amd.h: alga_stitch_targets_device).  Everything behind the overlap decision is the merge stage's (merge_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "merge_kernels.h"

namespace alga {

// counters[] (unsigned long long): the merge stage's (its launchers count into them), then the stitch stage's own
enum { ST_BAD = MG_COUNTERS, ST_SELECTED, ST_WITH_OVERLAP, ST_AMBIGUOUS, ST_SATURATED, ST_OUTSIDE_SLACK, ST_COUNTERS };
constexpr uint32_t ST_BAD_END = 1, ST_BAD_SAME_TARGET = 2, ST_BAD_END_TWICE = 4;                       // bits of counters[ST_BAD]
constexpr uint8_t  ST_J_SELECTED = 1, ST_J_HAS_OVERLAP = 2, ST_J_AMBIGUOUS = 4, ST_J_STITCHED = 8, ST_J_DROPPED_CYCLE = 16;   // ALGA_STITCH_* of include/alga_amd.h
constexpr int32_t  ST_MAX_OVERLAP = 4096;

// the entry list: ends a and b (x = 2t left, 2t + 1 right), the estimated gap, the state (NULL: every entry is selected)
struct StEntries {
    const uint32_t *a, *b;
    const int32_t *gap;
    const uint8_t *state;
    uint32_t J;
};
struct StParams {
    int32_t max_mm, min_overlap, max_overlap, slack;
};
struct StEntryOut {
    int32_t *olen;
    uint8_t *mm, *hits, *state;
};

// begin[t] = col_off[t], len[t] = col_off[t + 1] - col_off[t]: a placement's targets as a ragged target set
void launch_st_targets(const uint32_t *col_off, uint32_t T, unsigned long long *begin, int32_t *len, uint32_t max_blocks, hipStream_t s);
// the refusals of the selected entries -> counters[ST_BAD]; counters[ST_SELECTED]; end_count[x] += 1 and end_entry[x] = j for both ends of a
// selected entry that is in range (end_count zeroed, end_entry filled with -1 by the caller; 2T entries each)
void launch_st_check(const StEntries &en, uint32_t T, uint32_t *end_count, int32_t *end_entry, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);
// one wave per selected entry: every overlap length compared, the entry's olen / mm / hits / state
void launch_st_overlap(const MgTargets &t, const StEntries &en, const StParams &p, const StEntryOut &o, unsigned long long *counters, hipStream_t s);
// one thread per end: the stitched entry that names it scattered into the per-end arrays the merge stage's launchers take
void launch_st_joins(const StEntries &en, const StEntryOut &o, const int32_t *end_entry, uint32_t E, const MgEndOut &eo, uint32_t *join, uint32_t max_blocks, hipStream_t s);
// (after the cycles) one thread per entry: a stitched entry whose join was dropped loses STITCHED and gets DROPPED_CYCLE
void launch_st_dropped(const StEntries &en, const uint32_t *join, uint8_t *state, uint32_t max_blocks, hipStream_t s);

}  // namespace alga
