// alga_amd/csrc/tip_kernels.h -- launchers of tip_kernels.hip (dangling-branch removal, include/alga_amd.h: alga_remove_dangling_branches_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tip_walk.h"

namespace alga {

// counters[] (unsigned long long) of a call
enum { TIP_FLAGS = 0, TIP_N_BRANCH, TIP_N_OVERFLOW, TIP_BRANCH_TOTAL, TIP_OVERFLOW_TOTAL, TIP_DOWN, TIP_UP, TIP_COUNTERS };
// bits of counters[TIP_FLAGS]
enum { TIP_BAD_ID = 1, TIP_BAD_OFFSET = 2 };

// one CSR direction of the graph: edges sorted by (row, neighbour), row pointers, forward edge id of every slot (NULL: forward direction)
struct TipDir { const alga_edge_dev *E; const uint32_t *rowptr; const uint32_t *fid; };

// ids in [0, n) and offsets >= 0 -> counters[TIP_FLAGS]; nothing else is written
void launch_tip_check(const alga_edge_dev *e, uint64_t m, int32_t n, unsigned long long *counters, hipStream_t s);
// keys[i] = src << 32 | dst, vals[i] = offset << 1 (the form k_ut_group_heads reduces per (src, dst))
void launch_tip_keys(const alga_edge_dev *e, uint64_t m, unsigned long long *keys, uint32_t *vals, hipStream_t s);
// the unique sorted edges: keys[i] = dst << 32 | src, vals[i] = i -> (sorted) -> the reverse CSR's edges and their forward ids
void launch_tip_rev_keys(const alga_edge_dev *est, uint64_t ms, unsigned long long *keys, uint32_t *vals, hipStream_t s);
void launch_tip_rev_edges(const unsigned long long *keys, const uint32_t *vals, const alga_edge_dev *est, uint64_t ms, alga_edge_dev *rev, uint32_t *rfid,
                          hipStream_t s);
// per pass: the records of both directions from the live edges; the nodes with >= 2 live edges in direction `dir` -> branch[], counters[TIP_N_BRANCH]
void launch_tip_degrees(const TipDir &fwd, const TipDir &rev, const uint8_t *alive, int32_t n, int dir, TipRec *frec, TipRec *rrec, int32_t *branch,
                        unsigned long long *counters, hipStream_t s);
// one thread per branching node (tip_walk_junction): kill[] of the edges to go; those it cannot hold -> overflow[], counters[TIP_N_OVERFLOW]
void launch_tip_find(const TipGraph &g, const int32_t *branch, int32_t n, int32_t max_offset, uint8_t *kill, int32_t *overflow, unsigned long long *counters,
                     hipStream_t s);
// the overflow list, one thread per workspace (tip_walk_full): ws = n_ws x 5 x n words, the first n of each -1
void launch_tip_find_overflow(const TipGraph &g, const int32_t *overflow, int32_t max_offset, uint8_t *kill, int32_t *ws, int32_t n, int32_t n_ws,
                              unsigned long long *counters, hipStream_t s);
// alive &= ~kill, kill = 0; the number of edges that went -> *removed
void launch_tip_apply(uint8_t *alive, uint8_t *kill, uint64_t ms, unsigned long long *removed, hipStream_t s);
// flag[i] = alive[i] -> (scan) -> the surviving edges in order
void launch_tip_flags(const uint8_t *alive, uint64_t ms, uint32_t *flag, hipStream_t s);
void launch_tip_emit(const alga_edge_dev *est, const uint32_t *flag, const uint32_t *pos, uint64_t ms, alga_edge_dev *out, hipStream_t s);

}  // namespace alga
