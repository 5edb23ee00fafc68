// alga_amd/csrc/mst_kernels.h -- launchers of mst_kernels.hip (removal of short parallel paths, include/alga_amd.h:
// alga_remove_short_parallel_paths_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mst_walk.h"

namespace alga {

// counters[] (unsigned long long) of a call
enum { MST_FLAGS = 0, MST_N_PEND0, MST_N_PEND1, MST_N_WIN, MST_N_OVF_CLAIM, MST_N_OVF_SELECT, MST_N_OVF_RUN, MST_N_OVF2_CLAIM, MST_N_OVF2_SELECT, MST_N_OVF2_RUN,
       MST_OVERFLOW_TOTAL, MST_BALL_MAX, MST_COUNTERS };
constexpr int MST_ROUND_COUNTERS = 7;                       // MST_N_WIN .. MST_N_OVF2_RUN: zeroed at the start of every round
// bits of counters[MST_FLAGS]
enum { MST_BAD_ID = 1, MST_BAD_OFFSET = 2, MST_BAD_ORDER = 4 };

// the short form's state, per wave in LDS: 256 map slots, 192 nodes, 256 collected edges
constexpr uint32_t MST_LDS_HBITS = 8, MST_LDS_NODES = 192, MST_LDS_EDGES = 256;

// what a round's kernels share.  owner[v]: (0xFFFFFFFF - round) << 32 | smallest claiming id -- a later round's claim is smaller than
// whatever an earlier round left, so the array is set once per call and never cleared
struct MstRound {
    MstGraph g;
    unsigned long long *owner;
    unsigned long long tag;       // (0xFFFFFFFF - round) << 32
    int32_t max_offset;
    int32_t *win, *pend_next;     // select: the winners / the losers that still branch
    int32_t *overflow, *overflow2; // the begs the short form of the phase at hand could not hold; those the first overflow tier could not hold either
    unsigned long long *counters;
    int next;                     // counters[MST_N_PEND0 + next] counts pend_next
};

// overflow route, two tiers of states in device workspaces, one thread per state, all words 0xFF on entry and on return:
//   mid  states of a fixed size (a few thousand nodes and edges): what the begs that LDS cannot hold need on read graphs, many of them
//   big  states sized for the whole graph (n + 1 nodes, m + 1 edges: they cannot fail), as many as a fixed budget allows, at least one;
//        n_big = 0 when a mid state already holds the whole graph
struct MstTier { uint32_t *ws; int32_t n_ws; uint32_t hbits, cap_nodes, cap_edges; };
struct MstTiers { MstTier mid, big; };
inline size_t mst_tier_words(const MstTier &t) { return 2 * ((size_t) 1 << t.hbits) + (size_t) t.cap_nodes + 3 * (size_t) t.cap_edges; }
// the smallest map that keeps `nodes` entries at most half full
uint32_t mst_hbits_for(uint64_t nodes);

// ids in [0, n), offsets >= 0, src non-decreasing -> counters[MST_FLAGS]; nothing else is written
void launch_mst_check(const alga_edge_dev *e, uint64_t m, int32_t n, unsigned long long *counters, hipStream_t s);
// len[v] = rowptr[v + 1] - rowptr[v], owner[v] = all ones, the nodes with >= 2 entries -> pend, counters[MST_N_PEND0]
void launch_mst_init(const uint32_t *rowptr, int32_t n, uint32_t *len, unsigned long long *owner, int32_t *pend, unsigned long long *counters, hipStream_t s);
// one wave per pending beg that still branches: its ball (mst_ball), every node of it claimed with atomicMin
void launch_mst_claim(const MstRound &r, const int32_t *pend, int cur, uint64_t n_pend, const MstTiers &t, hipStream_t s);
// the ball once more: a beg that holds all of it -> win, any other that still branches -> pend_next
void launch_mst_select(const MstRound &r, const int32_t *pend, int cur, uint64_t n_pend, const MstTiers &t, hipStream_t s);
// one wave per winner: the literal step (mst_run) on the live rows
void launch_mst_run(const MstRound &r, uint64_t n_win, const MstTiers &t, hipStream_t s);

}  // namespace alga
