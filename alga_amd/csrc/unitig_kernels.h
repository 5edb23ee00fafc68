// alga_amd/csrc/unitig_kernels.h -- launchers of unitig_kernels.hip (the unitig graph of include/alga_amd.h: alga_unitigs_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "prefsuf_kernels.h"

namespace alga {

// counters[] (unsigned long long) the unitig kernels fill (behind them: one count of unresolved nodes per jump round)
enum { UT_FLAGS = 0, UT_TWINS_ADDED, UT_CYCLES, UT_ISOLATED, UT_LONGEST_NODES, UT_LONGEST_BASES, UT_TOTAL_BASES,
       UT_TOTAL_NODES, UT_OVERFLOW, UT_COUNTERS };
// bits of counters[UT_FLAGS]
enum { UT_BAD_ID = 1, UT_BAD_DEAD = 2, UT_BAD_DOVETAIL = 4, UT_BAD_TWIN_LEN = 8, UT_BAD_LEN = 16 };

// one node of the list ranking: the ancestor reached so far (towards the head), the number of path edges and of bases up to it,
// done != 0: `up` is the head of the path and rank / pos are final
struct __attribute__((aligned(16))) UtRank { int32_t up, rank, pos, done; };
// ... of the search for the smallest pair of a cycle
struct __attribute__((aligned(8))) UtMin { int32_t up, min_pair; };

// step 1: node and edge checks -> counters[UT_FLAGS]; nothing else is written
void launch_ut_check(const int32_t *len, int32_t n, const alga_edge_dev *e, uint64_t m, unsigned long long *counters, hipStream_t s);
// step 2: keys[i] = (src << 32 | dst), vals[i] = offset << 1 | is_twin for the m edges (i < m) and their twins (m + i)
void launch_ut_twins(const int32_t *len, const alga_edge_dev *e, uint64_t m, unsigned long long *keys, uint32_t *vals, hipStream_t s);
// the sorted 2 m records: flag[i] = first of its (src, dst); best[i] (at a first) = the smallest offset of the group
void launch_ut_group_heads(const unsigned long long *keys, const uint32_t *vals, uint64_t m2, uint32_t *flag, uint32_t *best,
                           unsigned long long *counters, hipStream_t s);
void launch_ut_compact_edges(const unsigned long long *keys, const uint32_t *flag, const uint32_t *pos, const uint32_t *best, uint64_t m2,
                             alga_edge_dev *estar, hipStream_t s);
// step 3: nxt[v] / noff[v] = the compactable edge out of v (-1: none); prv[] through the twin identity in a second pass
void launch_ut_next(const alga_edge_dev *estar, const uint32_t *rowptr, int32_t n, int32_t *nxt, int32_t *noff, hipStream_t s);
void launch_ut_prev(const int32_t *nxt, int32_t n, int32_t *prv, hipStream_t s);
// list ranking: records of the nodes with only_unresolved == 0 or done == 0 from prv / noff; one jump round a -> b (counts the unresolved)
void launch_ut_rank_init(const int32_t *len, const int32_t *prv, const int32_t *noff, int32_t n, int only_unresolved, UtRank *a, hipStream_t s);
void launch_ut_rank_jump(const UtRank *a, UtRank *b, int32_t n, unsigned long long *counters, hipStream_t s);
// ruling set (an accelerator of the ranking; what it leaves unresolved -- cycles -- the jump rounds finish): flag[v] = v is a ruler (a head, or
// sampled: one id in 64); link[v] = (next, offset); the rulers' list and the heads' records; walk 1: every ruler to the next one, which gets
// (index of this ruler, steps, bases, 0); walk 2: every ranked ruler writes the final records of the nodes up to the next ruler into a[]
void launch_ut_ruler_flags(const int32_t *len, const int32_t *prv, int32_t n, uint32_t *flag, hipStream_t s);
void launch_ut_links(const int32_t *nxt, const int32_t *noff, int32_t n, int2 *link, hipStream_t s);
void launch_ut_ruler_list(const uint32_t *flag, const uint32_t *ridx, const int32_t *prv, int32_t n, int32_t *rnode, UtRank *rrec, hipStream_t s);
void launch_ut_ruler_walk1(const int2 *link, const int32_t *rnode, const uint32_t *ridx, uint32_t R, UtRank *rrec, hipStream_t s);
void launch_ut_ruler_walk2(const int2 *link, const int32_t *rnode, const UtRank *rrec, uint32_t R, UtRank *a, hipStream_t s);
// step 4: the smallest pair of every cycle (unresolved nodes), then the two cuts
void launch_ut_min_init(const UtRank *r, const int32_t *prv, int32_t n, UtMin *a, hipStream_t s);
void launch_ut_min_jump(const UtRank *r, const UtMin *a, UtMin *b, int32_t n, hipStream_t s);
void launch_ut_cut(const UtRank *r, const UtMin *a, int32_t n, int32_t *nxt, int32_t *prv, unsigned long long *counters, hipStream_t s);
// steps 5-6: tail_of[head] = the path's last node; win[v] = 1 for the head of a `+` orientation that is kept
void launch_ut_tails(const UtRank *r, const int32_t *len, const int32_t *nxt, int32_t n, int32_t *tail_of, hipStream_t s);
void launch_ut_winners(const UtRank *r, const int32_t *len, const int32_t *prv, const int32_t *tail_of, const uint32_t *rowptr, int32_t n, int skip_isolated,
                       uint32_t *win, unsigned long long *counters, hipStream_t s);
// per pair: node count, length in bases (ulen2: the same per oriented unitig id), words of the packed sequence
void launch_ut_pair_sizes(const UtRank *r, const int32_t *len, const int32_t *tail_of, const uint32_t *win, const uint32_t *pair_of, int32_t n,
                          uint32_t *cnt, int32_t *ulen, int32_t *ulen2, uint32_t *uwords, unsigned long long *counters, hipStream_t s);
// step 7: the path arrays of the `+` orientations; uid[v] = the oriented unitig of v (-1: left out)
void launch_ut_layout(const UtRank *r, const int32_t *len, const int32_t *tail_of, const uint32_t *win, const uint32_t *pair_of,
                      const unsigned long long *path_off, int32_t n, int32_t *path_node, int32_t *path_pos, int32_t *uid, hipStream_t s);
// step 8: one lane per output word
void launch_ut_sequence(const uint32_t *words, int32_t stride, const int32_t *path_node, const int32_t *path_pos,
                        const unsigned long long *path_off, const unsigned long long *word_off, const int32_t *ulen, uint32_t n_pairs,
                        uint64_t n_words, uint32_t *out, hipStream_t s);
// step 9: flag[i] = edge i of E* is not compactable; then the flagged ones as unitig edges in (key, value) form for the edge sort
void launch_ut_edge_flags(const alga_edge_dev *estar, uint64_t ms, const int32_t *nxt, uint32_t *flag, hipStream_t s);
void launch_ut_edges(const alga_edge_dev *estar, uint64_t ms, const uint32_t *flag, const uint32_t *pos, const int32_t *uid, const UtRank *r,
                     unsigned long long *keys, uint32_t *vals, hipStream_t s);

}  // namespace alga
