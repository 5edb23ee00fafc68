// alga_amd/csrc/contig_kernels.h -- launchers of contig_kernels.hip (the contigs of include/alga_amd.h: alga_contigs_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "prefsuf_kernels.h"
#include "unitig_kernels.h"

namespace alga {

// counters[] (unsigned long long) the contig kernels fill; cleared before every round
enum { CT_CHAINS = 0, CT_CLOSED, CT_PARALLEL, CT_GROUPS_CUT, CT_CUT_REMOVED, CT_PATH_NODES, CT_TOUCHED, CT_OVERFLOW, CT_LONGEST_NODES, CT_LONGEST_BASES,
       CT_TOTAL_BASES, CT_COUNTERS };
constexpr uint32_t CT_NO_KEY = 0xFFFFFFFFu;        // key of a chain without interior: it loses every tie

// one chain, stored at the index of its first edge a -> b in B (a not in P): its end c, weight, node count, the node before c, the smallest
// read index of its interior, the index of the twin chain's first edge (c^1 -> x^1)
struct __attribute__((aligned(16))) CtChain { int32_t end, w, nodes, x; uint32_t key; int32_t tw, pad0, pad1; };

// 2a: pflag[v] = v is a path node of B; nxt / noff = the edge out of a path node into a path node (-1: none)
void launch_ct_pflags(const alga_edge_dev *B, const uint32_t *rowptr, int32_t n, uint32_t *pflag, hipStream_t s);
void launch_ct_next(const alga_edge_dev *B, const uint32_t *rowptr, const uint32_t *pflag, int32_t n, int32_t *nxt, int32_t *noff, hipStream_t s);
// a cycle of path nodes (what the ranking left unresolved): m = 2 * (smallest pair) and m^1 leave P, their links go; counters[UT_CYCLES]
void launch_ct_open_cycles(const UtRank *r, const UtMin *a, int32_t n, int32_t *nxt, int32_t *prv, uint32_t *pflag, unsigned long long *ut_counters,
                           hipStream_t s);
// per run of path nodes (indexed by its head): the last node and the smallest read index; counts the path nodes and the nodes with an edge
void launch_ct_run_info(const UtRank *r, const uint32_t *pflag, const int32_t *nxt, const uint32_t *rowptr, int32_t n, int32_t *tail_of, uint32_t *runkey,
                        unsigned long long *counters, hipStream_t s);
// 2b: the chain records, headchain[head of a run] = the chain that enters it, openflag[i] = edge i starts an open chain
void launch_ct_chains(const alga_edge_dev *B, const uint32_t *rowptr, uint64_t mb, const uint32_t *pflag, const UtRank *r, const int32_t *tail_of,
                      const uint32_t *runkey, CtChain *chain, uint32_t *headchain, uint32_t *openflag, unsigned long long *counters, hipStream_t s);
// the open chains as (a << 32 | c, chain) for the engine's edge sort
void launch_ct_open_keys(const alga_edge_dev *B, const uint32_t *openflag, const uint32_t *opos, const CtChain *chain, uint64_t mb,
                         unsigned long long *keys, uint32_t *vals, hipStream_t s);
// 2c on the sorted records: hflag[j] = first of its (a, c); there hw / hk = the group's smallest (weight, key); drop[chain] = 1 for the others
// of weight <= max_offset
void launch_ct_groups(const unsigned long long *keys, const uint32_t *vals, uint64_t no, const CtChain *chain, int32_t max_offset, uint32_t *hflag,
                      uint32_t *hw, uint32_t *hk, uint8_t *drop, unsigned long long *counters, hipStream_t s);
// 2d, after the cut of H: hlist[hrow[a] .. hrow[a] + hcnt[a]) are the survivors out of a; a group whose edge or whose twin's edge is not among
// them has its representatives dropped
void launch_ct_cut_back(const unsigned long long *keys, const uint32_t *vals, uint64_t no, const uint32_t *hflag, const uint32_t *hw, const uint32_t *hk,
                        const CtChain *chain, const uint32_t *hrow, const alga_edge_dev *hlist, const uint32_t *hcnt, uint8_t *drop,
                        unsigned long long *counters, hipStream_t s);
// 2e: keep[i] = neither the chain of edge i nor the chain of its twin is dropped; then the kept edges in order
void launch_ct_edge_keep(const alga_edge_dev *B, const uint32_t *rowptr, uint64_t mb, const uint32_t *pflag, const UtRank *r, const uint32_t *headchain,
                         const uint8_t *drop, uint32_t *keep, hipStream_t s);
void launch_ct_compact(const alga_edge_dev *B, const uint32_t *keep, const uint32_t *kpos, uint64_t mb, alga_edge_dev *out, hipStream_t s);
// step 3: win[i] = chain i is a `+` orientation; sizes per pair, oid[chain] = its oriented contig, cid[oriented contig] = its chain
void launch_ct_winners(const alga_edge_dev *B, uint64_t mb, const uint32_t *pflag, const CtChain *chain, uint32_t *win, hipStream_t s);
void launch_ct_pair_sizes(const alga_edge_dev *B, const CtChain *chain, const int32_t *len, const uint32_t *win, const uint32_t *pair_of, uint64_t mb,
                          uint32_t *pcnt, int32_t *ulen, int32_t *ulen2, uint32_t *uwords, uint32_t *oid, uint32_t *cid, unsigned long long *counters,
                          hipStream_t s);
// the layout: the two junction entries of every pair (one thread per chain), the path nodes in between (one thread per node)
void launch_ct_layout_ends(const alga_edge_dev *B, uint64_t mb, const CtChain *chain, const uint32_t *win, const uint32_t *pair_of,
                           const unsigned long long *path_off, int32_t *path_node, int32_t *path_pos, hipStream_t s);
void launch_ct_layout_inner(const alga_edge_dev *B, int32_t n, const uint32_t *pflag, const UtRank *r, const uint32_t *headchain, const uint32_t *win,
                            const uint32_t *pair_of, const unsigned long long *path_off, int32_t *path_node, int32_t *path_pos, hipStream_t s);
// step 4: per oriented contig X the number of oriented contigs that start at its last node; then (X << 32 | Y, pos of that node in X)
void launch_ct_join_count(const uint32_t *cid, const CtChain *chain, const uint32_t *rowptr, uint64_t n_oriented, uint32_t *deg, hipStream_t s);
void launch_ct_join_fill(const uint32_t *cid, const CtChain *chain, const uint32_t *rowptr, const uint32_t *oid, const uint32_t *epos, uint64_t n_oriented,
                         unsigned long long *keys, uint32_t *vals, hipStream_t s);
// FASTA of a contig result: sel[k] = pair k is written
void launch_ct_fasta_select(const int32_t *len, uint64_t n_pairs, int32_t min_length, uint32_t *sel, hipStream_t s);

}  // namespace alga
