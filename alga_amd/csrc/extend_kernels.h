// alga_amd/csrc/extend_kernels.h -- launchers of extend_kernels.hip (the extension of contigs by paired connections of include/alga_amd.h:
// alga_extend_contigs_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/alga_amd.h"
#include "prefsuf_kernels.h"
#include "unitig_kernels.h"

namespace alga {

// counters[] (unsigned long long) the extension kernels fill
enum { EX_FLAGS = 0, EX_CANDIDATES, EX_DIRECT, EX_LINKS, EX_AMBIGUOUS, EX_JOINABLE, EX_HEAD_MAX, EX_LONGEST_NODES, EX_LONGEST_BASES, EX_TOTAL_BASES, EX_OVERFLOW,
       EX_COUNTERS };
// bits of counters[EX_FLAGS]
enum { EX_BAD_VALUE = 1, EX_BAD_TWIN = 2, EX_BAD_MATE = 4 };

// the per-wave table of k_ex_count: EX_SLOTS read indices in LDS, filled with at most EX_FILL head entries a pass (load factor <= 1/2); four
// waves a block: 32 KB of LDS a block
constexpr int EX_WAVES = 4, EX_FILL = ALGA_EXTEND_HEAD_SLICE, EX_SLOTS = 2 * EX_FILL;

// the contig result the extension reads (oriented contig c: pair c >> 1, `+` when c & 1), the node lengths and the pairing
struct ExIn {
    const int32_t *len;
    const uint8_t *pair_off;          // nullptr: every read unpaired
    int32_t n;
    const int32_t *path_node, *path_pos;
    const unsigned long long *path_off;
    const int32_t *ulen;
    uint32_t P;
    const alga_edge_dev *edges;       // the contig graph, sorted by (src, dst)
    const uint32_t *rowptr;           // ... its row pointers over oriented contig ids (2 P + 1)
};

// step 0 on pair_off -> counters[EX_FLAGS]; nothing else is written
void launch_ex_check(const uint8_t *pair_off, int32_t n, unsigned long long *counters, hipStream_t s);
// step 1: w[c] of every oriented contig, kcnt[c] = its entries - 1
void launch_ex_weights(const ExIn &in, int32_t *w, int32_t *kcnt, hipStream_t s);
// steps 2-4, one wave per oriented contig X: dlink[X] = Y when X -> Y is a DIRECT link (-1: none)
void launch_ex_count(const ExIn &in, const int32_t *w, int32_t min_chain_weight, int32_t min_connections, int32_t max_insert, int32_t *dlink,
                     unsigned long long *counters, hipStream_t s);
// step 4-5: outcnt[X] / sole[X] = the links of L* out of X / the only one; then nxt[X] = the joinable link out of X (-1: none)
void launch_ex_outlinks(const ExIn &in, const int32_t *dlink, uint32_t *outcnt, int32_t *sole, unsigned long long *counters, hipStream_t s);
void launch_ex_next(const uint32_t *outcnt, const int32_t *sole, uint32_t n2, int32_t *nxt, unsigned long long *counters, hipStream_t s);
// the ranking's records as arrays: head, bases and links before X on its path
void launch_ex_save(const UtRank *r, uint32_t n2, int32_t *xhead, int32_t *xbase, int32_t *xrank, hipStream_t s);
// win[h ^ 1] = 1 for the head h of a `+` path (the key h ^ 1 puts `+` of a pair before its `-`)
void launch_ex_winners(const int32_t *prv, const int32_t *tail_of, uint32_t n2, uint32_t *win, hipStream_t s);
// per new pair: entries, length (ulen2: per oriented id), words, seam indices; r2: the ranking whose pos counts the entries before X
void launch_ex_pair_sizes(const ExIn &in, const int32_t *prv, const int32_t *tail_of, const uint32_t *win, const uint32_t *pair_of, const int32_t *xbase,
                          const int32_t *xrank, const UtRank *r2, const int32_t *kcnt, uint32_t *pcnt, int32_t *ulen, int32_t *ulen2, uint32_t *uwords,
                          uint32_t *scnt, unsigned long long *counters, hipStream_t s);
// step 8 and the new ids: uid[X] = the new oriented id of X's path, the seam indices of the `+` paths (one thread per oriented contig)
void launch_ex_ids(const ExIn &in, const int32_t *xhead, const int32_t *xrank, const UtRank *r2, const int32_t *nxt, const int32_t *tail_of,
                   const uint32_t *win, const uint32_t *pair_of, const int32_t *kcnt, const unsigned long long *seam_off, int32_t *seam_entry, int32_t *uid,
                   hipStream_t s);
// step 6, one thread per path entry of the input (n_entries of them): the entries of the `+` paths into the new path arrays
void launch_ex_layout(const ExIn &in, uint64_t n_entries, const int32_t *xhead, const int32_t *xbase, const int32_t *xrank, const UtRank *r2,
                      const uint32_t *win, const int32_t *uid, const unsigned long long *path_off, int32_t *path_node, int32_t *path_pos, hipStream_t s);
// step 7: per path tail X the heads that start at its last node; then (uid[X] << 32 | uid[Y], position of that node)
void launch_ex_join_count(const ExIn &in, const int32_t *nxt, const int32_t *prv, uint32_t *deg, hipStream_t s);
void launch_ex_join_fill(const ExIn &in, const int32_t *nxt, const int32_t *prv, const int32_t *uid, const int32_t *xbase, const int32_t *w,
                         const uint32_t *epos, unsigned long long *keys, uint32_t *vals, hipStream_t s);

}  // namespace alga
