// alga_amd/csrc/gfa_kernels.h -- launchers of gfa_kernels.hip (the GFA 1.0 export of include/alga_amd.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "prefsuf_kernels.h"

namespace alga {

// what the GFA kernels read: the node set, the edge list and the layout (items: n_seg segment lines, then m link lines)
struct GfaCfg {
    const uint32_t *words;
    int32_t stride;
    const int32_t *len;
    int32_t n;
    const alga_edge_dev *e;
    uint64_t m;
    uint64_t n_seg;                 // twins: n / 2, else n
    int32_t twins, seqs;
    // optional: ragged rows (the unitig graph).  Non-null: the row of node v starts at words + row_off[v >> 1] (one row per twin pair, read
    // through its odd node; `stride` is not used); null: at words + v * stride
    const unsigned long long *row_off = nullptr;
    __host__ __device__ __forceinline__ const uint32_t *row(uint64_t node) const {
        return row_off ? words + row_off[twins ? node >> 1 : node] : words + node * (uint64_t) stride;
    }
};

// The consensus windows as FASTA (one ragged row per item): item j is `>unitig_<j>_length=<len[j]>\n<bases seq_off[j] .. seq_off[j] + len[j] of its
// row>\n`, written when len[j] >= min_length and len[j] > 0.  rec_rank non-null: the records of a contig result,
// `>contig_id=<rec_rank[j]>_length=<len[j]>` (rec_rank[j] = records written before item j)
struct GfaFasta {
    const uint32_t *words;
    const unsigned long long *row_off;
    const int32_t *len, *seq_off;
    const uint32_t *rec_rank;
    uint64_t n;
    int32_t min_length;
};

// counters[] (unsigned long long) the kernels fill
enum { GFA_FLAGS = 0, GFA_SEGMENTS, GFA_LINKS, GFA_MERGED, GFA_MAX_LINE, GFA_COUNTERS };
// bits of counters[GFA_FLAGS]
enum { GFA_BAD_ID = 1, GFA_BAD_ORDER = 2, GFA_BAD_LEN = 4, GFA_BAD_TWIN = 8 };

void   launch_gfa_check(const GfaCfg &c, unsigned long long *counters, hipStream_t s);
// rowptr: per-source row pointers of the (validated) edge list; sizes: n_seg + m line lengths in bytes (0 = not written)
void   launch_gfa_sizes(const GfaCfg &c, const uint32_t *rowptr, uint32_t *sizes, unsigned long long *counters, hipStream_t s);
size_t gfa_scan_tiles(uint64_t n);
// off[0 .. n] = exclusive 64-bit prefix sums of sizes[0 .. n) (off[n] = total); tiles: gfa_scan_tiles(n) + 1 entries
void   launch_gfa_scan64(const uint32_t *sizes, uint64_t n, unsigned long long *off, unsigned long long *tiles, hipStream_t s);
// bounds[k] (k in [0, K]) = first item whose offset is >= k * step (bounds[K] = n), bounds[K + 1 + k] = that item's offset
void   launch_gfa_bounds(const unsigned long long *off, uint64_t n, uint64_t step, uint64_t K, unsigned long long *bounds, hipStream_t s);
// the lines of items [i0, i1) into buf, item i at byte off[i] - off[i0]
void   launch_gfa_format(const GfaCfg &c, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);
void   launch_gfa_fasta_sizes(const GfaFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s);
void   launch_gfa_fasta_write(const GfaFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
