// alga_amd/csrc/contain_kernels.h -- launchers of contain_kernels.hip: contigs contained in another contig dropped
// (include/alga_amd.h: alga_drop_contained_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seed_index.h"

namespace alga {

// counters[] (unsigned long long): the refusal flag and the sizes, then what the kernels count
enum { CN_BAD = 0, CN_COLUMNS, CN_PAD_COLUMNS, CN_INDEX_POS, CN_QUERIES, CN_SEEDS, CN_SEEDS_OVER, CN_CANDIDATES, CN_CONTAINED, CN_MINUS, CN_DUPLICATES, CN_AMBIGUOUS,
       CN_SATURATED, CN_KEPT, CN_REMOVED, CN_LONGEST_CONTAINED, CN_COLUMNS_AFTER, CN_LONGEST_KEPT, CN_COUNTERS };
constexpr uint32_t CN_BAD_LEN = 1;                                       // bit of counters[CN_BAD]
constexpr uint8_t  CN_CONTAINED_BIT = 1, CN_MINUS_BIT = 2, CN_AMBIGUOUS_BIT = 4, CN_DUPLICATE_BIT = 8, CN_KEPT_BIT = 16;   // ALGA_CONTAIN_* of include/alga_amd.h
constexpr uint32_t CN_HITS_CAP = 256;                                    // what a (c, s) counts its containers up to: two of them still say "more than 255"

// a ragged target set as the placement takes it
struct CnTargets {
    const uint32_t *words;
    const unsigned long long *begin;  // T: base index of the first base
    const int32_t *len;               // T
    uint32_t T;
    uint32_t max_blocks;              // the cap of every grid here but k_ct_contain's and the FASTA kernels' (8192; option "contain_max_blocks")
};
// the targets in a column space of their own, the space their index is built over (alga_seed_index): target t is the columns off[t] ..
// off[t] + len[t], off[t] a multiple of 16; cols holds the targets, n = T
struct CnSpace : SeedSpace {
    const uint32_t *rcols;            // the reverse complement of every target, at the same columns
};
// what k_ct_contain leaves per (c, s), x = 2c + s: the smallest (mm, h, p) and the number of containers, counted up to CN_HITS_CAP
struct CnQueryOut {
    uint32_t *mm, *hits;
    int32_t *host, *pos;
};
// per target (T)
struct CnOut {
    int32_t *host, *host_pos;
    uint8_t *host_orient;
    uint32_t *mm;
    uint8_t *hits, *state;
};
// one of the two buffers of the pointer jumping
struct CnRoots {
    int32_t *root, *pos;
    uint8_t *orient;
};

// a negative length -> counters[CN_BAD]; pad[t] = len[t] rounded up to 16 (T + 1 entries, the last 0; 0 for a negative length);
// counters[CN_COLUMNS], [CN_PAD_COLUMNS], [CN_INDEX_POS], [CN_QUERIES]
void launch_cn_check(const CnTargets &t, int32_t k, uint32_t *pad, unsigned long long *counters, hipStream_t s);
// the targets and their reverse complements, one thread per word
void launch_cn_cols(const CnTargets &t, const CnSpace &sp, uint32_t *cols, uint32_t *rcols, hipStream_t s);
// one wave per (c, s) (blocks: seed_blocks(2T))
void launch_cn_contain(const CnSpace &sp, const SeedIndex &x, int32_t k, int32_t max_permille, int32_t max_occ, const CnQueryOut &q, int blocks, unsigned long long *counters,
                       hipStream_t s);
// one thread per target: the two orientations into host / host_pos / host_orient / mm / hits / state; keep[c] (T + 1 entries, the last 0) for the scan
void launch_cn_decide(const CnTargets &t, const CnQueryOut &q, const CnOut &o, uint32_t *keep, unsigned long long *counters, hipStream_t s);
// the roots by pointer jumping: a = what item 4 says, then rounds of b = a after a
void launch_cn_root_init(const CnTargets &t, const CnOut &o, const CnRoots &a, hipStream_t s);
void launch_cn_root_jump(const CnTargets &t, const CnRoots &a, const CnRoots &b, hipStream_t s);
// absorbed[root[c]] += 1 for every contained c (absorbed zeroed)
void launch_cn_absorbed(const CnTargets &t, const CnOut &o, const CnRoots &r, uint32_t *absorbed, hipStream_t s);
// new ids from the scan of keep: d_new (T), d_old and klen (n_kept; klen has one entry more, zeroed, for its scan)
void launch_cn_number(const CnTargets &t, const uint32_t *keep, const uint32_t *keep_scan, int32_t *d_new, int32_t *d_old, int32_t *klen, hipStream_t s);
// the kept targets' column array, one thread per word; begin[j] = col_off[j]
void launch_cn_build(const CnTargets &t, const int32_t *d_old, const uint32_t *col_off, uint32_t n_kept, uint64_t columns, uint32_t *words, unsigned long long *begin, hipStream_t s);

// `>contig_id=<j>_length=<len>_absorbed=<m>\n<kept contig>\n`, one record per kept target
struct CnFasta {
    const uint32_t *words, *col_off, *absorbed;
    const int32_t *len, *old;
    uint64_t n;
};
void launch_cn_fasta_sizes(const CnFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_cn_fasta_write(const CnFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
