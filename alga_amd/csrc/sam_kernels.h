// alga_amd/csrc/sam_kernels.h -- launchers of sam_kernels.hip: the pairs judged over the Hamming and the gapped placement together, and every
// read as a SAM record (include/alga_amd.h: alga_judge_pairs_device, alga_write_sam_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

// counters[] (unsigned long long): the refusal flag, then what k_sam_judge counts
enum { SAM_BAD_PAIR = 0, SAM_LIVE, SAM_PLACED_H, SAM_PLACED_G, SAM_UNPLACED, SAM_PAIRS, SAM_PROPER, SAM_IMPROPER, SAM_SPLIT, SAM_NOT_UNIQUE, SAM_WITH_GAPPED,
       SAM_PROPER_GAPPED, SAM_INSERT_SUM, SAM_COUNTERS };
// bits the sizes pass of the writer leaves in counters[GFA_FLAGS] (above the GFA's own)
enum { SAM_BAD_LEN = 256, SAM_BAD_SCRIPT = 512 };

// the two placement passes over one node set: the combined view of a read is made from these (g_state == nullptr: the Hamming pass alone)
struct SamReads {
    const int32_t *len;               // the node lengths: len[2r + 1] is read r's
    const uint8_t *pair_off;          // per node, or nullptr
    const int32_t *h_target, *h_pos;
    const uint8_t *h_mm, *h_state;
    const int32_t *g_target, *g_pos, *g_end;
    const uint8_t *g_edits, *g_state;
    const uint32_t *g_cigar_off, *g_cigar;
    uint64_t R;
};

// the pair_off rules of the placement (SAM_BAD_PAIR)
void launch_sam_pair_check(const uint8_t *pair_off, uint64_t n, unsigned long long *counters, int max_blocks, hipStream_t s);
// flag[r], tlen[r], hist[max_insert + 1] (zeroed), counters[SAM_LIVE ..]
void launch_sam_judge(const SamReads &v, int32_t max_insert, uint16_t *flag, int32_t *tlen, unsigned long long *hist, unsigned long long *counters, int max_blocks,
                      hipStream_t s);

// the SAM records: one per live read
struct SamText {
    SamReads v;
    const uint32_t *words;            // the rows of the node set, stride words apart
    int32_t stride;
    const uint16_t *flag;
    const int32_t *tlen;
    const uint32_t *col_off;          // the placement's: len[t] = col_off[t + 1] - col_off[t]
    const unsigned long long *t_reads, *t_bases;   // the placement's, for the names in the depth form
    int names_depth, skip_unplaced;
    int max_blocks;                   // the cap of the write grid (0: its own)
    uint64_t n;                       // == v.R
};
void launch_sam_sizes(const SamText &f, uint32_t *sizes, unsigned long long *counters /* GFA_FLAGS / GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_sam_write(const SamText &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
