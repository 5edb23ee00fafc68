// alga_amd/csrc/consensus_kernels.h -- launchers of consensus_kernels.hip (the per-column read vote of include/alga_amd.h: alga_unitig_consensus_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

// what the consensus kernels read: the node set and the result of the unitig call
struct ConsCfg {
    const uint32_t *words;          // node rows
    int32_t stride;
    const int32_t *len;
    int32_t n;
    const int32_t *path_node, *path_pos;
    const unsigned long long *path_off, *word_off;
    const int32_t *ulen;
    const uint32_t *spelled;        // the unitig call's sequences (for `changed`)
    uint32_t n_pairs;
    uint64_t n_words, n_entries;
    int32_t min_votes;
    uint32_t max_blocks;            // cap on every grid (0: the kernel's own cap); the rest is done by grid stride
};

// counters[] (unsigned long long) the kernels fill
enum { CS_FLAGS = 0, CS_CHANGED, CS_MAX_DEPTH, CS_WIDE, CS_KEPT, CS_TRIMMED, CS_COUNTERS };
// bits of counters[CS_FLAGS]
enum { CS_BAD_NODE = 1, CS_BAD_LEN = 2, CS_BAD_LAYOUT = 4 };
// mask[w]: bits 0..15 = the columns of word w with votes > min_votes; this bit = the word is left to the wide route
constexpr uint32_t CS_WIDE_BIT = 0x80000000u;
// a word takes the wide route when more than this many path entries cover it (the bit-sliced counters have 8 planes)
constexpr int CS_NARROW_DEPTH = 255;

// one thread per path entry: node ids in range, lengths within the rows, and the layout the vote relies on (first entry at 0, positions
// and ends non-decreasing, no gap between consecutive entries, last end == the unitig's length) -> counters[CS_FLAGS]; nothing else is written
void launch_cons_check(const ConsCfg &c, unsigned long long *counters, hipStream_t s);
// one lane per output word: out[w], mask[w], the 16 bytes votes + 16 w (votes may be null), changed[pair] (zeroed by the caller)
void launch_cons_vote(const ConsCfg &c, uint32_t *out, uint32_t *mask, uint8_t *votes, int32_t *changed, unsigned long long *counters, hipStream_t s);
// the words k_cons_vote left (CS_WIDE_BIT): one wave per word, lane = (column, base), 32-bit counts
void launch_cons_vote_wide(const ConsCfg &c, uint32_t *out, uint32_t *mask, uint8_t *votes, int32_t *changed, unsigned long long *counters, hipStream_t s);
// one wave per pair: first and last set bit of its mask words -> trim_left[k], len[k]
void launch_cons_window(const ConsCfg &c, const uint32_t *mask, int32_t *trim_left, int32_t *len, unsigned long long *counters, hipStream_t s);

}  // namespace alga
