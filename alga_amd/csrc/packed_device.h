// alga_amd/csrc/packed_device.h -- packed 2-bit sequence sets on the device: the helpers over an offset table and a packed array, the one body
// of every kernel that writes such a set, and the grid size the stages' launchers share.  Included by the *_kernels.hip files only; everything
// here is internal to the including file (the build has no relocatable device code).
//
// A sequence set is `n_items` items laid end to end in a column space: item i holds the columns [off[i], off[i + 1]), column g is the 2-bit
// code in word g >> 4 at bits 2 (g & 15), and columns = off[n_items] <= 0xFFFFFFFE.  packed_words_body writes the words of such a set, one
// lane per word; what differs between the stages enters as
//   BaseOf   uint32_t operator()(uint32_t item, q): the code 0..3 of base q of the item (q < its length; handed over as uint64_t, a rule that
//            goes on in 32 bits takes it as uint32_t)
// DESIGN.md ("The packed-word builder") names the kernels that use it; a new stage that packs a sequence set uses the body and copies none of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace alga {

namespace {

// the item of position g < off[n]: the last i with off[i] <= g (it has a length: off[i + 1] > g)
__device__ __forceinline__ uint32_t item_of(const uint32_t *__restrict__ off, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t base_at(const uint32_t *__restrict__ words, uint64_t g) { return (words[g >> 4] >> ((g & 15ull) << 1)) & 3u; }

// Words 0 .. n_words - 1 of the set, a grid-stride loop of blocks of BLOCK lanes, a lane a word: one bisection for the word's first column, then
// a walk through its 16 columns.  A word at or past `columns` is 0: a caller whose array has padding words behind the last column passes
// n_words with them.  Every column the walk meets is g < columns = off[n_items], so it ends at an item that has a length (empty items are
// stepped over, nothing past off[n_items] is read).
template <int BLOCK, class BaseOf>
__device__ __forceinline__ void packed_words_body(const uint32_t *__restrict__ off, uint32_t n_items, uint64_t columns, uint64_t n_words, uint32_t *__restrict__ words,
                                                  BaseOf base_of) {
    for (uint64_t w = (uint64_t) blockIdx.x * BLOCK + threadIdx.x; w < n_words; w += (uint64_t) gridDim.x * BLOCK) {
        const uint64_t g0 = w << 4;
        uint32_t v = 0;
        if (g0 < columns) {
            uint32_t it = item_of(off, n_items, (uint32_t) g0);
            for (int j = 0; j < 16; j++) {
                const uint64_t g = g0 + (uint64_t) j;
                if (g >= columns) break;
                while ((uint64_t) off[it + 1] <= g) it++;
                v |= base_of(it, g - off[it]) << (2 * j);
            }
        }
        words[w] = v;
    }
}

// Blocks of `block` lanes for `items` items, at least one and at most `cap`.  Where a stage has a "<stage>_max_blocks" option the cap is that
// (8192 unless a test lowers it: a knob of the tests, which make every grid-stride loop of the stage take further passes).
inline unsigned stage_grid(uint64_t items, int block, uint64_t cap) {
    const uint64_t g = (items + (uint64_t) block - 1) / (uint64_t) block;
    return (unsigned) std::max<uint64_t>(1, std::min<uint64_t>(g, cap));
}

}  // namespace

}  // namespace alga
