// alga_amd/csrc/consensus_kernels.hip -- consensus sequences of the unitigs: every column decided by the majority of the reads laid over it
// (include/alga_amd.h: alga_unitig_consensus_device; the reference's Contig::correctSnipsInContig).
//
// Integer work only, wave-64, every output word written once, no atomics on the sequence words.
//   k_cons_check      one thread per path entry: ids, lengths and the layout the walk below relies on -> one flag word
//   k_cons_vote       one lane per output word (16 columns): the pair and the last entry that starts before the word's end by the two binary
//                     searches of k_ut_sequence, then a walk BACKWARDS over the entries while their end lies behind the word's first column (ends
//                     are non-decreasing along a path: every edge is a dovetail, checked).  Per covering entry the at most two row words are
//                     shifted to the word's 16 columns and masked to the columns the read covers; the four one-hot column masks are added into
//                     BIT-SLICED counters: 8 planes per base, bases A / C in the even / odd bits of one register and G / T of another (16 VGPRs),
//                     ripple carry, exact up to 255 covering entries
//   k_cons_vote_wide  the words with more covering entries than that: one wave per word, lane = (column, base), a 32-bit count per lane
//   k_cons_window     one wave per pair: first and last column with votes > min_votes from the 16-bit masks of its words (a scan from both
//                     ends, 64 words per step: a long unitig without any such column costs its wave len / 1024 steps)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "consensus_kernels.h"

namespace alga {

namespace {

constexpr int CS_BLOCK = 256;

__device__ __forceinline__ uint32_t cs_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t cs_wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t cs_wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// the last pair k with off[k] <= x (no pair is empty)
__device__ __forceinline__ uint32_t cs_pair_of(const unsigned long long *__restrict__ off, uint32_t n_pairs, uint64_t x) {
    uint32_t lo = 0, hi = n_pairs;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(CS_BLOCK) k_cons_check(ConsCfg c, unsigned long long *__restrict__ counters) {
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < c.n_entries; i += (uint64_t) gridDim.x * blockDim.x) {
        const int32_t v = c.path_node[i];
        if (v < 0 || v >= c.n) { bad |= CS_BAD_NODE; continue; }
        const int32_t l = c.len[v], p = c.path_pos[i];
        if (l <= 0 || (int64_t) l > 16ll * c.stride) { bad |= CS_BAD_LEN; continue; }
        const uint32_t k = cs_pair_of(c.path_off, c.n_pairs, i);
        const int64_t end = (int64_t) p + l;
        if (p < 0 || end > c.ulen[k] || (i == c.path_off[k] && p != 0)) bad |= CS_BAD_LAYOUT;
        if (i + 1 == c.path_off[k + 1]) { if (end != c.ulen[k]) bad |= CS_BAD_LAYOUT; continue; }
        const int32_t v2 = c.path_node[i + 1], p2 = c.path_pos[i + 1];
        if (v2 < 0 || v2 >= c.n) continue;                          // flagged by its own thread
        if (p2 < p || p2 >= end || (int64_t) p2 + c.len[v2] < end) bad |= CS_BAD_LAYOUT;
    }
    if (bad) atomicOr(&counters[CS_FLAGS], bad);
}

// what a lane / a wave knows about its word
struct CsWord {
    uint32_t k;                     // pair
    int32_t L, j0;                  // the unitig's length, the word's first column
    const int32_t *pn, *pp;         // the pair's path entries
    int64_t last;                   // the last entry with pos <= j0 + 15
};
__device__ __forceinline__ CsWord cs_locate(const ConsCfg &c, uint64_t w) {
    CsWord x;
    x.k = cs_pair_of(c.word_off, c.n_pairs, w);
    x.L = c.ulen[x.k];
    x.j0 = (int32_t) ((w - c.word_off[x.k]) << 4);
    const unsigned long long p0 = c.path_off[x.k];
    x.pn = c.path_node + p0; x.pp = c.path_pos + p0;
    const uint32_t cnt = (uint32_t) (c.path_off[x.k + 1] - p0);
    uint32_t a = 0, b = cnt;                                        // pos[0] = 0
    while (b - a > 1) { const uint32_t mid = a + ((b - a) >> 1); if (x.pp[mid] <= x.j0 + 15) a = mid; else b = mid; }
    x.last = a;
    return x;
}

// changed[k] += ch: one atomic per wave where all its lanes belong to one pair (nearly always), else one per lane that has something to add
__device__ __forceinline__ void cs_add_changed(int32_t *__restrict__ changed, bool active, uint32_t k, uint32_t ch, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint32_t k0 = __shfl(k, 0);
    const uint32_t total = cs_wave_sum(ch);
    if (!total) return;
    if (__all(!active || k == k0)) { if (lane == 0) atomicAdd(&changed[k0], (int32_t) total); }
    else if (ch) atomicAdd(&changed[k], (int32_t) ch);
    if (lane == 0) atomicAdd(&counters[CS_CHANGED], (unsigned long long) total);
}

__global__ void __launch_bounds__(CS_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) k_cons_vote(ConsCfg c, uint32_t *__restrict__ out, uint32_t *__restrict__ mask, uint8_t *__restrict__ votes,
                                                        int32_t *__restrict__ changed, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    uint32_t depth_max = 0, wide_n = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < c.n_words; base += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t w = base + threadIdx.x;
        const bool active = w < c.n_words;
        uint32_t k = 0, ch = 0;
        if (active) {
            const CsWord x = cs_locate(c, w);
            k = x.k;
            uint32_t ac[8], gt[8];                                   // plane p: bit 2 col = bit p of count(A), bit 2 col + 1 of count(C); G / T alike
#pragma unroll
            for (int p = 0; p < 8; p++) ac[p] = gt[p] = 0;
            uint32_t depth = 0;
            bool wide = false;
            for (int64_t i = x.last; i >= 0; i--) {
                const int32_t p = x.pp[i], v = x.pn[i], l = c.len[v];
                if (p + l <= x.j0) break;                             // ends are non-decreasing: nothing before it reaches the word either
                if (++depth > (uint32_t) CS_NARROW_DEPTH) { wide = true; break; }
                const int32_t q = x.j0 - p;                           // the read's base under the word's first column (negative: the read starts inside)
                const int32_t lo = q < 0 ? -q : 0, hi = l - q < 16 ? l - q : 16;      // columns [lo, hi) of the word are covered, lo < hi
                const uint32_t *row = c.words + (uint64_t) v * (uint64_t) c.stride;
                uint32_t codes;
                if (q >= 0) {
                    const int32_t wq = q >> 4, sh = q & 15;
                    uint64_t y = row[wq];
                    if (((q + hi - 1) >> 4) != wq) y |= (uint64_t) row[wq + 1] << 32;
                    codes = (uint32_t) (y >> (2 * sh));
                } else codes = row[0] << (2 * lo);
                const uint32_t cm = ((hi == 16 ? 0xFFFFFFFFu : (1u << (2 * hi)) - 1u) & ~((1u << (2 * lo)) - 1u)) & 0x55555555u;
                const uint32_t b0 = codes & cm, b1 = (codes >> 1) & cm, n1 = cm ^ b1;
                uint32_t ca = (n1 & ~b0) | ((n1 & b0) << 1), cg = (b1 & ~b0) | ((b1 & b0) << 1);
#pragma unroll
                for (int pl = 0; pl < 8; pl++) {
                    const uint32_t ta = ac[pl] & ca, tg = gt[pl] & cg;
                    ac[pl] ^= ca; gt[pl] ^= cg;
                    ca = ta; cg = tg;
                }
            }
            depth_max = depth > depth_max ? depth : depth_max;
            if (wide) { mask[w] = CS_WIDE_BIT; wide_n++; }
            else {
                uint32_t word = 0, m16 = 0;
                uint64_t vlo = 0, vhi = 0;                           // the 16 vote bytes
#pragma unroll 1
                for (int col = 0; col < 16; col++) {                  // (not unrolled: the planes are shifted down instead, which keeps the kernel at 8 waves / SIMD)
                    uint32_t n[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int pl = 0; pl < 8; pl++) {
                        n[0] |= (ac[pl] & 1u) << pl; n[1] |= ((ac[pl] >> 1) & 1u) << pl;
                        n[2] |= (gt[pl] & 1u) << pl; n[3] |= ((gt[pl] >> 1) & 1u) << pl;
                        ac[pl] >>= 2; gt[pl] >>= 2;
                    }
                    uint32_t best = n[0], b = 0;
                    if (n[1] > best) { best = n[1]; b = 1; }
                    if (n[2] > best) { best = n[2]; b = 2; }
                    if (n[3] > best) { best = n[3]; b = 3; }
                    // columns from L on are covered by nothing: all counts 0, base 0, no vote
                    word |= b << (2 * col);
                    m16 |= (uint32_t) ((int32_t) best > c.min_votes) << col;
                    const uint64_t t = (uint64_t) best << (8 * (col & 7));
                    vlo |= col < 8 ? t : 0ull; vhi |= col < 8 ? 0ull : t;
                }
                out[w] = word;
                mask[w] = m16;
                if (votes) *reinterpret_cast<uint4 *>(votes + (w << 4)) = make_uint4((uint32_t) vlo, (uint32_t) (vlo >> 32), (uint32_t) vhi, (uint32_t) (vhi >> 32));
                const uint32_t d = word ^ c.spelled[w];
                ch = (uint32_t) __popc((d | (d >> 1)) & 0x55555555u);
            }
        }
        cs_add_changed(changed, active, k, ch, counters);
    }
    depth_max = cs_wave_max(depth_max);
    wide_n = cs_wave_sum(wide_n);
    if (lane == 0) {
        if (depth_max) atomicMax(&counters[CS_MAX_DEPTH], (unsigned long long) depth_max);
        if (wide_n) atomicAdd(&counters[CS_WIDE], (unsigned long long) wide_n);
    }
}

__global__ void __launch_bounds__(CS_BLOCK) k_cons_vote_wide(ConsCfg c, uint32_t *__restrict__ out, uint32_t *__restrict__ mask, uint8_t *__restrict__ votes,
                                                             int32_t *__restrict__ changed, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63, col = lane >> 2;
    const uint32_t b = (uint32_t) lane & 3u;
    const uint64_t waves = (uint64_t) gridDim.x * (blockDim.x >> 6);
    uint32_t depth_max = 0;
    for (uint64_t base = ((uint64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) << 6; base < c.n_words; base += waves << 6) {
        const uint64_t mine = base + lane;
        unsigned long long todo = __ballot(mine < c.n_words && (mask[mine] & CS_WIDE_BIT));
        while (todo) {
            const uint64_t w = base + (uint64_t) (__ffsll(todo) - 1);
            todo &= todo - 1;
            const CsWord x = cs_locate(c, w);                         // the same for every lane of the wave
            const int32_t j = x.j0 + col;
            uint32_t count = 0, depth = 0;
            for (int64_t i = x.last; i >= 0; i--) {
                const int32_t p = x.pp[i], v = x.pn[i], l = c.len[v];
                if (p + l <= x.j0) break;
                depth++;
                if (j >= p && j - p < l) {
                    const int32_t q = j - p;
                    count += ((c.words[(uint64_t) v * (uint64_t) c.stride + (q >> 4)] >> (2 * (q & 15))) & 3u) == b;
                }
            }
            uint32_t best = __shfl(count, lane & ~3), bb = 0;
#pragma unroll
            for (int t = 1; t < 4; t++) { const uint32_t n = __shfl(count, (lane & ~3) + t); if (n > best) { best = n; bb = (uint32_t) t; } }
            const bool first = b == 0;                                // one lane per column speaks for it
            const uint32_t word = cs_wave_or(first ? bb << (2 * col) : 0u);
            const uint32_t m16 = cs_wave_or(first && (int64_t) best > (int64_t) c.min_votes ? 1u << col : 0u);
            if (first && votes) votes[(w << 4) + col] = (uint8_t) (best > 255u ? 255u : best);
            if (lane == 0) {
                out[w] = word;
                mask[w] = m16;
                const uint32_t d = word ^ c.spelled[w];
                const uint32_t ch = (uint32_t) __popc((d | (d >> 1)) & 0x55555555u);
                if (ch) { atomicAdd(&changed[x.k], (int32_t) ch); atomicAdd(&counters[CS_CHANGED], (unsigned long long) ch); }
            }
            depth_max = depth > depth_max ? depth : depth_max;
        }
    }
    if (lane == 0 && depth_max) atomicMax(&counters[CS_MAX_DEPTH], (unsigned long long) depth_max);
}

__global__ void __launch_bounds__(CS_BLOCK) k_cons_window(ConsCfg c, const uint32_t *__restrict__ mask, int32_t *__restrict__ trim_left, int32_t *__restrict__ len,
                                                          unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t) gridDim.x * (blockDim.x >> 6);
    unsigned long long kept = 0, bases = 0;
    for (uint64_t k = (uint64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < c.n_pairs; k += waves) {
        const uint64_t w0 = c.word_off[k];
        const int64_t nw = (int64_t) (c.word_off[k + 1] - w0);
        int64_t first = -1, last = -1;
        for (int64_t at = 0; at < nw && first < 0; at += 64) {
            const uint32_t m = at + lane < nw ? mask[w0 + (uint64_t) (at + lane)] & 0xFFFFu : 0u;
            const unsigned long long any = __ballot(m != 0);
            if (any) {
                const int src = __ffsll(any) - 1;
                first = ((at + src) << 4) + (__ffs((int) __shfl(m, src)) - 1);
            }
        }
        for (int64_t end = nw; first >= 0 && end > 0 && last < 0; end -= 64) {       // lane t looks at word end - 1 - t
            const uint32_t m = end - 1 - lane >= 0 ? mask[w0 + (uint64_t) (end - 1 - lane)] & 0xFFFFu : 0u;
            const unsigned long long any = __ballot(m != 0);
            if (any) {
                const int src = __ffsll(any) - 1;
                last = ((end - 1 - src) << 4) + (31 - __clz((int) __shfl(m, src)));
            }
        }
        if (lane == 0) {
            trim_left[k] = first < 0 ? 0 : (int32_t) first;
            len[k] = first < 0 ? 0 : (int32_t) (last - first + 1);
            if (first >= 0) { kept++; bases += (unsigned long long) (last - first + 1); }
        }
    }
    if (lane == 0 && kept) { atomicAdd(&counters[CS_KEPT], kept); atomicAdd(&counters[CS_TRIMMED], bases); }
}

inline unsigned cs_grid(const ConsCfg &c, uint64_t items, unsigned cap) {
    const uint64_t g = (items + CS_BLOCK - 1) / CS_BLOCK;
    if (c.max_blocks && c.max_blocks < cap) cap = c.max_blocks;
    return (unsigned) (g < cap ? g : cap);
}

}  // namespace

void launch_cons_check(const ConsCfg &c, unsigned long long *counters, hipStream_t s) {
    if (!c.n_entries) return;
    hipLaunchKernelGGL(k_cons_check, dim3(cs_grid(c, c.n_entries, 65536u)), dim3(CS_BLOCK), 0, s, c, counters);
}
void launch_cons_vote(const ConsCfg &c, uint32_t *out, uint32_t *mask, uint8_t *votes, int32_t *changed, unsigned long long *counters, hipStream_t s) {
    if (!c.n_words || !c.n_pairs) return;
    hipLaunchKernelGGL(k_cons_vote, dim3(cs_grid(c, c.n_words, 1u << 18)), dim3(CS_BLOCK), 0, s, c, out, mask, votes, changed, counters);
}
void launch_cons_vote_wide(const ConsCfg &c, uint32_t *out, uint32_t *mask, uint8_t *votes, int32_t *changed, unsigned long long *counters, hipStream_t s) {
    if (!c.n_words || !c.n_pairs) return;
    // a wave takes 64 consecutive words at a time
    hipLaunchKernelGGL(k_cons_vote_wide, dim3(cs_grid(c, (c.n_words + 63) / 64 * 64, 1u << 16)), dim3(CS_BLOCK), 0, s, c, out, mask, votes, changed, counters);
}
void launch_cons_window(const ConsCfg &c, const uint32_t *mask, int32_t *trim_left, int32_t *len, unsigned long long *counters, hipStream_t s) {
    if (!c.n_pairs) return;
    hipLaunchKernelGGL(k_cons_window, dim3(cs_grid(c, (uint64_t) c.n_pairs * 64, 1u << 16)), dim3(CS_BLOCK), 0, s, c, mask, trim_left, len, counters);
}

}  // namespace alga
