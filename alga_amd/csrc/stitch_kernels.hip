// alga_amd/csrc/stitch_kernels.hip -- scaffold joins whose contig ends overlap stitched into one sequence (include/alga_amd.h:
// alga_stitch_targets_device; the definition is the comment there, host side in engine_stitch.hip).
//
// An entry names two ends and nothing else is compared: no index, no seed condition, every overlap length.  Integer work only, wave-64,
// nothing depends on thread order.
//   k_st_targets      begin / len of a placement's targets from its col_off
//   k_st_check        the refusals of the selected entries; a per-end count finds an end that two selected entries name; end_entry
//   k_st_overlap      one wave per selected entry.  The first M = min(W_a, W_b) bases of P_a and the last M bases of E_b are staged in the
//                     wave's piece of LDS (at most 4096 bases each: 256 words + a zero word behind E, 2 KB per wave).  Lane l takes
//                     o = min_overlap + l + 64 i: 16 bases at a time, one word of P_a (every lane reads the same address: a broadcast) against
//                     the funnel-shifted pair of words of E_b at base M - o (16 neighbouring lanes share a word pair: at most five addresses
//                     per 64 lanes, each on a bank of its own), mismatches = popc((x | x >> 1) & 0x55555555), the last word masked; a lane leaves
//                     its o past max_mismatches.  hits, best = the smallest (mm, o descending) and the candidates outside the slack are reduced
//                     across the wave; lane 0 writes the entry.  The loop over the entries is uniform per block (the barriers around the LDS
//                     piece are the block's), an unselected entry costs its wave one branch.
//   k_st_joins        one thread per end: the stitched entry that names it -> join / partner / olen / mm / hits / state as k_mg_joins leaves them
//   k_st_dropped      one thread per entry: the join a cycle lost -> DROPPED_CYCLE
// Cycles, ranks, places, layout, build and the FASTA are the merge stage's kernels (merge_kernels.hip), launched from engine_stitch.hip.
// Block 256 and the grid caps are picked, not tuned; option "stitch_max_blocks" lowers the cap of every grid here (a knob of the tests).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/alga_amd.h"
#include "stitch_kernels.h"
#include "seed_device.h"
#include "text_record.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int ST_BLOCK = 256, ST_WAVES = ST_BLOCK / 64;
constexpr int ST_P_WORDS = ST_MAX_OVERLAP / 16, ST_E_WORDS = ST_MAX_OVERLAP / 16 + 1;      // E: a zero word behind the last (the funnel shift's upper half)

__global__ void __launch_bounds__(ST_BLOCK) k_st_targets(const uint32_t *__restrict__ col_off, uint32_t T, unsigned long long *__restrict__ begin,
                                                         int32_t *__restrict__ len) {
    for (uint64_t i = (uint64_t) blockIdx.x * ST_BLOCK + threadIdx.x; i < T; i += (uint64_t) gridDim.x * ST_BLOCK) {
        begin[i] = col_off[i]; len[i] = (int32_t) (col_off[i + 1] - col_off[i]);
    }
}

__device__ __forceinline__ bool st_selected(const StEntries &en, uint64_t j) {
    if (!en.state) return true;
    const uint8_t st = en.state[j];
    return (st & ALGA_SCAFFOLD_BUNDLE_JOIN) && !(st & ALGA_SCAFFOLD_BUNDLE_DROPPED_CYCLE);
}

// (end_count and end_entry have 2T entries: only ends below 2T index them)
__global__ void __launch_bounds__(ST_BLOCK) k_st_check(StEntries en, uint32_t T, uint32_t *__restrict__ end_count, int32_t *__restrict__ end_entry,
                                                       unsigned long long *__restrict__ counters) {
    unsigned long long bad = 0, n_sel = 0;
    const uint64_t E = 2ull * T;
    for (uint64_t j = (uint64_t) blockIdx.x * ST_BLOCK + threadIdx.x; j < en.J; j += (uint64_t) gridDim.x * ST_BLOCK) {
        if (!st_selected(en, j)) continue;
        n_sel++;
        const uint32_t a = en.a[j], b = en.b[j];
        if (a >= E || b >= E) { bad |= ST_BAD_END; continue; }
        if ((a >> 1) == (b >> 1)) { bad |= ST_BAD_SAME_TARGET; continue; }
        if (atomicAdd(&end_count[a], 1u)) bad |= ST_BAD_END_TWICE;
        if (atomicAdd(&end_count[b], 1u)) bad |= ST_BAD_END_TWICE;
        end_entry[a] = (int32_t) j; end_entry[b] = (int32_t) j;            // (an end named twice: the call is refused, the value is never read)
    }
    n_sel = wave_sum(n_sel);
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) {
        if (n_sel) atomicAdd(&counters[ST_SELECTED], n_sel);
        if (bad) atomicOr(&counters[ST_BAD], bad);
    }
}

// 16 bases of a window of M bases from q0 on (zero past M); base(q) = the window's base q
template <class F> __device__ __forceinline__ uint32_t st_word(uint32_t q0, uint32_t M, F base) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 16 && q0 + i < M; i++) v |= base(q0 + i) << (2 * i);
    return v;
}

// (after the check: no length is negative, the ends of a selected entry are below 2T and of two targets.  M <= W <= len / 2: every base read
// lies in its target; M <= 4096: word M / 16 of the E piece is its last)
__global__ void __launch_bounds__(ST_BLOCK) k_st_overlap(MgTargets t, StEntries en, StParams p, StEntryOut out, unsigned long long *__restrict__ counters) {
    __shared__ uint32_t lds[ST_WAVES][ST_P_WORDS + ST_E_WORDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *Pw = lds[wv], *Ew = Pw + ST_P_WORDS;
    unsigned long long n_with = 0, n_amb = 0, n_sat = 0, n_out = 0;                          // wave-uniform
    for (uint64_t j0 = (uint64_t) blockIdx.x * ST_WAVES; j0 < en.J; j0 += (uint64_t) gridDim.x * ST_WAVES) {       // block-uniform
        const uint64_t j = j0 + (uint64_t) wv;
        const bool sel = j < en.J && st_selected(en, j);                                     // wave-uniform
        int32_t M = 0, gap = 0;
        if (sel) {
            const uint32_t a = en.a[j], b = en.b[j];
            const int32_t na = t.len[a >> 1], nb = t.len[b >> 1];
            gap = en.gap[j];
            M = std::min(std::min(na >> 1, nb >> 1), p.max_overlap);                         // min(W_a, W_b)
            if (M >= p.min_overlap) {
                const uint64_t a0 = t.begin[a >> 1], b0 = t.begin[b >> 1];
                const uint32_t uM = (uint32_t) M, nw = (uM + 15u) >> 4;
                const uint32_t *words = t.words;
                for (uint32_t w = (uint32_t) lane; w <= nw; w += 64u) {
                    // P_a: the first bases read inward from end a; the last M bases of E_b: the contig end at the right
                    if (w < nw) {
                        Pw[w] = (a & 1u) ? st_word(w << 4, uM, [&](uint32_t q) { return 3u - base_at(words, a0 + (uint64_t) (na - 1) - q); })
                                         : st_word(w << 4, uM, [&](uint32_t q) { return base_at(words, a0 + q); });
                        Ew[w] = (b & 1u) ? st_word(w << 4, uM, [&](uint32_t q) { return base_at(words, b0 + (uint64_t) (nb - M) + q); })
                                         : st_word(w << 4, uM, [&](uint32_t q) { return 3u - base_at(words, b0 + (uint64_t) (uM - 1u - q)); });
                    } else Ew[w] = 0;
                }
            }
        }
        __syncthreads();
        if (sel) {
            unsigned long long best = ~0ull;
            uint32_t hits = 0, outside = 0;
            for (int32_t o0 = p.min_overlap; o0 <= M; o0 += 64) {                            // wave-uniform
                const int32_t o = o0 + lane;
                if (o > M) continue;
                const uint32_t off = (uint32_t) (M - o), wi = off >> 4, sh = (off & 15u) << 1, nw = ((uint32_t) o + 15u) >> 4;
                uint32_t mm = 0;
                for (uint32_t w = 0; w < nw && mm <= (uint32_t) p.max_mm; w++) {
                    uint32_t x = Pw[w] ^ __funnelshift_r(Ew[wi + w], Ew[wi + w + 1], sh);
                    const uint32_t rem = (uint32_t) o - (w << 4);
                    if (rem < 16u) x &= (1u << (2u * rem)) - 1u;
                    mm += (uint32_t) __popc((x | (x >> 1)) & 0x55555555u);
                }
                if (mm > (uint32_t) p.max_mm) continue;
                long long g = (long long) gap + (long long) o;
                g = g < 0 ? -g : g;
                if (g > (long long) p.slack) { outside++; continue; }
                hits++;
                const unsigned long long key = ((unsigned long long) mm << 13) | (unsigned long long) (uint32_t) (ST_MAX_OVERLAP - o);
                best = key < best ? key : best;
            }
            const unsigned long long win = wave_min_u64(best), n_hits = wave_sum((unsigned long long) hits);
            n_out += wave_sum((unsigned long long) outside);
            int32_t o_out = 0;
            uint8_t mm8 = 0, hits8 = 0, st8 = ST_J_SELECTED;
            if (win != ~0ull) {
                o_out = ST_MAX_OVERLAP - (int32_t) (win & 8191ull); mm8 = (uint8_t) (win >> 13);
                hits8 = (uint8_t) (n_hits > 255ull ? 255ull : n_hits);
                st8 |= (uint8_t) (ST_J_HAS_OVERLAP | (n_hits > 1ull ? ST_J_AMBIGUOUS : ST_J_STITCHED));
                n_with++; n_amb += n_hits > 1ull; n_sat += n_hits > 255ull;
            }
            if (lane == 0) { out.olen[j] = o_out; out.mm[j] = mm8; out.hits[j] = hits8; out.state[j] = st8; }
        } else if (j < en.J && lane == 0) { out.olen[j] = 0; out.mm[j] = 0; out.hits[j] = 0; out.state[j] = 0; }
        __syncthreads();                                                                     // the pieces are staged again
    }
    if (lane == 0) {
        if (n_with) atomicAdd(&counters[ST_WITH_OVERLAP], n_with);
        if (n_amb) atomicAdd(&counters[ST_AMBIGUOUS], n_amb);
        if (n_sat) atomicAdd(&counters[ST_SATURATED], n_sat);
        if (n_out) atomicAdd(&counters[ST_OUTSIDE_SLACK], n_out);
    }
}

// (a thread writes its own end only; end_entry[x] names a selected entry, whose ends are in range)
__global__ void __launch_bounds__(ST_BLOCK) k_st_joins(StEntries en, StEntryOut o, const int32_t *__restrict__ end_entry, uint32_t E, MgEndOut eo, uint32_t *__restrict__ join) {
    for (uint64_t x = (uint64_t) blockIdx.x * ST_BLOCK + threadIdx.x; x < E; x += (uint64_t) gridDim.x * ST_BLOCK) {
        const int32_t j = end_entry[x];
        uint32_t y = CHAIN_NONE;
        int32_t ol = 0;
        uint8_t mm = 0;
        if (j >= 0 && (o.state[j] & ST_J_STITCHED)) {
            const uint32_t a = en.a[j];
            y = a == (uint32_t) x ? en.b[j] : a; ol = o.olen[j]; mm = o.mm[j];
        }
        const bool joined = y != CHAIN_NONE;
        join[x] = y;
        eo.partner[x] = joined ? (int32_t) y : -1; eo.olen[x] = ol; eo.mm[x] = mm; eo.hits[x] = joined ? 1 : 0;
        eo.state[x] = joined ? (uint8_t) (MG_E_HAS_OVERLAP | MG_E_JOINED) : (uint8_t) 0;
    }
}

__global__ void __launch_bounds__(ST_BLOCK) k_st_dropped(StEntries en, const uint32_t *__restrict__ join, uint8_t *__restrict__ state) {
    for (uint64_t j = (uint64_t) blockIdx.x * ST_BLOCK + threadIdx.x; j < en.J; j += (uint64_t) gridDim.x * ST_BLOCK) {
        const uint8_t st = state[j];
        if ((st & ST_J_STITCHED) && join[en.a[j]] == CHAIN_NONE) state[j] = (uint8_t) ((st & ~ST_J_STITCHED) | ST_J_DROPPED_CYCLE);
    }
}

}  // namespace

void launch_st_targets(const uint32_t *col_off, uint32_t T, unsigned long long *begin, int32_t *len, uint32_t max_blocks, hipStream_t s) {
    if (T) hipLaunchKernelGGL(k_st_targets, dim3(stage_grid(T, ST_BLOCK, max_blocks)), dim3(ST_BLOCK), 0, s, col_off, T, begin, len);
}

void launch_st_check(const StEntries &en, uint32_t T, uint32_t *end_count, int32_t *end_entry, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (en.J) hipLaunchKernelGGL(k_st_check, dim3(stage_grid(en.J, ST_BLOCK, max_blocks)), dim3(ST_BLOCK), 0, s, en, T, end_count, end_entry, counters);
}

void launch_st_overlap(const MgTargets &t, const StEntries &en, const StParams &p, const StEntryOut &o, unsigned long long *counters, hipStream_t s) {
    if (!en.J) return;
    const uint64_t g = ((uint64_t) en.J + ST_WAVES - 1) / ST_WAVES;
    hipLaunchKernelGGL(k_st_overlap, dim3((unsigned) std::max<uint64_t>(1, std::min<uint64_t>(g, t.max_blocks))), dim3(ST_BLOCK), 0, s, t, en, p, o, counters);
}

void launch_st_joins(const StEntries &en, const StEntryOut &o, const int32_t *end_entry, uint32_t E, const MgEndOut &eo, uint32_t *join, uint32_t max_blocks, hipStream_t s) {
    if (E) hipLaunchKernelGGL(k_st_joins, dim3(stage_grid(E, ST_BLOCK, max_blocks)), dim3(ST_BLOCK), 0, s, en, o, end_entry, E, eo, join);
}

void launch_st_dropped(const StEntries &en, const uint32_t *join, uint8_t *state, uint32_t max_blocks, hipStream_t s) {
    if (en.J) hipLaunchKernelGGL(k_st_dropped, dim3(stage_grid(en.J, ST_BLOCK, max_blocks)), dim3(ST_BLOCK), 0, s, en, join, state);
}

}  // namespace alga
