// alga_amd/csrc/polish_kernels.hip -- the placed targets voted again, by every read the placement laid over them (include/alga_amd.h:
// alga_polish_placed_device; the definition is the comment there, host side in engine_polish.hip).
//
// Everything is in the placement's COLUMN space (column g = col_off[t] + the base's index in t, 16 columns a word), so a voter is one interval
// [g0, g0 + len) of columns and the seams between targets need no case of their own: the check keeps every voter inside its target.
// Integer work only, wave-64, every output word written once, no atomics on the sequence words or the counts.
//   k_po_check      one thread per read: the refusals (a voter's length against the stride, its placement against its target; col_off[T]
//                   against the columns the caller's struct names), the voters, the sum of their lengths, the longest -> one read-back
//   k_po_keys       (first column, voting node) per read, 0xFFFFFFFF for a read without a vote: the engine's radix sort puts the voters in
//                   front, ascending by first column (the order among equal columns is free: adds commute)
//   k_po_vote       one lane per output word: a bisection for the last voter that starts before the word's end, then a walk BACKWARDS while
//                   start + longest voter > the word's first column, skipping voters that end at or before it.  Per covering voter the at most
//                   two row words are funnel-shifted to the word's 16 columns and masked to the columns covered; the four one-hot column masks
//                   are added into BIT-SLICED counters (k_cons_vote's layout: 8 planes per base, A / C in the even / odd bits of one register
//                   and G / T of another, ripple carry, exact to 255 covering voters).  The decision is taken in the same kernel: the word, a
//                   16-bit changed and a 16-bit ambiguous mask, the popcount for the scan, the optional counts as one 16-byte store per column
//   k_po_vote_wide  the words with more covering voters than that: one wave per word, lane = (column, base), a 32-bit count per lane
//   k_po_changes    one thread per word: its changed columns, ascending, at the place the exclusive scan of the popcounts gives
//   k_po_fasta_sizes / k_po_fasta_write   the records of the final FASTA, with or without the depth in the header, the sequence read from the
//                   polished column array; one wave per record
// Per-target sums as k_cons_vote's: one atomic per wave where the wave's 1024 columns lie in one target, else one per changed column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "polish_kernels.h"
#include "packed_device.h"
#include "text_record.h"

namespace alga {

namespace {

constexpr int PO_BLOCK = 256, PO_WAVES = PO_BLOCK / 64;
constexpr uint8_t PO_ST_MINUS = 4;                                      // ALGA_PLACE_MINUS
constexpr uint8_t PO_V_ACCEPTED = 2;                                    // ALGA_FINAL_ACCEPTED

__device__ __forceinline__ uint32_t po_wave_sum32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t) __shfl_xor((int) v, o);
    return v;
}
__device__ __forceinline__ uint32_t po_wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t) __shfl_xor((int) v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t po_wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t) __shfl_xor((int) v, o);
    return v;
}

__global__ void __launch_bounds__(PO_BLOCK) k_po_check(PoReads r, PoTargets t, unsigned long long *__restrict__ counters) {
    unsigned long long voters = 0, votes = 0;
    uint32_t bad = 0, mx = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && (uint64_t) t.col_off[t.T] != t.columns) bad |= PO_BAD_COLUMNS;
    for (uint64_t i = (uint64_t) blockIdx.x * PO_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * PO_BLOCK) {
        const uint8_t st = r.state[i];
        if (!(st & r.vote_bit)) continue;
        const int32_t L = r.len[2 * i + ((st & PO_ST_MINUS) ? 0u : 1u)];
        if (L < 1 || (int64_t) L > 16ll * r.stride) { bad |= PO_BAD_LEN; continue; }
        const int32_t tt = r.target[i], p = r.pos[i];
        if (tt < 0 || (uint32_t) tt >= t.T || p < 0 || (int64_t) p + L > (int64_t) t.col_off[tt + 1] - (int64_t) t.col_off[tt]) { bad |= PO_BAD_PLACE; continue; }
        voters++; votes += (unsigned long long) L;
        mx = (uint32_t) L > mx ? (uint32_t) L : mx;
    }
    voters = wave_sum(voters); votes = wave_sum(votes); mx = po_wave_max(mx); bad = po_wave_or(bad);
    if ((threadIdx.x & 63) == 0) {
        if (voters) { atomicAdd(&counters[PO_VOTERS], voters); atomicAdd(&counters[PO_VOTES], votes); atomicMax(&counters[PO_MAX_LEN], (unsigned long long) mx); }
        if (bad) atomicOr(&counters[PO_BAD], (unsigned long long) bad);
    }
}

// (after the check: every voter's target and position are in range)
__global__ void __launch_bounds__(PO_BLOCK) k_po_keys(PoReads r, PoTargets t, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    for (uint64_t i = (uint64_t) blockIdx.x * PO_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * PO_BLOCK) {
        const uint8_t st = r.state[i];
        const bool votes = st & r.vote_bit;
        keys[i] = votes ? t.col_off[r.target[i]] + (uint32_t) r.pos[i] : 0xFFFFFFFFu;
        vals[i] = (uint32_t) (2 * i) + ((st & PO_ST_MINUS) ? 0u : 1u);
    }
}

// the voters sorted by first column: the number of them that start at or before column g_end
__device__ __forceinline__ uint32_t po_upper(const uint32_t *__restrict__ keys, uint32_t n, uint64_t g_end) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t) keys[mid] <= g_end) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// rule 3 of the definition on the four counts of one column: the base the column gets, changed or ambiguous
struct PoVerdict { uint32_t base, cover; bool changed, ambiguous; };
__device__ __forceinline__ PoVerdict po_decide(const uint32_t n[4], uint32_t cur, int32_t min_cover, int32_t min_percent) {
    PoVerdict d;
    d.cover = n[0] + n[1] + n[2] + n[3];
    uint32_t best = n[0], w = 0;
    if (n[1] > best) { best = n[1]; w = 1; }
    if (n[2] > best) { best = n[2]; w = 2; }
    if (n[3] > best) { best = n[3]; w = 3; }
    const uint32_t ncur = cur == 0 ? n[0] : cur == 1 ? n[1] : cur == 2 ? n[2] : n[3];
    if (ncur == best) w = cur;                                       // a tie goes to cur, else to the smallest code
    const bool differs = w != cur && d.cover >= (uint32_t) min_cover;
    const bool enough = 100ull * (unsigned long long) best >= (unsigned long long) min_percent * (unsigned long long) d.cover;
    d.changed = differs && enough; d.ambiguous = differs && !enough;
    d.base = d.changed ? w : cur;
    return d;
}

// t_changed / t_ambiguous of the words a wave holds (lane l: word w0 + l, masks chm / amm): one atomic per wave where its columns lie in
// one target, else one per marked column
__device__ __forceinline__ void po_add_targets(const PoTargets &t, const PoVote &v, bool active, uint64_t w, uint32_t chm, uint32_t amm) {
    if (!__ballot(active && (chm | amm))) return;
    const int lane = threadIdx.x & 63;
    const uint32_t first = (uint32_t) __shfl((int) (uint32_t) (w << 4), 0);        // lane 0 holds the wave's lowest word and is active where any lane is
    const uint64_t glast = (uint64_t) first + 1023 < t.columns ? (uint64_t) first + 1023 : t.columns - 1;
    const uint32_t t0 = item_of(t.col_off, t.T, first);
    const uint32_t nc = po_wave_sum32(active ? (uint32_t) __popc(chm) : 0u), na = po_wave_sum32(active ? (uint32_t) __popc(amm) : 0u);
    if ((uint64_t) t.col_off[t0 + 1] > glast) {
        if (lane == 0) {
            if (nc) atomicAdd(&v.t_changed[t0], (unsigned long long) nc);
            if (na) atomicAdd(&v.t_ambiguous[t0], (unsigned long long) na);
        }
    } else if (active) {
        for (uint32_t m = chm; m; m &= m - 1) atomicAdd(&v.t_changed[item_of(t.col_off, t.T, (uint32_t) (w << 4) + (uint32_t) (__ffs((int) m) - 1))], 1ull);
        for (uint32_t m = amm; m; m &= m - 1) atomicAdd(&v.t_ambiguous[item_of(t.col_off, t.T, (uint32_t) (w << 4) + (uint32_t) (__ffs((int) m) - 1))], 1ull);
    }
}

__global__ void __launch_bounds__(PO_BLOCK) k_po_vote(PoReads r, PoTargets t, PoVote v, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint64_t n_words = (t.columns + 15) >> 4;
    uint32_t cover_max = 0, wide_n = 0, n_changed = 0, n_amb = 0, n_voted = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * PO_BLOCK; base < n_words; base += (uint64_t) gridDim.x * PO_BLOCK) {
        const uint64_t w = base + threadIdx.x;
        const bool active = w < n_words;
        uint32_t chm = 0, amm = 0;
        if (active) {
            const uint64_t g0 = w << 4;
            uint32_t ac[8], gt[8];                                   // plane p: bit 2 col = bit p of count(A), bit 2 col + 1 of count(C); G / T alike
#pragma unroll
            for (int p = 0; p < 8; p++) ac[p] = gt[p] = 0;
            uint32_t depth = 0;
            bool wide = false;
            for (int64_t i = (int64_t) po_upper(v.keys, v.n_voters, g0 + 15) - 1; i >= 0; i--) {
                const uint64_t start = v.keys[i];
                if (start + v.longest <= g0) break;                   // nothing before it reaches the word either
                const uint32_t node = v.vals[i];
                const int32_t l = r.len[node];
                if (start + (uint64_t) l <= g0) continue;
                if (++depth > PO_NARROW_DEPTH) { wide = true; break; }
                const int32_t q = (int32_t) ((int64_t) g0 - (int64_t) start);   // the voter's base under the word's first column (negative: it starts inside)
                const int32_t lo = q < 0 ? -q : 0, hi = l - q < 16 ? l - q : 16;     // columns [lo, hi) of the word are covered, lo < hi
                const uint32_t *row = r.rows + (uint64_t) node * (uint64_t) r.stride;
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
            if (wide) { v.pop[w] = PO_WIDE_MARK; wide_n++; }
            else {
                const uint32_t cur_word = t.cols[w];
                uint32_t word = 0;
#pragma unroll 1
                for (int col = 0; col < 16; col++) {                  // (not unrolled: the planes are shifted down instead)
                    uint32_t n[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int pl = 0; pl < 8; pl++) {
                        n[0] |= (ac[pl] & 1u) << pl; n[1] |= ((ac[pl] >> 1) & 1u) << pl;
                        n[2] |= (gt[pl] & 1u) << pl; n[3] |= ((gt[pl] >> 1) & 1u) << pl;
                        ac[pl] >>= 2; gt[pl] >>= 2;
                    }
                    // columns from n_columns on are covered by nothing: all counts 0, cur 0, no change
                    const PoVerdict d = po_decide(n, (cur_word >> (2 * col)) & 3u, v.min_cover, v.min_percent);
                    word |= d.base << (2 * col);
                    chm |= (uint32_t) d.changed << col; amm |= (uint32_t) d.ambiguous << col;
                    n_voted += d.cover >= (uint32_t) v.min_cover;
                    cover_max = d.cover > cover_max ? d.cover : cover_max;
                    if (v.counts && g0 + (uint64_t) col < t.columns) *reinterpret_cast<uint4 *>(v.counts + 4 * (g0 + (uint64_t) col)) = make_uint4(n[0], n[1], n[2], n[3]);
                }
                v.words[w] = word;
                v.marks[w] = chm | (amm << 16);
                v.pop[w] = (uint32_t) __popc(chm);
                n_changed += (uint32_t) __popc(chm); n_amb += (uint32_t) __popc(amm);
            }
        }
        po_add_targets(t, v, active, w, chm, amm);
    }
    cover_max = po_wave_max(cover_max); wide_n = po_wave_sum32(wide_n);
    n_changed = po_wave_sum32(n_changed); n_amb = po_wave_sum32(n_amb); n_voted = po_wave_sum32(n_voted);
    if (lane == 0) {
        if (cover_max) atomicMax(&counters[PO_MAX_COVER], (unsigned long long) cover_max);
        if (wide_n) atomicAdd(&counters[PO_WIDE], (unsigned long long) wide_n);
        if (n_changed) atomicAdd(&counters[PO_CHANGED], (unsigned long long) n_changed);
        if (n_amb) atomicAdd(&counters[PO_AMBIGUOUS], (unsigned long long) n_amb);
        if (n_voted) atomicAdd(&counters[PO_VOTED], (unsigned long long) n_voted);
    }
}

__global__ void __launch_bounds__(PO_BLOCK) k_po_vote_wide(PoReads r, PoTargets t, PoVote v, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63, col = lane >> 2;
    const uint32_t b = (uint32_t) lane & 3u;
    const uint64_t n_words = (t.columns + 15) >> 4, waves = (uint64_t) gridDim.x * PO_WAVES;
    uint32_t cover_max = 0;
    unsigned long long n_changed = 0, n_amb = 0, n_voted = 0;         // wave-uniform
    for (uint64_t base = ((uint64_t) blockIdx.x * PO_WAVES + (threadIdx.x >> 6)) << 6; base < n_words; base += waves << 6) {
        const uint64_t mine = base + (uint64_t) lane;
        unsigned long long todo = __ballot(mine < n_words && v.pop[mine] == PO_WIDE_MARK);
        while (todo) {
            const uint64_t w = base + (uint64_t) (__ffsll(todo) - 1);     // the same for every lane of the wave
            todo &= todo - 1;
            const uint64_t g0 = w << 4, g = g0 + (uint64_t) col;
            uint32_t count = 0;
            for (int64_t i = (int64_t) po_upper(v.keys, v.n_voters, g0 + 15) - 1; i >= 0; i--) {
                const uint64_t start = v.keys[i];
                if (start + v.longest <= g0) break;
                const uint32_t node = v.vals[i];
                const int32_t l = r.len[node];
                if (g >= start && g - start < (uint64_t) l) {
                    const uint32_t q = (uint32_t) (g - start);
                    count += ((r.rows[(uint64_t) node * (uint64_t) r.stride + (q >> 4)] >> (2 * (q & 15u))) & 3u) == b;
                }
            }
            uint32_t n[4];
#pragma unroll
            for (int k = 0; k < 4; k++) n[k] = (uint32_t) __shfl((int) count, (lane & ~3) + k);
            const uint32_t cur_word = t.cols[w];
            const PoVerdict d = po_decide(n, (cur_word >> (2 * col)) & 3u, v.min_cover, v.min_percent);
            const bool first = b == 0;                                // one lane per column speaks for it
            const uint32_t word = po_wave_or(first ? d.base << (2 * col) : 0u);
            const uint32_t chm = po_wave_or(first && d.changed ? 1u << col : 0u), amm = po_wave_or(first && d.ambiguous ? 1u << col : 0u);
            n_voted += (unsigned long long) __popcll(__ballot(first && d.cover >= (uint32_t) v.min_cover));
            cover_max = d.cover > cover_max ? d.cover : cover_max;
            if (v.counts && g < t.columns) v.counts[4 * g + b] = count;
            if (lane == 0) { v.words[w] = word; v.marks[w] = chm | (amm << 16); v.pop[w] = (uint32_t) __popc(chm); }
            n_changed += (unsigned long long) __popc(chm); n_amb += (unsigned long long) __popc(amm);
            if (lane == 0) {                                          // rare: one atomic per marked column
                for (uint32_t m = chm; m; m &= m - 1) atomicAdd(&v.t_changed[item_of(t.col_off, t.T, (uint32_t) g0 + (uint32_t) (__ffs((int) m) - 1))], 1ull);
                for (uint32_t m = amm; m; m &= m - 1) atomicAdd(&v.t_ambiguous[item_of(t.col_off, t.T, (uint32_t) g0 + (uint32_t) (__ffs((int) m) - 1))], 1ull);
            }
        }
    }
    cover_max = po_wave_max(cover_max);
    if (lane == 0) {
        if (cover_max) atomicMax(&counters[PO_MAX_COVER], (unsigned long long) cover_max);
        if (n_changed) atomicAdd(&counters[PO_CHANGED], n_changed);
        if (n_amb) atomicAdd(&counters[PO_AMBIGUOUS], n_amb);
        if (n_voted) atomicAdd(&counters[PO_VOTED], n_voted);
    }
}

__global__ void __launch_bounds__(PO_BLOCK) k_po_changes(PoTargets t, const uint32_t *__restrict__ words, const uint32_t *__restrict__ marks,
                                                         const uint32_t *__restrict__ pos, uint32_t *__restrict__ cols_out, uint8_t *__restrict__ bases_out) {
    const uint64_t n_words = (t.columns + 15) >> 4;
    for (uint64_t w = (uint64_t) blockIdx.x * PO_BLOCK + threadIdx.x; w < n_words; w += (uint64_t) gridDim.x * PO_BLOCK) {
        uint32_t m = marks[w] & 0xFFFFu;
        if (!m) continue;
        const uint32_t was = t.cols[w], now = words[w];
        for (uint32_t o = pos[w]; m; m &= m - 1, o++) {
            const uint32_t c = (uint32_t) (__ffs((int) m) - 1);
            cols_out[o] = (uint32_t) (w << 4) + c;
            bases_out[o] = (uint8_t) (((was >> (2 * c)) & 3u) | (((now >> (2 * c)) & 3u) << 2));
        }
    }
}

// ---- FASTA of the polished sequences ----------------------------------------------------------------------------------------------------
// `>contig_id=<id>_length=<L>[_reads=<n>_depth=<q>.<dd>]\n<columns col_off[id] .. col_off[id + 1])>\n`
struct PoRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const PoFasta &f, uint64_t j) {
        const uint32_t c0 = f.col_off[j], len = f.col_off[j + 1] - c0;
        if (f.verdict[(uint32_t) f.order[j]] != PO_V_ACCEPTED || !len) return false;
        contig_head(j, len);
        if (f.depth) depth(f.t_reads[j], f.t_bases[j]);
        seal();
        seq.row = f.words; seq.q0 = c0;
        return true;
    }
};

__global__ void __launch_bounds__(PO_BLOCK) k_po_fasta_sizes(PoFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<PoRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(PO_BLOCK) k_po_fasta_write(PoFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<PoRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_po_check(const PoReads &r, const PoTargets &t, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_po_check, dim3(stage_grid(r.R, PO_BLOCK, 4096)), dim3(PO_BLOCK), 0, s, r, t, counters);
}

void launch_po_keys(const PoReads &r, const PoTargets &t, uint32_t *keys, uint32_t *vals, hipStream_t s) {
    if (r.R) hipLaunchKernelGGL(k_po_keys, dim3(stage_grid(r.R, PO_BLOCK, 8192)), dim3(PO_BLOCK), 0, s, r, t, keys, vals);
}

void launch_po_vote(const PoReads &r, const PoTargets &t, const PoVote &v, unsigned long long *counters, hipStream_t s) {
    if (t.columns) hipLaunchKernelGGL(k_po_vote, dim3(stage_grid((t.columns + 15) >> 4, PO_BLOCK, 1u << 18)), dim3(PO_BLOCK), 0, s, r, t, v, counters);
}

void launch_po_vote_wide(const PoReads &r, const PoTargets &t, const PoVote &v, unsigned long long *counters, hipStream_t s) {
    // a wave takes 64 consecutive words at a time
    if (t.columns) hipLaunchKernelGGL(k_po_vote_wide, dim3(stage_grid((((t.columns + 15) >> 4) + 63) / 64 * 64, PO_BLOCK, 1u << 16)), dim3(PO_BLOCK), 0, s, r, t, v, counters);
}

void launch_po_changes(const PoTargets &t, const uint32_t *words, const uint32_t *marks, const uint32_t *pos, uint32_t *cols_out, uint8_t *bases_out, hipStream_t s) {
    if (t.columns) hipLaunchKernelGGL(k_po_changes, dim3(stage_grid((t.columns + 15) >> 4, PO_BLOCK, 1u << 16)), dim3(PO_BLOCK), 0, s, t, words, marks, pos, cols_out, bases_out);
}

void launch_po_fasta_sizes(const PoFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_po_fasta_sizes, dim3(text_sizes_blocks(f.n, PO_BLOCK)), dim3(PO_BLOCK), 0, s, f, sizes, counters);
}

void launch_po_fasta_write(const PoFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_po_fasta_write, dim3(text_write_blocks(i0, i1, PO_WAVES)), dim3(PO_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
