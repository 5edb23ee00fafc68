// alga_amd/csrc/grow_kernels.hip -- contig ends grown with the reads that hang over them (include/alga_amd.h: alga_grow_placed_device; the
// definition is the comment there, host side in engine_grow.hip).
//
// The 2T end sequences are gathered into one 2-bit array in a column space of their own (end e at end_off[e], the contig end at the right:
// the left ends complemented and mirrored), so the boundary problem is in one place and a left overhang is the right overhang of the twin.
// Within an end a larger overhang h is a larger first column, and the ends lie in the order of e: the tuple (mm, e, h, strand) is the
// 64-bit key (mm, first end column of the anchored part, strand), as in the placement.
//   k_gr_check        every len <= 16 * stride, columns == col_off[T] -> the refusal flags; the longest node
//   k_gr_candidates   flag per read: not PLACED and len >= min_anchor + 1; (scan); k_gr_compact: the candidates' ids, so that the hot kernel
//                     spends no wave on a placed read
//   k_gr_end_lens     W_e of every end and the indexed positions; (scan): end_off
//   k_gr_ends         the end sequences, one thread per word
//   (the index over the end columns: alga_seed_index, seed_index.hip)
//   k_gr_place        one wave per candidate, both nodes: seed_and_verify (seed_device.h) once per node over the seeds with (j + 1) k <= L - 1.
//                     A (seed j, occurrence at position q of end e) gives a = W_e - q + j k and h = L - a; only the anchored part is
//                     verified, the overhanging bases are never compared.  The minimum key and the number of placements at its mm are
//                     reduced across the wave.
//   k_gr_vote         one wave per candidate, a lane a growth column: 32-bit integer atomics into count
//   k_gr_decide       one thread per end: the leading run of passing columns, their bases, the stop reason, the counters
//   k_gr_lens         left / right / new length per target; (scan): the new col_off
//   k_gr_build        every output word gathered by one lane, from the old column array or from the growth
//   k_gr_fasta_sizes / k_gr_fasta_write   one record per target with a length, one wave per record, a lane a byte
// Block 256 and the grid caps are picked, not tuned; the launches' max_blocks lowers the cap of every grid that goes through stage_grid (the check
// keeps min(4096, cap)), of k_gr_place (whose per-wave scratch the host sizes from the capped block count) and of the FASTA write grid (option
// "grow_max_blocks": a knob of the tests, which make every grid-stride and wave-stride loop here take further passes).  k_gr_fasta_sizes has one
// thread per item and no loop: its grid is exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "grow_kernels.h"
#include "seed_device.h"
#include "text_record.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int GR_BLOCK = 256, GR_WAVES = GR_BLOCK / 64;
constexpr uint8_t GR_PL_PLACED = 1;                                    // ALGA_PLACE_PLACED

__global__ void __launch_bounds__(GR_BLOCK) k_gr_check(SeedReads r, GrTargets t, unsigned long long *__restrict__ counters) {
    unsigned long long mx = 0;
    uint32_t bad = 0;
    // every column array of the stage is sized from the caller's `columns`: it has to be the placement's
    if (blockIdx.x == 0 && threadIdx.x == 0 && (uint64_t) t.col_off[t.T] != t.columns) bad |= GR_BAD_COLUMNS;
    for (uint64_t v = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; v < 2 * r.R; v += (uint64_t) gridDim.x * GR_BLOCK) {
        const int32_t l = r.len[v];
        if (l > 0 && (unsigned long long) l > mx) mx = (unsigned long long) l;
        if ((int64_t) l > 16ll * r.stride) bad |= GR_BAD_LEN;
    }
    mx = wave_max(mx);
    for (int o = 32; o > 0; o >>= 1) bad |= (uint32_t) __shfl_xor((int) bad, o);
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(&counters[GR_MAX_LEN], mx);
        if (bad) atomicOr(&counters[GR_BAD], (unsigned long long) bad);
    }
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_candidates(SeedReads r, const uint8_t *__restrict__ pl_state, int32_t min_anchor, uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; i <= r.R; i += (uint64_t) gridDim.x * GR_BLOCK)
        flag[i] = i < r.R && !(pl_state[i] & GR_PL_PLACED) && r.len[2 * i + 1] > min_anchor ? 1u : 0u;   // entry R: the place of the scan's total
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint64_t R, uint32_t *__restrict__ cand) {
    for (uint64_t i = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; i < R; i += (uint64_t) gridDim.x * GR_BLOCK)
        if (flag[i]) cand[pos[i]] = (uint32_t) i;
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_end_lens(GrTargets t, int32_t max_len, int32_t k, int32_t *__restrict__ elen, unsigned long long *__restrict__ counters) {
    unsigned long long idx = 0, sum = 0;
    const uint64_t E = 2ull * t.T;
    for (uint64_t e = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; e <= E; e += (uint64_t) gridDim.x * GR_BLOCK) {
        int64_t w = 0;
        if (e < E) {
            const int64_t n = (int64_t) t.col_off[(e >> 1) + 1] - (int64_t) t.col_off[e >> 1];
            w = std::max<int64_t>(0, std::min<int64_t>(n, (int64_t) max_len - 1));
            if (w >= k) idx += (unsigned long long) (w - k + 1);
        }
        elen[e] = (int32_t) w;                                                // entry 2T: the place of the scan's total
        sum += (unsigned long long) w;
    }
    idx = wave_sum(idx); sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&counters[GR_END_COLUMNS], sum);
        if (idx) atomicAdd(&counters[GR_INDEX_POS], idx);
    }
}

// (after the check: columns is col_off[T]; W_e <= the target's length, so every source column lies in its target)
__global__ void __launch_bounds__(GR_BLOCK) k_gr_ends(GrTargets t, GrEnds e, uint32_t *__restrict__ ecols) {
    packed_words_body<GR_BLOCK>(e.off, e.n, e.columns, (e.columns + 15) >> 4, ecols, [&](uint32_t ee, uint32_t q) {
        const uint32_t tt = ee >> 1, W = (uint32_t) e.len[ee];
        if (ee & 1u) return base_at(t.cols, (uint64_t) t.col_off[tt + 1] - W + q);             // the last W bases
        return 3u - base_at(t.cols, (uint64_t) t.col_off[tt] + (W - 1u - q));                  // the first W, complemented and mirrored
    });
}

// Geometry of a read of L bases on the ends: seed js at position q of end e puts v[js k] on E[q], so v[a], a = W_e - q + js k, is the first
// base behind the end; the anchored part begins at column end_off[e] + W_e - a >= end_off[e]
struct GrGeometry {
    static constexpr int kMmShift = 33;              // the key: (mm << 33) | (first end column of the anchored part << 1) | strand
    const GrEnds &en;
    int k, L, min_anchor, strand;
    __device__ __forceinline__ bool operator()(int js, uint32_t g, uint32_t &gp, int &n, unsigned long long &low) const {
        const uint32_t ee = item_of(en.off, en.n, g);
        const long long W = en.len[ee], q = (long long) g - (long long) en.off[ee];
        const long long a = W - q + (long long) js * k;
        if (a > W || a < (long long) min_anchor || a > (long long) L - 1) return false;
        gp = g - (uint32_t) (js * k); n = (int) a;
        low = ((unsigned long long) gp << 1) | (unsigned long long) strand;
        return true;
    }
};

__global__ void __launch_bounds__(GR_BLOCK) k_gr_place(SeedReads rd, const uint32_t *__restrict__ cand, uint64_t n_cand, GrEnds en, SeedIndex x, int32_t k, uint32_t max_mm,
                                                       uint32_t max_occ, int32_t min_anchor, GrOut o, unsigned long long *__restrict__ scratch, uint32_t scratch_words,
                                                       unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t) blockIdx.x * GR_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * GR_WAVES;
    unsigned long long *ub = scratch + wave * (uint64_t) scratch_words;
    unsigned long long n_hang = 0, n_vote = 0, n_sat = 0, n_seeds = 0, n_over = 0;            // wave-uniform
    for (uint64_t ci0 = wave; ci0 < n_cand; ci0 += n_waves) {
        const uint64_t r = cand[ci0];
        const int32_t L = rd.len[2 * r + 1];                 // >= min_anchor + 1 >= k + 1
        unsigned long long best = ~0ull;                     // of this lane's placements
        MinMmTally tally;
        for (int strand = 0; strand < 2; strand++) {
            const RowQuery q{rd.rows + (2 * r + (strand == 0 ? 1u : 0u)) * (size_t) rd.stride, blocks_of(L), k};
            // the seeds with (j + 1) k <= L - 1: no other lies in an anchored part
            seed_and_verify(x, en.cols, k, max_mm, max_occ, (L - 1) / k, q, GrGeometry{en, k, L, min_anchor, strand}, ub, best, tally, n_seeds, n_over);
        }
        const unsigned long long win = wave_min_u64(best);
        int32_t e_out = -1, h_out = 0;
        uint8_t mm8 = 0, hits8 = 0, st8 = 0;
        if (win != ~0ull) {
            const uint32_t bmm = (uint32_t) (win >> 33), gp = (uint32_t) (win >> 1);
            const unsigned long long hits = wave_sum(tally.mm == bmm ? (unsigned long long) tally.cnt : 0ull);
            const uint32_t ee = item_of(en.off, en.n, gp);
            const int32_t a = (int32_t) (en.off[ee] + (uint32_t) en.len[ee] - gp);
            e_out = (int32_t) ee; h_out = L - a; mm8 = (uint8_t) bmm; hits8 = (uint8_t) (hits > 255ull ? 255ull : hits);
            st8 = (uint8_t) (GR_ST_OVERHANGS | (hits == 1ull ? GR_ST_VOTES : 0) | ((win & 1ull) ? GR_ST_MINUS : 0));
            n_hang++; n_vote += hits == 1ull; n_sat += hits > 255ull;
        }
        if (lane == 0) { o.end[r] = e_out; o.over[r] = h_out; o.mm[r] = mm8; o.hits[r] = hits8; o.state[r] = st8; }
    }
    if (lane == 0) {
        if (n_hang) atomicAdd(&counters[GR_OVERHANGING], n_hang);
        if (n_vote) atomicAdd(&counters[GR_VOTING], n_vote);
        if (n_sat) atomicAdd(&counters[GR_SATURATED], n_sat);
        if (n_seeds) atomicAdd(&counters[GR_SEEDS], n_seeds);
        if (n_over) atomicAdd(&counters[GR_SEEDS_OVER], n_over);
    }
}

// (a voting read has 1 <= h <= L - min_anchor and its end e < 2T from k_gr_place: base L - h + i < L lies in its row, the count entry in end e's slice)
__global__ void __launch_bounds__(GR_BLOCK) k_gr_vote(SeedReads rd, const uint32_t *__restrict__ cand, uint64_t n_cand, GrOut o, int32_t max_grow, uint32_t *__restrict__ count,
                                                      uint32_t *__restrict__ voters) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t) blockIdx.x * GR_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * GR_WAVES;
    for (uint64_t ci = wave; ci < n_cand; ci += n_waves) {
        const uint64_t r = cand[ci];
        const uint8_t st = o.state[r];
        if (!(st & GR_ST_VOTES)) continue;
        const int32_t L = rd.len[2 * r + 1], h = o.over[r], n = h < max_grow ? h : max_grow;
        const uint64_t e = (uint64_t) o.end[r];
        const uint32_t *row = rd.rows + (2 * r + ((st & GR_ST_MINUS) ? 0u : 1u)) * (size_t) rd.stride;
        if (lane == 0) atomicAdd(&voters[e], 1u);
        for (int32_t i = lane; i < n; i += 64) atomicAdd(&count[(e * (uint64_t) max_grow + (uint64_t) i) * 4ull + base_at(row, (uint64_t) (L - h + i))], 1u);
    }
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_decide(const uint32_t *__restrict__ count, const uint32_t *__restrict__ voters, uint32_t E, int32_t max_grow,
                                                        uint32_t min_cover, uint32_t min_percent, uint32_t *__restrict__ x, uint8_t *__restrict__ g,
                                                        uint8_t *__restrict__ stop, unsigned long long *__restrict__ counters) {
    unsigned long long n_voters = 0, n_grown = 0, added = 0, longest = 0, s_cover = 0, s_percent = 0, s_max = 0;
    for (uint64_t e = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; e < E; e += (uint64_t) gridDim.x * GR_BLOCK) {
        const uint4 *c4 = reinterpret_cast<const uint4 *>(count) + e * (uint64_t) max_grow;
        uint8_t *ge = g + e * (uint64_t) max_grow;
        uint32_t i = 0, why = 2;
        for (; i < (uint32_t) max_grow; i++) {
            const uint4 c = c4[i];
            uint32_t w = 0, top = c.x;
            if (c.y > top) { top = c.y; w = 1; }
            if (c.z > top) { top = c.z; w = 2; }
            if (c.w > top) { top = c.w; w = 3; }
            const unsigned long long cover = (unsigned long long) c.x + c.y + c.z + c.w;
            if (cover < (unsigned long long) min_cover) { why = 0; break; }
            if (100ull * top < (unsigned long long) min_percent * cover) { why = 1; break; }
            ge[i] = (uint8_t) w;
        }
        x[e] = i; stop[e] = (uint8_t) why;
        n_voters += voters[e] > 0; n_grown += i > 0; added += i; longest = i > longest ? i : longest;
        s_cover += why == 0; s_percent += why == 1; s_max += why == 2;
    }
    n_voters = wave_sum(n_voters); n_grown = wave_sum(n_grown); added = wave_sum(added); longest = wave_max(longest);
    s_cover = wave_sum(s_cover); s_percent = wave_sum(s_percent); s_max = wave_sum(s_max);
    if ((threadIdx.x & 63) == 0) {
        if (n_voters) atomicAdd(&counters[GR_ENDS_VOTERS], n_voters);
        if (n_grown) { atomicAdd(&counters[GR_ENDS_GROWN], n_grown); atomicAdd(&counters[GR_ADDED], added); atomicMax(&counters[GR_LONGEST_GROWTH], longest); }
        if (s_cover) atomicAdd(&counters[GR_STOPS_COVER], s_cover);
        if (s_percent) atomicAdd(&counters[GR_STOPS_PERCENT], s_percent);
        if (s_max) atomicAdd(&counters[GR_STOPS_MAX], s_max);
    }
}

__global__ void __launch_bounds__(GR_BLOCK) k_gr_lens(GrTargets t, const uint32_t *__restrict__ x, uint32_t *__restrict__ left, uint32_t *__restrict__ right,
                                                      int32_t *__restrict__ newlen, unsigned long long *__restrict__ counters) {
    unsigned long long sum = 0, longest = 0, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; i <= t.T; i += (uint64_t) gridDim.x * GR_BLOCK) {
        unsigned long long n = 0;
        if (i < t.T) {
            const uint32_t l = x[2 * i], r = x[2 * i + 1];
            n = (unsigned long long) (t.col_off[i + 1] - t.col_off[i]) + l + r;
            left[i] = l; right[i] = r;
            if (n > 0x7FFFFFFFull) { bad = 1; n = 0; }
        }
        newlen[i] = (int32_t) n;                                               // entry T: the place of the scan's total
        sum += n; longest = n > longest ? n : longest;
    }
    sum = wave_sum(sum); longest = wave_max(longest); bad = wave_max(bad);
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&counters[GR_COLUMNS_AFTER], sum);
        if (longest) atomicMax(&counters[GR_LONGEST], longest);
        if (bad) atomicMax(&counters[GR_BAD_NEWLEN], bad);
    }
}

// (new_off is the scan of the old lengths + left + right, new_columns its total: a column of target t lies in its left growth, in the old
// target or in its right growth, and left[t] / the rest below x <= max_grow)
__global__ void __launch_bounds__(GR_BLOCK) k_gr_build(GrTargets t, const uint32_t *__restrict__ new_off, uint64_t new_columns, const uint32_t *__restrict__ left,
                                                       const uint8_t *__restrict__ g, int32_t max_grow, uint32_t *__restrict__ words, unsigned long long *__restrict__ begin) {
    for (uint64_t i = (uint64_t) blockIdx.x * GR_BLOCK + threadIdx.x; i < t.T; i += (uint64_t) gridDim.x * GR_BLOCK) begin[i] = new_off[i];
    packed_words_body<GR_BLOCK>(new_off, t.T, new_columns, ((new_columns + 15) >> 4) + 2, words, [&](uint32_t tt, uint64_t q) -> uint32_t {
        const uint64_t l = left[tt], n = (uint64_t) t.col_off[tt + 1] - t.col_off[tt];
        if (q < l) return 3u - g[(2ull * tt) * (uint64_t) max_grow + (l - 1 - q)];
        if (q < l + n) return base_at(t.cols, (uint64_t) t.col_off[tt] + (q - l));
        return g[(2ull * tt + 1) * (uint64_t) max_grow + (q - l - n)];
    });
}

// ---- FASTA of the grown targets --------------------------------------------------------------------------------------------------------
// `>contig_id=<t>_length=<len>_left=<xl>_right=<xr>\n<target>\n`
struct GrRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const GrFasta &f, uint64_t j) {
        const int32_t len = f.len[j];
        if (len <= 0) return false;
        contig_head(j, (uint32_t) len);
        h.f[2] = text_field("_left=", (uint64_t) f.left[j]); h.f[3] = text_field("_right=", (uint64_t) f.right[j]); seal();
        seq.row = f.words; seq.q0 = f.col_off[j];
        return true;
    }
};

__global__ void __launch_bounds__(GR_BLOCK) k_gr_fasta_sizes(GrFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<GrRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(GR_BLOCK) k_gr_fasta_write(GrFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<GrRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_gr_check(const SeedReads &r, const GrTargets &t, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_gr_check, dim3(stage_grid(2 * r.R, GR_BLOCK, std::min<uint64_t>(4096, t.max_blocks))), dim3(GR_BLOCK), 0, s, r, t, counters);
}

void launch_gr_candidates(const SeedReads &r, const uint8_t *pl_state, int32_t min_anchor, uint32_t *flag, uint32_t max_blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_gr_candidates, dim3(stage_grid(r.R + 1, GR_BLOCK, max_blocks)), dim3(GR_BLOCK), 0, s, r, pl_state, min_anchor, flag);
}

void launch_gr_compact(const uint32_t *flag, const uint32_t *pos, uint64_t R, uint32_t *cand, uint32_t max_blocks, hipStream_t s) {
    if (R) hipLaunchKernelGGL(k_gr_compact, dim3(stage_grid(R, GR_BLOCK, max_blocks)), dim3(GR_BLOCK), 0, s, flag, pos, R, cand);
}

void launch_gr_end_lens(const GrTargets &t, int32_t max_len, int32_t k, int32_t *elen, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_gr_end_lens, dim3(stage_grid(2ull * t.T + 1, GR_BLOCK, t.max_blocks)), dim3(GR_BLOCK), 0, s, t, max_len, k, elen, counters);
}

void launch_gr_ends(const GrTargets &t, const GrEnds &e, uint32_t *ecols, hipStream_t s) {
    if (e.columns) hipLaunchKernelGGL(k_gr_ends, dim3(stage_grid((e.columns + 15) >> 4, GR_BLOCK, t.max_blocks)), dim3(GR_BLOCK), 0, s, t, e, ecols);
}

void launch_gr_place(const SeedReads &r, const uint32_t *cand, uint64_t n_cand, const GrEnds &e, const SeedIndex &x, int32_t k, int32_t max_mm, int32_t max_occ,
                     int32_t min_anchor, const GrOut &o, unsigned long long *scratch, uint32_t scratch_words_per_wave, int blocks, unsigned long long *counters,
                     hipStream_t s) {
    if (n_cand) hipLaunchKernelGGL(k_gr_place, dim3((unsigned) blocks), dim3(GR_BLOCK), 0, s, r, cand, n_cand, e, x, k, (uint32_t) max_mm, (uint32_t) max_occ, min_anchor, o,
                                   scratch, scratch_words_per_wave, counters);
}

void launch_gr_vote(const SeedReads &r, const uint32_t *cand, uint64_t n_cand, const GrOut &o, int32_t max_grow, uint32_t *count, uint32_t *voters, uint32_t max_blocks,
                    hipStream_t s) {
    if (n_cand) hipLaunchKernelGGL(k_gr_vote, dim3(stage_grid(n_cand * 64, GR_BLOCK, max_blocks)), dim3(GR_BLOCK), 0, s, r, cand, n_cand, o, max_grow, count, voters);
}

void launch_gr_decide(const uint32_t *count, const uint32_t *voters, uint32_t E, int32_t max_grow, int32_t min_cover, int32_t min_percent, uint32_t *x, uint8_t *g,
                      uint8_t *stop, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (E) hipLaunchKernelGGL(k_gr_decide, dim3(stage_grid(E, GR_BLOCK, max_blocks)), dim3(GR_BLOCK), 0, s, count, voters, E, max_grow, (uint32_t) min_cover, (uint32_t) min_percent, x, g, stop, counters);
}

void launch_gr_lens(const GrTargets &t, const uint32_t *x, uint32_t *left, uint32_t *right, int32_t *newlen, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_gr_lens, dim3(stage_grid((uint64_t) t.T + 1, GR_BLOCK, t.max_blocks)), dim3(GR_BLOCK), 0, s, t, x, left, right, newlen, counters);
}

void launch_gr_build(const GrTargets &t, const uint32_t *new_off, uint64_t new_columns, const uint32_t *left, const uint8_t *g, int32_t max_grow, uint32_t *words,
                     unsigned long long *begin, hipStream_t s) {
    const uint64_t n_words = ((new_columns + 15) >> 4) + 2;
    hipLaunchKernelGGL(k_gr_build, dim3(stage_grid(std::max<uint64_t>(n_words, t.T), GR_BLOCK, t.max_blocks)), dim3(GR_BLOCK), 0, s, t, new_off, new_columns, left, g, max_grow, words, begin);
}

void launch_gr_fasta_sizes(const GrFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_gr_fasta_sizes, dim3(text_sizes_blocks(f.n, GR_BLOCK)), dim3(GR_BLOCK), 0, s, f, sizes, counters);
}

void launch_gr_fasta_write(const GrFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_gr_fasta_write, dim3(text_write_blocks(i0, i1, GR_WAVES, f.max_blocks)), dim3(GR_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
