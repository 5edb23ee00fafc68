// alga_amd/csrc/merge_kernels.hip -- contigs whose ends overlap merged into one sequence (include/alga_amd.h: alga_merge_targets_device; the
// definition is the comment there, host side in engine_merge.hip).
//
// The 2T end sequences are gathered into one padded 2-bit array in a column space of their own (end x at end_off[x], a multiple of 16, the
// contig end at the right: the left ends complemented and mirrored), and next to it their reverse complements P_x at the same columns: an
// overlap of o bases is P_x[0 .. o) laid on the last o columns of E_y, whatever the pairing of left and right ends.  Integer work only,
// wave-64, nothing depends on thread order or on the sort's order among equal keys.
//   k_mg_check        a negative length -> the refusal flag; the column sum
//   k_mg_end_lens     W_x of every end, W_x rounded up to a word, the indexed positions; (scan): end_off
//   k_mg_ends         E_x and P_x, one thread per word
//   (the index over the end columns: alga_seed_index, seed_index.hip)
//   k_mg_overlap      one wave per end: seed_and_verify (seed_device.h) over the at most 64 seeds of P_x, one chunk.  A hit of seed j at position q
//                     of E_y gives o = W_y - q + j k; the o bases only are verified, so every (y, o) counts once.  The minimum key
//                     (mm, y, o descending) and the number of (y, o) are reduced across the wave.
//   k_mg_joins        one thread per end: joined where both ends have one overlap, each other, at one o
//   k_mg_cycle_drop / k_mg_rank_init / k_mg_place / k_mg_layout   the joins turned into ordered, oriented paths by the chain core (chain_kernels.h;
//                     these four instantiate chain_device.h): a dropped join loses JOINED and gets DROPPED_CYCLE on both ends, a state weighs len -
//                     overlap; start, overlap_after and the join counters; the 32-bit merged lengths (a flag for one above 2^31 - 1), count and sum
//   k_mg_build        every output word gathered by one lane: a column finds its member by bisection over the starts, an overlapped column is
//                     the earlier contig's; minus-oriented members complemented and mirrored
//   k_mg_fasta_sizes / k_mg_fasta_write   one record per merged contig, one wave per record
// No LDS.  Block 256 and the grid caps are picked, not tuned; MgTargets::max_blocks lowers the cap of every grid that goes through stage_grid
// (option "merge_max_blocks": a knob of the tests, which make every grid-stride loop here take further passes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "merge_kernels.h"
#include "seed_device.h"
#include "text_record.h"
#include "chain_device.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int MG_BLOCK = 256, MG_WAVES = MG_BLOCK / 64;
static_assert(MG_BLOCK == CHAIN_BLOCK, "the bodies of chain_device.h stride by CHAIN_BLOCK");

__global__ void __launch_bounds__(MG_BLOCK) k_mg_check(MgTargets t, unsigned long long *__restrict__ counters) {
    unsigned long long sum = 0, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * MG_BLOCK + threadIdx.x; i < t.T; i += (uint64_t) gridDim.x * MG_BLOCK) {
        const int32_t n = t.len[i];
        if (n < 0) bad = MG_BAD_LEN; else sum += (unsigned long long) n;
    }
    sum = wave_sum(sum); bad = wave_max(bad);
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&counters[MG_COLUMNS], sum);
        if (bad) atomicOr(&counters[MG_BAD], bad);
    }
}

// (after the check: no length is negative)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_end_lens(MgTargets t, int32_t max_overlap, int32_t min_overlap, int32_t k, int32_t *__restrict__ elen,
                                                          uint32_t *__restrict__ epad, unsigned long long *__restrict__ counters) {
    unsigned long long idx = 0, sum = 0, ends = 0;
    const uint64_t E = 2ull * t.T;
    for (uint64_t x = (uint64_t) blockIdx.x * MG_BLOCK + threadIdx.x; x <= E; x += (uint64_t) gridDim.x * MG_BLOCK) {
        int32_t w = 0;
        if (x < E) {
            w = std::min(t.len[x >> 1] >> 1, max_overlap);
            if (w >= k) idx += (unsigned long long) (w - k + 1);
            ends += w >= min_overlap;
        }
        const uint32_t pad = ((uint32_t) w + 15u) & ~15u;
        elen[x] = w; epad[x] = pad;                                           // entry 2T: the place of the scan's total
        sum += pad;
    }
    idx = wave_sum(idx); sum = wave_sum(sum); ends = wave_sum(ends);
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&counters[MG_END_COLUMNS], sum);
        if (idx) atomicAdd(&counters[MG_INDEX_POS], idx);
        if (ends) atomicAdd(&counters[MG_ENDS], ends);
    }
}

// (every end begins a word, so a word lies in one end; W_x <= len / 2: every source base lies in its target)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_ends(MgTargets t, MgEnds e, uint32_t *__restrict__ ecols, uint32_t *__restrict__ pcols) {
    const uint64_t n_words = e.columns >> 4;
    for (uint64_t w = (uint64_t) blockIdx.x * MG_BLOCK + threadIdx.x; w < n_words; w += (uint64_t) gridDim.x * MG_BLOCK) {
        const uint32_t g0 = (uint32_t) (w << 4), x = item_of(e.off, e.n, g0), tt = x >> 1, q0 = g0 - e.off[x], W = (uint32_t) e.len[x];
        const uint64_t b0 = t.begin[tt], n = (uint64_t) t.len[tt];
        uint32_t ve = 0, vp = 0;
        for (uint32_t j = 0; j < 16 && q0 + j < W; j++) {
            const uint32_t q = q0 + j;
            uint32_t be, bp;
            if (x & 1u) { be = base_at(t.words, b0 + n - W + q); bp = 3u - base_at(t.words, b0 + n - 1u - q); }          // the last W bases
            else { be = 3u - base_at(t.words, b0 + (W - 1u - q)); bp = base_at(t.words, b0 + q); }                       // the first W, complemented and mirrored
            ve |= be << (2 * j); vp |= bp << (2 * j);
        }
        ecols[w] = ve; pcols[w] = vp;
    }
}

// Query: P_x, which begins a word of pcols at column x0
struct MgQuery {
    const uint32_t *pcols, *row;
    uint32_t x0;
    int k;
    __device__ __forceinline__ unsigned long long kmer(int j) const { return col_kmer(pcols, x0 + (uint32_t) (j * k), k); }
};

// Geometry of P_x on the ends: seed js at position q of E_y puts P_x[js k] on E_y[q], and the overlap of o = W_y - q + js k bases ends with
// E_y: it begins at column end_off[y] + W_y - o >= end_off[y]
struct MgGeometry {
    static constexpr int kMmShift = 45;              // the key: (mm, y, o descending); o <= 4096
    const MgEnds &en;
    uint32_t x;
    int k, W, min_overlap;
    __device__ __forceinline__ bool operator()(int js, uint32_t g, uint32_t &gp, int &n, unsigned long long &low) const {
        const uint32_t y = item_of(en.off, en.n, g);
        if ((y >> 1) == (x >> 1)) return false;              // the same target: no overlap here
        const int32_t Wy = en.len[y], q = (int32_t) (g - en.off[y]);
        const int32_t o = Wy - q + js * k;
        if (o < min_overlap || o > W || o > Wy) return false;
        gp = g - (uint32_t) (js * k); n = o;
        low = ((unsigned long long) y << 13) | (unsigned long long) ((uint32_t) MG_MAX_OVERLAP - (uint32_t) o);
        return true;
    }
};

// Tally: every (y, o) of the lane
struct MgTally {
    uint32_t cnt = 0;
    __device__ __forceinline__ void add(uint32_t) { cnt++; }
};

__global__ void __launch_bounds__(MG_BLOCK) k_mg_overlap(MgEnds en, SeedIndex ix, int32_t k, uint32_t max_mm, uint32_t max_occ, int32_t min_overlap, MgEndOut out,
                                                         unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t) blockIdx.x * MG_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * MG_WAVES;
    unsigned long long n_with = 0, n_amb = 0, n_sat = 0, n_seeds = 0, n_over = 0;            // wave-uniform
    for (uint64_t x = wave; x < en.n; x += n_waves) {
        const int32_t W = en.len[x];
        unsigned long long best = ~0ull;
        MgTally tally;
        if (W >= min_overlap) {                              // (wave-uniform) a shorter end has no overlap: o <= W
            const uint32_t x0 = en.off[x];
            const int S = W / k;                             // the seeds with (j + 1) k <= W
            __builtin_assume(S >= 1 && S <= 64);             // (k <= min_overlap <= W <= max_overlap <= 64 k: one chunk, the scratch is never touched)
            seed_and_verify(ix, en.cols, k, max_mm, max_occ, S, MgQuery{en.pcols, en.pcols + (x0 >> 4), x0, k}, MgGeometry{en, (uint32_t) x, k, W, min_overlap}, nullptr,
                            best, tally, n_seeds, n_over);
        }
        const unsigned long long win = wave_min_u64(best);
        int32_t y_out = -1, o_out = 0;
        uint8_t mm8 = 0, hits8 = 0, st8 = 0;
        if (win != ~0ull) {
            const unsigned long long hits = wave_sum((unsigned long long) tally.cnt);
            y_out = (int32_t) (uint32_t) (win >> 13); o_out = MG_MAX_OVERLAP - (int32_t) (win & 8191ull); mm8 = (uint8_t) (win >> 45);
            hits8 = (uint8_t) (hits > 255ull ? 255ull : hits);
            st8 = (uint8_t) (MG_E_HAS_OVERLAP | (hits > 1ull ? MG_E_AMBIGUOUS : 0));
            n_with++; n_amb += hits > 1ull; n_sat += hits > 255ull;
        }
        if (lane == 0) { out.partner[x] = y_out; out.olen[x] = o_out; out.mm[x] = mm8; out.hits[x] = hits8; out.state[x] = st8; }
    }
    if (lane == 0) {
        if (n_with) atomicAdd(&counters[MG_WITH_OVERLAP], n_with);
        if (n_amb) atomicAdd(&counters[MG_AMBIGUOUS], n_amb);
        if (n_sat) atomicAdd(&counters[MG_SATURATED], n_sat);
        if (n_seeds) atomicAdd(&counters[MG_SEEDS], n_seeds);
        if (n_over) atomicAdd(&counters[MG_SEEDS_OVER], n_over);
    }
}

// (a thread writes its own end only; partner[x] < 2T wherever hits[x] > 0)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_joins(MgEndOut o, uint32_t E, uint32_t *__restrict__ join) {
    for (uint64_t x = (uint64_t) blockIdx.x * MG_BLOCK + threadIdx.x; x < E; x += (uint64_t) gridDim.x * MG_BLOCK) {
        uint32_t j = CHAIN_NONE;
        if (o.hits[x] == 1) {
            const uint32_t y = (uint32_t) o.partner[x];
            if (o.hits[y] == 1 && (uint32_t) o.partner[y] == (uint32_t) x && o.olen[y] == o.olen[x]) j = y;
        }
        join[x] = j;
        if (j != CHAIN_NONE) o.state[x] |= MG_E_JOINED;
    }
}

__global__ void __launch_bounds__(MG_BLOCK) k_mg_cycle_drop(ChainLists l, uint32_t T, uint32_t *__restrict__ join, uint8_t *__restrict__ end_state,
                                                            unsigned long long *__restrict__ counters) {
    chain_cycle_drop_body(l, T, join, [=](uint64_t x, uint32_t y) {
        end_state[x] = (uint8_t) ((end_state[x] & ~MG_E_JOINED) | MG_E_DROPPED_CYCLE);
        end_state[y] = (uint8_t) ((end_state[y] & ~MG_E_JOINED) | MG_E_DROPPED_CYCLE);
    }, &counters[MG_DROPPED]);
}

// (a joined end has 42 <= olen <= len / 2: len - olen > 0)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_rank_init(MgTargets t, const uint32_t *__restrict__ join, const int32_t *__restrict__ olen, ChainLists l) {
    chain_rank_init_body(join, 2ull * t.T, l, [=](uint32_t x, bool joined) { return (unsigned long long) (t.len[x >> 1] - (joined ? olen[x ^ 1u] : 0)); });
}

__global__ void __launch_bounds__(MG_BLOCK) k_mg_place(MgTargets t, ChainLists l, const uint32_t *__restrict__ join, MgEndOut eo, MgLayout o, uint32_t *__restrict__ head,
                                                       uint32_t *__restrict__ first, uint32_t *__restrict__ members, unsigned long long *__restrict__ counters) {
    unsigned long long n_joins = 0, n_mm = 0, n_removed = 0, longest = 0;
    for (uint64_t c = (uint64_t) blockIdx.x * MG_BLOCK + threadIdx.x; c <= t.T; c += (uint64_t) gridDim.x * MG_BLOCK) {
        if (c == t.T) { first[c] = 0; members[c] = 0; continue; }               // the place of the scans' totals
        if (t.len[c] == 0) {                                                   // in no merged contig (it has no end sequence: no join)
            o.merged[c] = -1; o.rank[c] = -1; o.orient[c] = 0; o.start[c] = 0; o.overlap_after[c] = 0;
            head[c] = (uint32_t) c; first[c] = 0; members[c] = 0;
            continue;
        }
        const ChainPos p = chain_position(l, (uint32_t) c);
        const bool joined = join[p.out] != CHAIN_NONE;
        const uint32_t ov = joined ? (uint32_t) eo.olen[p.out] : 0u;
        o.rank[c] = (int32_t) p.rank; o.orient[c] = (uint8_t) p.e;
        o.start[c] = (uint32_t) (l.wsum[p.hx] - l.wsum[p.x]);
        o.overlap_after[c] = (int32_t) ov;
        if (joined) { n_joins++; n_mm += eo.mm[p.out]; n_removed += ov; longest = ov > longest ? ov : longest; }
        head[c] = p.hx >> 1; first[c] = p.rank == 0; members[c] = p.rank == 0 ? p.m : 0u;
    }
    n_joins = wave_sum(n_joins); n_mm = wave_sum(n_mm); n_removed = wave_sum(n_removed); longest = wave_max(longest);
    if ((threadIdx.x & 63) == 0 && n_joins) {
        atomicAdd(&counters[MG_JOINS], n_joins); atomicAdd(&counters[MG_REMOVED], n_removed); atomicMax(&counters[MG_LONGEST_OVERLAP], longest);
        if (n_mm) atomicAdd(&counters[MG_JOIN_MM], n_mm);
    }
}

__global__ void __launch_bounds__(MG_BLOCK) k_mg_layout(MgTargets t, ChainLists l, const uint32_t *__restrict__ head, const uint32_t *__restrict__ first_scan,
                                                        const uint32_t *__restrict__ members_scan, MgLayout o, unsigned long long *__restrict__ counters) {
    unsigned long long n_mg = 0, n_multi = 0, n_mem = 0, longest = 0, sum = 0, bad = 0;
    chain_layout_body(l, t.T, o.rank, o.orient, head, first_scan, members_scan, o.merged, o.m_off, o.m_members,
                      [&](uint32_t, uint32_t mid, uint32_t, unsigned long long bases, uint32_t members) {      // the 32-bit length: one above 2^31 - 1 is refused
                          if (bases > 0x7FFFFFFFull) { bad = 1; bases = 0; }
                          o.m_len[mid] = (int32_t) bases;
                          n_mg++; n_multi += members > 1u; n_mem += members; sum += bases;
                          longest = bases > longest ? bases : longest;
                      });
    bad = wave_max(bad); n_mg = wave_sum(n_mg); n_multi = wave_sum(n_multi); n_mem = wave_sum(n_mem); longest = wave_max(longest); sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && n_mg) {
        atomicAdd(&counters[MG_MERGED], n_mg); atomicAdd(&counters[MG_MEMBERS], n_mem); atomicMax(&counters[MG_LONGEST], longest);
        atomicAdd(&counters[MG_COLUMNS_AFTER], sum);
        if (n_multi) atomicAdd(&counters[MG_MULTI], n_multi);
        if (bad) atomicMax(&counters[MG_BAD_MERGED_LEN], bad);
    }
}

// (col_off is the scan of the merged lengths, columns its total; every merged contig has a length and at least one member; a column of a member
// lies in that member's target: p - start < len)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_build(MgTargets t, MgLayout o, const uint32_t *__restrict__ col_off, uint32_t n_merged, uint64_t columns,
                                                       uint32_t *__restrict__ words, unsigned long long *__restrict__ begin) {
    for (uint64_t i = (uint64_t) blockIdx.x * MG_BLOCK + threadIdx.x; i < n_merged; i += (uint64_t) gridDim.x * MG_BLOCK) begin[i] = col_off[i];
    packed_words_body<MG_BLOCK>(col_off, n_merged, columns, ((columns + 15) >> 4) + 2, words, [&](uint32_t j, uint32_t p) {
        const uint32_t m0 = o.m_off[j], m = o.m_off[j + 1] - m0;
        const int32_t *mem = o.m_members + m0;
        uint32_t lo = 0, hi = m;                                             // the member of largest rank that starts at or before p
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (o.start[mem[mid]] <= p) lo = mid; else hi = mid;
        }
        uint32_t c = (uint32_t) mem[lo];
        if (lo > 0) {                                                        // an overlapped column is the earlier contig's
            const uint32_t cp = (uint32_t) mem[lo - 1];
            if (p < o.start[cp] + (uint32_t) t.len[cp]) c = cp;
        }
        const uint32_t q = p - o.start[c], n = (uint32_t) t.len[c];
        return o.orient[c] ? 3u - base_at(t.words, t.begin[c] + (n - 1u - q)) : base_at(t.words, t.begin[c] + q);
    });
}

// ---- FASTA of the merged contigs -------------------------------------------------------------------------------------------------------
// `>contig_id=<j>_length=<len>_contigs=<m>\n<merged contig>\n`
struct MgRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const MgFasta &f, uint64_t j) {
        const int32_t len = f.len[j];
        if (len <= 0) return false;
        contig_head(j, (uint32_t) len);
        h.f[2] = text_field("_contigs=", (uint64_t) (f.m_off[j + 1] - f.m_off[j])); seal();
        seq.row = f.words; seq.q0 = f.col_off[j];
        return true;
    }
};

__global__ void __launch_bounds__(MG_BLOCK) k_mg_fasta_sizes(MgFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<MgRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(MG_BLOCK) k_mg_fasta_write(MgFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<MgRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_mg_check(const MgTargets &t, unsigned long long *counters, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_mg_check, dim3(stage_grid(t.T, MG_BLOCK, std::min<uint64_t>(4096, t.max_blocks))), dim3(MG_BLOCK), 0, s, t, counters);
}

void launch_mg_end_lens(const MgTargets &t, int32_t max_overlap, int32_t min_overlap, int32_t k, int32_t *elen, uint32_t *epad, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_mg_end_lens, dim3(stage_grid(2ull * t.T + 1, MG_BLOCK, t.max_blocks)), dim3(MG_BLOCK), 0, s, t, max_overlap, min_overlap, k, elen, epad, counters);
}

void launch_mg_ends(const MgTargets &t, const MgEnds &e, uint32_t *ecols, uint32_t *pcols, hipStream_t s) {
    if (e.columns) hipLaunchKernelGGL(k_mg_ends, dim3(stage_grid(e.columns >> 4, MG_BLOCK, t.max_blocks)), dim3(MG_BLOCK), 0, s, t, e, ecols, pcols);
}

void launch_mg_overlap(const MgEnds &e, const SeedIndex &x, int32_t k, int32_t max_mm, int32_t max_occ, int32_t min_overlap, const MgEndOut &o, int blocks,
                       unsigned long long *counters, hipStream_t s) {
    if (e.n) hipLaunchKernelGGL(k_mg_overlap, dim3((unsigned) blocks), dim3(MG_BLOCK), 0, s, e, x, k, (uint32_t) max_mm, (uint32_t) max_occ, min_overlap, o, counters);
}

void launch_mg_joins(const MgEndOut &o, uint32_t E, uint32_t *join, uint32_t max_blocks, hipStream_t s) {
    if (E) hipLaunchKernelGGL(k_mg_joins, dim3(stage_grid(E, MG_BLOCK, max_blocks)), dim3(MG_BLOCK), 0, s, o, E, join);
}

void launch_mg_cycle_drop(const ChainLists &l, uint32_t T, uint32_t *join, uint8_t *end_state, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (T) hipLaunchKernelGGL(k_mg_cycle_drop, dim3(stage_grid(T, MG_BLOCK, max_blocks)), dim3(MG_BLOCK), 0, s, l, T, join, end_state, counters);
}

void launch_mg_rank_init(const MgTargets &t, const uint32_t *join, const int32_t *olen, const ChainLists &l, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_mg_rank_init, dim3(stage_grid(2ull * t.T, MG_BLOCK, t.max_blocks)), dim3(MG_BLOCK), 0, s, t, join, olen, l);
}

void launch_mg_place(const MgTargets &t, const ChainLists &l, const uint32_t *join, const MgEndOut &o, const MgLayout &lo, uint32_t *head, uint32_t *first, uint32_t *members,
                     unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_mg_place, dim3(stage_grid((uint64_t) t.T + 1, MG_BLOCK, t.max_blocks)), dim3(MG_BLOCK), 0, s, t, l, join, o, lo, head, first, members, counters);
}

void launch_mg_layout(const MgTargets &t, const ChainLists &l, const uint32_t *head, const uint32_t *first_scan, const uint32_t *members_scan, const MgLayout &lo,
                      unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_mg_layout, dim3(stage_grid((uint64_t) t.T + 1, MG_BLOCK, t.max_blocks)), dim3(MG_BLOCK), 0, s, t, l, head, first_scan, members_scan, lo, counters);
}

void launch_mg_build(const MgTargets &t, const MgLayout &lo, const uint32_t *col_off, uint32_t n_merged, uint64_t columns, uint32_t *words, unsigned long long *begin,
                     hipStream_t s) {
    const uint64_t n_words = ((columns + 15) >> 4) + 2;
    hipLaunchKernelGGL(k_mg_build, dim3(stage_grid(std::max<uint64_t>(n_words, n_merged), MG_BLOCK, t.max_blocks)), dim3(MG_BLOCK), 0, s, t, lo, col_off, n_merged, columns, words, begin);
}

void launch_mg_fasta_sizes(const MgFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_mg_fasta_sizes, dim3(text_sizes_blocks(f.n, MG_BLOCK)), dim3(MG_BLOCK), 0, s, f, sizes, counters);
}

void launch_mg_fasta_write(const MgFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_mg_fasta_write, dim3(text_write_blocks(i0, i1, MG_WAVES)), dim3(MG_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
