// alga_amd/csrc/place_kernels.hip -- every read placed on a set of target sequences, the depth of every column, the pairs (include/alga_amd.h:
// alga_place_reads_device; the definition is the comment there, host side in engine_place.hip).
//
// The targets are repacked into one 2-bit array in COLUMN space (column g in word g >> 4, g = col_off[t] + the base's index in t), so the
// boundary problem is in one place: a base index anywhere else is a column.  (t, p) ascending is the column ascending, so a placement is its
// first column and the tuple (mm, t, p, strand) one 64-bit key.
//   k_pl_node_check     pair_off is well formed; the longest node
//   k_pl_target_check   no negative target length; the columns (64-bit sum) and the indexed positions
//   k_pl_final_targets  begin / length of the windows of a final result, by id
//   k_pl_gather         the column array, one thread per word
//   (the index over the columns: alga_seed_index, seed_index.hip)
//   k_pl_place          one wave per read, both strands: seed_and_verify (seed_device.h) once per strand over the read's L / k seeds.  A seed at
//                       column g stands for the placement at g - j k where that lies in g's target with all L bases; the whole read is
//                       verified.  The minimum key and the number of placements at its mm are reduced across the wave.
//   k_pl_depth_add      +1 / -1 of every counting read into the difference array, the per-target sums: 32- and 64-bit integer atomics
//   k_pl_uncovered      columns with cover 0 per target (the cover is one scan of the difference array over all columns: a read's +1 and -1
//                       lie in one target, or the -1 on the first column of the next)
//   k_pl_pairs          the verdict on every pair, the insert histogram (integer atomics on the global histogram: up to 2^20 + 1 bins)
//   k_pl_fasta_sizes / k_pl_fasta_write   the records of the final FASTA with `_reads=<n>_depth=<q>.<dd>` in the header, one wave per record
// Four waves per block; k_pl_place runs 8 blocks per CU (the lookups are dependent random reads: occupancy is what hides them).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "place_kernels.h"
#include "seed_device.h"
#include "text_record.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int PL_BLOCK = 256, PL_WAVES = PL_BLOCK / 64;
constexpr uint8_t PL_ST_PLACED = 1, PL_ST_UNIQUE = 2, PL_ST_MINUS = 4;   // ALGA_PLACE_* of include/alga_amd.h (the bits of d_state)
constexpr uint8_t PL_V_ACCEPTED = 2;                                   // ALGA_FINAL_ACCEPTED

__global__ void __launch_bounds__(PL_BLOCK) k_pl_node_check(const uint8_t *__restrict__ pair_off, const int32_t *__restrict__ len, uint64_t n,
                                                            unsigned long long *__restrict__ counters) {
    unsigned long long mx = 0;
    bool bad = false;
    for (uint64_t v = (uint64_t) blockIdx.x * PL_BLOCK + threadIdx.x; v < n; v += (uint64_t) gridDim.x * PL_BLOCK) {
        const int32_t l = len[v];
        if (l > 0 && (unsigned long long) l > mx) mx = (unsigned long long) l;
        if (pair_off) {
            const uint8_t po = pair_off[v];
            if (po > 2 || po != pair_off[v ^ 1]) bad = true;
            else if (po == 1 && (v + 2 >= n || pair_off[v + 2] != 2)) bad = true;
            else if (po == 2 && (v < 2 || pair_off[v - 2] != 1)) bad = true;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = (unsigned long long) (uint32_t) __shfl_xor((int) (uint32_t) mx, o); mx = w > mx ? w : mx; }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&counters[PL_MAX_READ_LEN], mx);
    if (bad) counters[PL_BAD_PAIR] = 1ull;
}

__global__ void __launch_bounds__(PL_BLOCK) k_pl_target_check(const int32_t *__restrict__ tlen, uint64_t T, int32_t k, unsigned long long *__restrict__ counters) {
    unsigned long long sum = 0, idx = 0;
    bool bad = false;
    for (uint64_t t = (uint64_t) blockIdx.x * PL_BLOCK + threadIdx.x; t < T; t += (uint64_t) gridDim.x * PL_BLOCK) {
        const int32_t l = tlen[t];
        if (l < 0) { bad = true; continue; }
        sum += (unsigned long long) l;
        if (l >= k) idx += (unsigned long long) (l - k + 1);
    }
    sum = wave_sum(sum); idx = wave_sum(idx);
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&counters[PL_COLUMNS], sum);
        if (idx) atomicAdd(&counters[PL_INDEX_POS], idx);
    }
    if (bad) counters[PL_BAD_LEN] = 1ull;
}

__global__ void __launch_bounds__(PL_BLOCK) k_pl_final_targets(const unsigned long long *__restrict__ word_off, const uint8_t *__restrict__ verdict,
                                                               const int32_t *__restrict__ order, const int32_t *__restrict__ begin, const int32_t *__restrict__ len,
                                                               uint64_t n, unsigned long long *__restrict__ tbegin, int32_t *__restrict__ tlen) {
    const uint64_t j = (uint64_t) blockIdx.x * PL_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = (uint32_t) order[j];
    const bool live = verdict[k] == PL_V_ACCEPTED;
    tbegin[j] = 16ull * word_off[k] + (unsigned long long) (live ? begin[k] : 0);
    tlen[j] = live ? len[k] : 0;
}

__global__ void __launch_bounds__(PL_BLOCK) k_pl_gather(const uint32_t *__restrict__ words, const unsigned long long *__restrict__ begin, PlTargets t,
                                                        uint32_t *__restrict__ cols) {
    packed_words_body<PL_BLOCK>(t.off, t.n, t.columns, (t.columns + 15) >> 4, cols, [&](uint32_t tt, uint32_t q) { return base_at(words, begin[tt] + q); });
}

// Geometry of a read of L bases on the targets: (seed js, column g) is the placement at g - js k where it lies in g's target
struct PlGeometry {
    static constexpr int kMmShift = 33;              // the key: (mm << 33) | (first column << 1) | strand
    const PlTargets &t;
    int k, L, strand;
    __device__ __forceinline__ bool operator()(int js, uint32_t g, uint32_t &gp, int &n, unsigned long long &low) const {
        const uint32_t tt = item_of(t.off, t.n, g);
        const long long p = (long long) g - (long long) t.off[tt] - (long long) js * k;
        if (p < 0 || p + (long long) L > (long long) t.len[tt]) return false;
        gp = g - (uint32_t) (js * k); n = L;
        low = ((unsigned long long) gp << 1) | (unsigned long long) strand;
        return true;
    }
};

__global__ void __launch_bounds__(PL_BLOCK) k_pl_place(SeedReads rd, PlTargets t, SeedIndex x, int32_t k, uint32_t max_mm, uint32_t max_occ, PlOut o,
                                                       unsigned long long *__restrict__ scratch, uint32_t scratch_words, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t) blockIdx.x * PL_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * PL_WAVES;
    unsigned long long *ub = scratch + wave * (uint64_t) scratch_words;
    unsigned long long n_placed = 0, n_unique = 0, n_sat = 0, n_seeds = 0, n_over = 0;       // wave-uniform
    for (uint64_t r = wave; r < rd.R; r += n_waves) {
        const int32_t L = rd.len[2 * r + 1];
        unsigned long long best = ~0ull;                 // of this lane's placements
        MinMmTally tally;
        if (L >= k) {
            for (int strand = 0; strand < 2; strand++) {
                const RowQuery q{rd.rows + (2 * r + (strand == 0 ? 1u : 0u)) * (size_t) rd.stride, blocks_of(L), k};
                seed_and_verify(x, t.cols, k, max_mm, max_occ, L / k, q, PlGeometry{t, k, L, strand}, ub, best, tally, n_seeds, n_over);
            }
        }
        const unsigned long long win = wave_min_u64(best);
        int32_t tg = -1, ps = -1;
        uint8_t mm8 = 0, hits8 = 0, st8 = 0;
        if (win != ~0ull) {
            const uint32_t bmm = (uint32_t) (win >> 33), gp = (uint32_t) (win >> 1);
            const unsigned long long hits = wave_sum(tally.mm == bmm ? (unsigned long long) tally.cnt : 0ull);
            const uint32_t tt = item_of(t.off, t.n, gp);
            tg = (int32_t) tt; ps = (int32_t) (gp - t.off[tt]); mm8 = (uint8_t) bmm; hits8 = (uint8_t) (hits > 255ull ? 255ull : hits);
            st8 = (uint8_t) (PL_ST_PLACED | (hits == 1ull ? PL_ST_UNIQUE : 0) | ((win & 1ull) ? PL_ST_MINUS : 0));
            n_placed++; n_unique += hits == 1ull; n_sat += hits > 255ull;
        }
        if (lane == 0) { o.target[r] = tg; o.pos[r] = ps; o.mm[r] = mm8; o.hits[r] = hits8; o.state[r] = st8; }
    }
    if (lane == 0) {
        if (n_placed) atomicAdd(&counters[PL_PLACED], n_placed);
        if (n_unique) atomicAdd(&counters[PL_UNIQUE], n_unique);
        if (n_sat) atomicAdd(&counters[PL_SATURATED], n_sat);
        if (n_seeds) atomicAdd(&counters[PL_SEEDS], n_seeds);
        if (n_over) atomicAdd(&counters[PL_SEEDS_OVER], n_over);
    }
}

__global__ void __launch_bounds__(PL_BLOCK) k_pl_depth_add(SeedReads rd, PlTargets t, PlOut o, int multi, uint32_t *__restrict__ diff, unsigned long long *__restrict__ tstat) {
    for (uint64_t r = (uint64_t) blockIdx.x * PL_BLOCK + threadIdx.x; r < rd.R; r += (uint64_t) gridDim.x * PL_BLOCK) {
        const uint8_t st = o.state[r];
        if (!(st & (multi ? PL_ST_PLACED : PL_ST_UNIQUE))) continue;
        const uint32_t tt = (uint32_t) o.target[r], L = (uint32_t) rd.len[2 * r + 1];
        const uint32_t gp = t.off[tt] + (uint32_t) o.pos[r];
        atomicAdd(&diff[gp], 1u);
        atomicAdd(&diff[gp + L], 0xFFFFFFFFu);                                // gp + L <= col_off[tt + 1] <= columns: the array has columns + 1 entries
        atomicAdd(&tstat[tt], 1ull);
        atomicAdd(&tstat[(size_t) t.n + tt], (unsigned long long) L);
        atomicAdd(&tstat[2 * (size_t) t.n + tt], (unsigned long long) o.mm[r]);
    }
}

__global__ void __launch_bounds__(PL_BLOCK) k_pl_uncovered(PlTargets t, const uint32_t *__restrict__ cover, unsigned long long *__restrict__ tstat) {
    const int lane = threadIdx.x & 63;
    unsigned long long *unc = tstat + 3 * (size_t) t.n;
    for (uint64_t g0 = ((uint64_t) blockIdx.x * PL_BLOCK + (threadIdx.x & ~63u)); g0 < t.columns; g0 += (uint64_t) gridDim.x * PL_BLOCK) {
        const uint64_t g = g0 + (uint64_t) lane;
        const bool zero = g < t.columns && cover[g] == 0u;
        const unsigned long long m = __ballot(zero);
        if (!m) continue;
        const uint64_t glast = g0 + 63 < t.columns ? g0 + 63 : t.columns - 1;
        const uint32_t t0 = item_of(t.off, t.n, (uint32_t) g0);
        if ((uint64_t) t.off[t0 + 1] > glast) {                           // the wave's columns lie in one target
            if (lane == 0) atomicAdd(&unc[t0], (unsigned long long) __popcll(m));
        } else if (zero) atomicAdd(&unc[item_of(t.off, t.n, (uint32_t) g)], 1ull);
    }
}

__global__ void __launch_bounds__(PL_BLOCK) k_pl_pairs(SeedReads rd, const uint8_t *__restrict__ pair_off, PlOut o, int32_t max_insert, unsigned long long *__restrict__ hist,
                                                       unsigned long long *__restrict__ counters) {
    unsigned long long n_pairs = 0, n_proper = 0, n_improper = 0, n_split = 0, n_nu = 0, sum = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * PL_BLOCK + threadIdx.x; r < rd.R; r += (uint64_t) gridDim.x * PL_BLOCK) {
        if (pair_off[2 * r + 1] != 1) continue;                                // the mate with the smaller index judges: its mate is read r + 1
        const uint64_t r2 = r + 1;
        const uint8_t s1 = o.state[r], s2 = o.state[r2];
        n_pairs++;
        if (!(s1 & PL_ST_UNIQUE) || !(s2 & PL_ST_UNIQUE)) { n_nu++; continue; }
        if (o.target[r] != o.target[r2]) { n_split++; continue; }
        if ((s1 & PL_ST_MINUS) == (s2 & PL_ST_MINUS)) { n_improper++; continue; }
        const uint64_t rp = (s1 & PL_ST_MINUS) ? r2 : r, rm = (s1 & PL_ST_MINUS) ? r : r2;
        const long long a = o.pos[rp], la = rd.len[2 * rp + 1], b = o.pos[rm], lb = rd.len[2 * rm + 1];
        const long long ins = b + lb - a;
        if (a <= b && a + la <= b + lb && ins <= (long long) max_insert) { n_proper++; sum += (unsigned long long) ins; atomicAdd(&hist[ins], 1ull); }
        else n_improper++;
    }
    n_pairs = wave_sum(n_pairs); n_proper = wave_sum(n_proper); n_improper = wave_sum(n_improper); n_split = wave_sum(n_split);
    n_nu = wave_sum(n_nu); sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && n_pairs) {
        atomicAdd(&counters[PL_PAIRS], n_pairs);
        if (n_proper) { atomicAdd(&counters[PL_PROPER], n_proper); atomicAdd(&counters[PL_INSERT_SUM], sum); }
        if (n_improper) atomicAdd(&counters[PL_IMPROPER], n_improper);
        if (n_split) atomicAdd(&counters[PL_SPLIT], n_split);
        if (n_nu) atomicAdd(&counters[PL_NOT_UNIQUE], n_nu);
    }
}

// ---- FASTA with depth headers ---------------------------------------------------------------------------------------------------------
// `>contig_id=<id>_length=<L>_reads=<n>_depth=<q>.<dd>\n<window>\n`
struct PlRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const PlFasta &f, uint64_t j) {
        const uint32_t k = (uint32_t) f.order[j];
        if (f.verdict[k] != PL_V_ACCEPTED) return false;
        contig_head(j, (uint32_t) f.len[k]); depth(f.t_reads[j], f.t_bases[j]); seal();
        seq.row = f.words + f.word_off[k]; seq.q0 = (uint32_t) f.begin[k];
        return true;
    }
};

__global__ void __launch_bounds__(PL_BLOCK) k_pl_fasta_sizes(PlFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<PlRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(PL_BLOCK) k_pl_fasta_write(PlFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<PlRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_pl_node_check(const uint8_t *pair_off, const int32_t *len, uint64_t n, unsigned long long *counters, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_pl_node_check, dim3(stage_grid(n, PL_BLOCK, 4096)), dim3(PL_BLOCK), 0, s, pair_off, len, n, counters);
}

void launch_pl_target_check(const int32_t *tlen, uint64_t T, int32_t k, unsigned long long *counters, hipStream_t s) {
    if (T) hipLaunchKernelGGL(k_pl_target_check, dim3(stage_grid(T, PL_BLOCK, 4096)), dim3(PL_BLOCK), 0, s, tlen, T, k, counters);
}

void launch_pl_final_targets(const unsigned long long *word_off, const uint8_t *verdict, const int32_t *order, const int32_t *begin, const int32_t *len, uint64_t n,
                             unsigned long long *tbegin, int32_t *tlen, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_pl_final_targets, dim3((unsigned) ((n + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, s, word_off, verdict, order, begin, len, n, tbegin, tlen);
}

void launch_pl_gather(const uint32_t *words, const unsigned long long *begin, const PlTargets &t, uint32_t *cols, hipStream_t s) {
    if (t.columns) hipLaunchKernelGGL(k_pl_gather, dim3(stage_grid((t.columns + 15) >> 4, PL_BLOCK, 1u << 16)), dim3(PL_BLOCK), 0, s, words, begin, t, cols);
}

void launch_pl_place(const SeedReads &r, const PlTargets &t, const SeedIndex &x, int32_t k, int32_t max_mm, int32_t max_occ, const PlOut &o, unsigned long long *scratch,
                     uint32_t scratch_words_per_wave, int blocks, unsigned long long *counters, hipStream_t s) {
    if (r.R) hipLaunchKernelGGL(k_pl_place, dim3((unsigned) blocks), dim3(PL_BLOCK), 0, s, r, t, x, k, (uint32_t) max_mm, (uint32_t) max_occ, o, scratch, scratch_words_per_wave,
                                counters);
}

void launch_pl_depth_add(const SeedReads &r, const PlTargets &t, const PlOut &o, int multi, uint32_t *diff, unsigned long long *tstat, hipStream_t s) {
    if (r.R && t.n) hipLaunchKernelGGL(k_pl_depth_add, dim3(stage_grid(r.R, PL_BLOCK, 8192)), dim3(PL_BLOCK), 0, s, r, t, o, multi, diff, tstat);
}

void launch_pl_uncovered(const PlTargets &t, const uint32_t *cover, unsigned long long *tstat, hipStream_t s) {
    if (t.columns) hipLaunchKernelGGL(k_pl_uncovered, dim3(stage_grid(t.columns, PL_BLOCK, 8192)), dim3(PL_BLOCK), 0, s, t, cover, tstat);
}

void launch_pl_pairs(const SeedReads &r, const uint8_t *pair_off, const PlOut &o, int32_t max_insert, unsigned long long *hist, unsigned long long *counters, hipStream_t s) {
    if (r.R && pair_off) hipLaunchKernelGGL(k_pl_pairs, dim3(stage_grid(r.R, PL_BLOCK, 8192)), dim3(PL_BLOCK), 0, s, r, pair_off, o, max_insert, hist, counters);
}

void launch_pl_fasta_sizes(const PlFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_pl_fasta_sizes, dim3(text_sizes_blocks(f.n, PL_BLOCK)), dim3(PL_BLOCK), 0, s, f, sizes, counters);
}

void launch_pl_fasta_write(const PlFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_pl_fasta_write, dim3(text_write_blocks(i0, i1, PL_WAVES)), dim3(PL_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
