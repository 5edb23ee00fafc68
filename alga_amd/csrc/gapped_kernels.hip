// alga_amd/csrc/gapped_kernels.hip -- the reads the Hamming placement left unplaced laid onto the same targets by edit distance: where they lie,
// how (CIGAR), their cover (include/alga_amd.h: alga_place_gapped_device; the definition is the comment there, host side in engine_gapped.hip).
//
// The targets are the placement's column space (place_kernels.hip) and the index is the shared seed index (seed_index.hip); the candidate loop
// is this file's own: a candidate is a (seed, indexed column) pair, not a first column, so seed_and_verify does not fit.
//   k_gp_target_check   the targets are the placement's (lengths against its col_off); the indexed positions
//   k_gp_flag           who takes part, the reads above the cap counted; k_gp_scatter: the dense list of them (flag, scan, scatter)
//   k_gp_score          one wave per participating read, both strands.  Seeds to lanes 64 at a time (look-up, usable mask, scan of the
//                       occurrences); the candidates then go to the two HALVES of the wave, one each: the diagonal rule is checked by the
//                       half's 32 lanes in parallel (lane h takes the earlier seeds h, h + 32, ..), the distance is the banded table with one
//                       lane per diagonal (2 E + 1 <= 31): the lane streams its own target bases, the up-neighbour comes from lane h + 1, the
//                       in-row dependency is a min-plus prefix over the half.  A half leaves its candidate when no cell of a row is <= E.
//                       Right part first, the left part only where the right one is within E.  Every lane 0 of a half keeps the minimum key
//                       and the maximum (strand, column) at its own smallest d; two wave reductions give best and UNIQUE.
//   k_gp_trace          one wave per placed read: half 0 the right part, half 1 the left part of the best candidate, again as banded tables,
//                       now with the first attaining direction of every cell (two ballots a row) in LDS; lanes 0 and 32 walk back, lane 0
//                       joins left, seed and right into runs.  k_gp_cigar compacts the strided runs behind the scan of their numbers.
//   k_gp_depth_add / k_gp_cover   difference array of the UNIQUE gapped reads, per-target sums by integer atomics; cover = the placement's + scan
//   k_gp_tsv_sizes / k_gp_tsv_write   the TSV lines through text_record.h
// Block sizes and blocks per CU are picked, not tuned: four waves a block and eight blocks per CU where the look-ups dominate (as k_pl_place),
// two waves a block in k_gp_trace (16 KB of directions per wave).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gapped_kernels.h"
#include "seed_device.h"
#include "text_record.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int GP_BLOCK = 256, GP_WAVES = GP_BLOCK / 64;
constexpr int GP_TR_BLOCK = 128, GP_TR_WAVES = GP_TR_BLOCK / 64;
constexpr int GP_INF = 1 << 20;
constexpr uint8_t GP_ST_PLACED = 1, GP_ST_UNIQUE = 2, GP_ST_MINUS = 4, GP_ST_INDEL = 8;   // ALGA_GAPPED_* of include/alga_amd.h (the bits of d_state)
constexpr uint32_t GP_OP_M = 0, GP_OP_I = 1, GP_OP_D = 2;                                 // ALGA_CIGAR_*
// the key of a candidate: d << 56 | strand << 55 | first column << 23 | (e - p) << 12 | seed << 5 | (left end - left bases + E)
constexpr int GP_K_D = 56, GP_K_STRAND = 55, GP_K_COL = 23, GP_K_SPAN = 12, GP_K_SEED = 5;

__global__ void __launch_bounds__(GP_BLOCK) k_gp_target_check(const int32_t *__restrict__ tlen, const uint32_t *__restrict__ col_off, uint64_t T, uint64_t columns,
                                                              int32_t k, unsigned long long *__restrict__ counters) {
    unsigned long long idx = 0;
    bool bad = false;
    if (blockIdx.x == 0 && threadIdx.x == 0 && (uint64_t) col_off[T] != columns) bad = true;
    for (uint64_t t = (uint64_t) blockIdx.x * GP_BLOCK + threadIdx.x; t < T; t += (uint64_t) gridDim.x * GP_BLOCK) {
        const int32_t l = tlen[t];
        if (l < 0 || col_off[t + 1] - col_off[t] != (uint32_t) l) { bad = true; continue; }
        if (l >= k) idx += (unsigned long long) (l - k + 1);
    }
    idx = wave_sum(idx);
    if ((threadIdx.x & 63) == 0 && idx) atomicAdd(&counters[GP_INDEX_POS], idx);
    if (bad) counters[GP_BAD_TARGETS] = 1ull;
}

__global__ void __launch_bounds__(GP_BLOCK) k_gp_flag(SeedReads rd, const uint8_t *__restrict__ pl_state, int32_t k, uint32_t *__restrict__ flag,
                                                      unsigned long long *__restrict__ counters) {
    unsigned long long tried = 0, longer = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * GP_BLOCK + threadIdx.x; r <= rd.R; r += (uint64_t) gridDim.x * GP_BLOCK) {
        uint32_t f = 0;
        if (r < rd.R && !(pl_state[r] & GP_ST_PLACED)) {
            const int32_t L = rd.len[2 * r + 1];
            if (L > GP_MAX_READ) longer++;
            else if (L >= k) { f = 1; tried++; }
        }
        flag[r] = f;
    }
    tried = wave_sum(tried); longer = wave_sum(longer);
    if ((threadIdx.x & 63) == 0) {
        if (tried) atomicAdd(&counters[GP_TRIED], tried);
        if (longer) atomicAdd(&counters[GP_SKIPPED_LONG], longer);
    }
}

__global__ void __launch_bounds__(GP_BLOCK) k_gp_scatter(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint64_t R, uint32_t *__restrict__ list) {
    for (uint64_t r = (uint64_t) blockIdx.x * GP_BLOCK + threadIdx.x; r < R; r += (uint64_t) gridDim.x * GP_BLOCK)
        if (flag[r]) list[pos[r]] = (uint32_t) r;
}

// One part of a candidate's alignment, seen from the seed: row i = 1 .. n is read base rd0 + rstep (i - 1), cell c = 1 .. avail of a row is column
// c0 + cstep (c - 1); on: the half has such a part to do
struct GpPart {
    int n, avail;
    int rd0, rstep;
    uint32_t c0;
    int cstep;
    bool on;
};

// The banded table of one part per HALF of the wave (the fields of pt are uniform in a half): lane h of the half is diagonal h - E, its cell of
// row i is c = i + h - E.  Row 0 is D[0][c] = c; a cell outside 0 <= c <= avail or off the band is GP_INF.  val / c_end: the end cell of row n
// by (value, |c - n|, c), val > E where the half left its candidate or had none; the same in all lanes of the half.  kTrace: the first
// attaining direction (0 diagonal, 1 up, 2 left) of every cell as two ballots a row, dirs[2 (i - 1)] and [.. + 1] (this wave's LDS).
// Every lane of the wave runs this with the same n_max >= the n of both halves: the shuffles are in uniform control flow.
template <bool kTrace>
__device__ __forceinline__ void band_part(const uint32_t *__restrict__ row, const uint32_t *__restrict__ cols, int E, const GpPart &pt, int n_max, int &val, int &c_end,
                                          unsigned long long *dirs) {
    const int lane = threadIdx.x & 63, h = lane & 31, dd = h - E;
    const bool diag_on = h <= 2 * E;
    int prev = (pt.on && diag_on && dd >= 0 && dd <= pt.avail) ? dd : GP_INF;
    bool alive = pt.on, dead = false;
    uint32_t rw = 0, cw = 0;
    int rwi = -1;
    long long cwi = -1;
    for (int i = 1; i <= n_max; i++) {
        const bool rowon = alive && i <= pt.n;
        if (__ballot(rowon) == 0ull) break;
        int up = __shfl_down(prev, 1, 32);
        if (h == 31) up = GP_INF;
        const int c = i + dd;
        const bool valid = rowon && diag_on && c >= 0 && c <= pt.avail;
        int sub = 1;
        if (valid && c >= 1) {
            const int ri = pt.rd0 + pt.rstep * (i - 1);
            if ((ri >> 4) != rwi) { rwi = ri >> 4; rw = row[rwi]; }
            const long long ci = (long long) pt.c0 + (long long) pt.cstep * (c - 1);
            if ((ci >> 4) != cwi) { cwi = ci >> 4; cw = cols[cwi]; }
            sub = ((rw >> ((ri & 15) << 1)) & 3u) != ((cw >> ((ci & 15) << 1)) & 3u) ? 1 : 0;
        }
        int a = GP_INF;
        if (valid) {
            a = up + 1;
            if (c >= 1 && prev + sub < a) a = prev + sub;
        }
        int b = a - h;                           // new[h] = h + min over h' <= h of (a[h'] - h')
        for (int o = 1; o < 32; o <<= 1) {
            const int t = __shfl_up(b, o, 32);
            if (h >= o && t < b) b = t;
        }
        int nw = b + h;
        if (!valid || nw > GP_INF) nw = GP_INF;
        if constexpr (kTrace) {
            const int dirv = (c >= 1 && prev + sub == nw) ? 0 : (up + 1 == nw ? 1 : 2);
            const unsigned long long b0 = __ballot(valid && (dirv & 1)), b1 = __ballot(valid && (dirv & 2));
            if (lane == 0) { dirs[2 * (i - 1)] = b0; dirs[2 * (i - 1) + 1] = b1; }
        }
        const unsigned long long within = __ballot(nw <= E);
        if (rowon) {
            prev = nw;
            if (((within >> (lane & 32)) & 0xFFFFFFFFull) == 0ull) { alive = false; dead = true; }
        }
    }
    uint32_t key = ((uint32_t) (prev < 63 ? prev : 63) << 12) | ((uint32_t) (dd < 0 ? -dd : dd) << 6) | (uint32_t) h;
    if (!pt.on || dead) key = 63u << 12;
    for (int o = 16; o > 0; o >>= 1) { const uint32_t w = (uint32_t) __shfl_xor((int) key, o, 32); key = w < key ? w : key; }
    val = (int) (key >> 12);
    c_end = pt.n + (int) (key & 63u) - E;
}

__global__ void __launch_bounds__(GP_BLOCK) k_gp_score(SeedReads rd, SeedSpace t, SeedIndex x, int32_t k, int32_t E, uint32_t max_occ, const uint32_t *__restrict__ list,
                                                       uint64_t n_list, GpOut o, unsigned long long *__restrict__ best_out, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63, h = lane & 31, half = lane >> 5;
    const uint64_t wave = (uint64_t) blockIdx.x * GP_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * GP_WAVES;
    unsigned long long n_placed = 0, n_unique = 0, n_seeds = 0, n_over = 0, n_cand = 0, n_edits = 0;       // wave-uniform
    for (uint64_t i = wave; i < n_list; i += n_waves) {
        const uint32_t r = list[i];
        const int32_t L = rd.len[2 * (uint64_t) r + 1];
        const int nwords = blocks_of(L), S = L / k;
        unsigned long long kmin = ~0ull, kmax = 0ull;                // of this lane's candidates
        for (int strand = 0; strand < 2; strand++) {
            const uint32_t *row = rd.rows + (2 * (uint64_t) r + (strand == 0 ? 1u : 0u)) * (size_t) rd.stride;
            unsigned long long um0 = 0ull, um1 = 0ull;               // the usable seeds 0 .. 63 and 64 .. 127 (S <= GP_MAX_READ / 8)
            for (int c0 = 0; c0 < S; c0 += 64) {
                const int j = c0 + lane;
                const bool act = j < S;
                uint32_t lb = 0, occ = 0;
                if (act) seed_lookup(x, row_kmer(row, nwords, j * k, k), max_occ, lb, occ);
                const bool usable = act && occ >= 1u && occ <= max_occ;
                const unsigned long long umask = __ballot(usable);
                if (c0 == 0) um0 = umask; else um1 = umask;
                n_seeds += (unsigned long long) __popcll(__ballot(act));
                n_over += (unsigned long long) __popcll(__ballot(act && occ > max_occ));
                const uint32_t mine = usable ? occ : 0u;
                uint32_t inc = mine;
                for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t) __shfl_up((int) inc, d); if (lane >= d) inc += up; }
                const uint32_t C = (uint32_t) __shfl((int) inc, 63), exc = inc - mine;
                for (uint32_t p0 = 0; p0 < C; p0 += 2) {
                    const bool cact = p0 + (uint32_t) half < C;
                    const uint32_t ci = cact ? p0 + (uint32_t) half : C - 1u;
                    int sl = 0;                  // the seed lane of candidate ci: the first with inc > ci
                    for (int st = 32; st > 0; st >>= 1) if ((uint32_t) __shfl((int) inc, sl + st - 1) <= ci) sl += st;
                    const uint32_t s_lb = (uint32_t) __shfl((int) lb, sl), s_exc = (uint32_t) __shfl((int) exc, sl);
                    const int js = c0 + sl;
                    const uint32_t g = x.vals[s_lb + (ci - s_exc)];
                    const uint32_t tt = item_of(t.off, t.n, g);
                    const int q = (int) (g - t.off[tt]), tl = t.len[tt];
                    // the diagonal rule: an earlier usable seed matches on this diagonal, in this target
                    bool dup = false;
                    for (int j2 = h; j2 < js && !dup; j2 += 32) {
                        const unsigned long long m = j2 < 64 ? um0 : um1;
                        if (!((m >> (j2 & 63)) & 1ull)) continue;
                        const int back = (js - j2) * k;
                        if (back <= q) dup = row_kmer(row, nwords, j2 * k, k) == col_kmer(t.cols, g - (uint32_t) back, k);
                    }
                    const unsigned long long dupm = __ballot(dup);
                    const bool counts = cact && ((dupm >> (lane & 32)) & 0xFFFFFFFFull) == 0ull;
                    n_cand += (unsigned long long) __popcll(__ballot(counts && h == 0));
                    const int n_r = L - js * k - k, n_l = js * k;
                    const int nr0 = __shfl(counts ? n_r : 0, 0), nr1 = __shfl(counts ? n_r : 0, 32);
                    int vr, cr, vl, cl;
                    band_part<false>(row, t.cols, E, GpPart{n_r, tl - q - k, js * k + k, 1, g + (uint32_t) k, 1, counts}, nr0 > nr1 ? nr0 : nr1, vr, cr, nullptr);
                    const bool okr = counts && vr <= E;
                    const int nl0 = __shfl(okr ? n_l : 0, 0), nl1 = __shfl(okr ? n_l : 0, 32);
                    band_part<false>(row, t.cols, E, GpPart{n_l, q, js * k - 1, -1, g - 1u, -1, okr}, nl0 > nl1 ? nl0 : nl1, vl, cl, nullptr);
                    if (okr && vr + vl <= E && h == 0) {
                        const unsigned long long d = (unsigned long long) (vr + vl), gp = (unsigned long long) (g - (uint32_t) cl);
                        const unsigned long long sg = ((unsigned long long) strand << 32) | gp;
                        const unsigned long long key = (d << GP_K_D) | (sg << GP_K_COL) | ((unsigned long long) (cl + k + cr) << GP_K_SPAN) |
                                                       ((unsigned long long) js << GP_K_SEED) | (unsigned long long) (cl - n_l + E);
                        if (kmin == ~0ull || d < (kmin >> GP_K_D)) { kmin = key; kmax = sg; }
                        else if (d == (kmin >> GP_K_D)) { kmin = key < kmin ? key : kmin; kmax = sg > kmax ? sg : kmax; }
                    }
                }
            }
        }
        const unsigned long long win = wave_min_u64(kmin);
        int32_t tg = -1, ps = -1, en = -1;
        uint8_t ed8 = 0, st8 = 0;
        if (win != ~0ull) {
            const unsigned long long bd = win >> GP_K_D;
            const unsigned long long far = wave_max((kmin != ~0ull && (kmin >> GP_K_D) == bd) ? kmax : 0ull);
            const uint32_t strand = (uint32_t) (win >> GP_K_STRAND) & 1u, gp = (uint32_t) (win >> GP_K_COL), span = (uint32_t) (win >> GP_K_SPAN) & 0x7FFu;
            const uint32_t tt = item_of(t.off, t.n, gp), fgp = (uint32_t) far;
            const bool unique = (uint32_t) (far >> 32) == strand && (unsigned long long) fgp <= (unsigned long long) gp + (unsigned long long) E && item_of(t.off, t.n, fgp) == tt;
            tg = (int32_t) tt; ps = (int32_t) (gp - t.off[tt]); en = ps + (int32_t) span; ed8 = (uint8_t) bd;
            st8 = (uint8_t) (GP_ST_PLACED | (unique ? GP_ST_UNIQUE : 0) | (strand ? GP_ST_MINUS : 0));
            n_placed++; n_unique += unique; n_edits += bd;
        }
        if (lane == 0) { o.target[r] = tg; o.pos[r] = ps; o.end[r] = en; o.edits[r] = ed8; o.state[r] = st8; best_out[i] = win; }
    }
    if (lane == 0) {
        if (n_placed) atomicAdd(&counters[GP_PLACED], n_placed);
        if (n_unique) atomicAdd(&counters[GP_UNIQUE], n_unique);
        if (n_edits) atomicAdd(&counters[GP_EDITS], n_edits);
        if (n_cand) atomicAdd(&counters[GP_CANDIDATES], n_cand);
        if (n_seeds) atomicAdd(&counters[GP_SEEDS], n_seeds);
        if (n_over) atomicAdd(&counters[GP_SEEDS_OVER], n_over);
    }
}

__global__ void __launch_bounds__(GP_TR_BLOCK) k_gp_trace(SeedReads rd, SeedSpace t, int32_t k, int32_t E, const uint32_t *__restrict__ list, uint64_t n_list,
                                                          const unsigned long long *__restrict__ best, uint8_t *__restrict__ state, uint32_t *__restrict__ runs,
                                                          uint32_t *__restrict__ n_runs, unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_dirs[GP_TR_WAVES][2 * GP_MAX_READ];
    __shared__ uint32_t s_runs[GP_TR_WAVES][2][32];                  // the runs of the right and of the left part, in the order they are walked
    __shared__ uint32_t s_cnt[GP_TR_WAVES][2];
    const int lane = threadIdx.x & 63, half = lane >> 5, wib = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t) blockIdx.x * GP_TR_WAVES + wib, n_waves = (uint64_t) gridDim.x * GP_TR_WAVES;
    unsigned long long *dirs = s_dirs[wib];
    unsigned long long n_indel = 0, n_ins = 0, n_del = 0;            // lane 0
    for (uint64_t i = wave; i < n_list; i += n_waves) {
        const unsigned long long win = best[i];
        if (win == ~0ull) continue;
        const uint32_t r = list[i];
        const int32_t L = rd.len[2 * (uint64_t) r + 1];
        const uint32_t strand = (uint32_t) (win >> GP_K_STRAND) & 1u, gp = (uint32_t) (win >> GP_K_COL);
        const int js = (int) ((win >> GP_K_SEED) & 0x7Full), dl = (int) (win & 0x1Full);
        const uint32_t *row = rd.rows + (2 * (uint64_t) r + (strand == 0 ? 1u : 0u)) * (size_t) rd.stride;
        const int n_r = L - js * k - k, n_l = js * k, cl0 = n_l + dl - E;
        const uint32_t g = gp + (uint32_t) cl0, tt = item_of(t.off, t.n, g);
        const int q = (int) (g - t.off[tt]), tl = t.len[tt];
        const GpPart pt = half == 0 ? GpPart{n_r, tl - q - k, js * k + k, 1, g + (uint32_t) k, 1, true} : GpPart{n_l, q, js * k - 1, -1, g - 1u, -1, true};
        int val, c_end;
        band_part<true>(row, t.cols, E, pt, n_r > n_l ? n_r : n_l, val, c_end, dirs);
        __threadfence_block();
        if ((lane & 31) == 0) {                                      // lanes 0 and 32 walk their part back from its end cell to (0, 0)
            const int hb = lane & 32;
            int ii = pt.n, c = val <= E ? c_end : 0, guard = 2 * GP_MAX_READ + 64;
            uint32_t cur = 3u, len = 0u, cnt = 0u;
            if (val > E) ii = 0;                                     // (cannot be: the candidate was scored within E)
            while ((ii > 0 || c > 0) && guard-- > 0) {
                uint32_t op = GP_OP_D;
                if (ii > 0) {
                    int hh = c - ii + E;
                    hh = hh < 0 ? 0 : (hh > 31 ? 31 : hh);
                    op = (uint32_t) ((dirs[2 * (ii - 1)] >> (hb + hh)) & 1ull) | ((uint32_t) ((dirs[2 * (ii - 1) + 1] >> (hb + hh)) & 1ull) << 1);
                }
                if (op == GP_OP_M) { ii--; c--; }
                else if (op == GP_OP_I) ii--;
                else c--;
                if (c < 0) break;
                if (op == cur) len++;
                else {
                    if (len && cnt < 32u) s_runs[wib][half][cnt++] = (len << 2) | cur;
                    cur = op; len = 1u;
                }
            }
            if (len && cnt < 32u) s_runs[wib][half][cnt++] = (len << 2) | cur;
            s_cnt[wib][half] = cnt;
        }
        __threadfence_block();
        if (lane == 0) {                                             // the left part as walked, the seed, the right part backwards
            uint32_t *out = runs + i * (uint64_t) GP_MAX_RUNS;
            uint32_t n_out = 0, cur = 3u, len = 0u, ins = 0, del = 0;
            const uint32_t nl = s_cnt[wib][1], nr = s_cnt[wib][0];
            for (uint32_t u = 0; u < nl + 1u + nr; u++) {
                const uint32_t w = u < nl ? s_runs[wib][1][u] : (u == nl ? ((uint32_t) k << 2) | GP_OP_M : s_runs[wib][0][nr - 1u - (u - nl - 1u)]);
                const uint32_t op = w & 3u, ln = w >> 2;
                ins += op == GP_OP_I ? ln : 0u; del += op == GP_OP_D ? ln : 0u;
                if (op == cur) len += ln;
                else {
                    if (len && n_out < (uint32_t) GP_MAX_RUNS) out[n_out++] = (len << 2) | cur;
                    cur = op; len = ln;
                }
            }
            if (len && n_out < (uint32_t) GP_MAX_RUNS) out[n_out++] = (len << 2) | cur;
            n_runs[r] = n_out;
            if (ins | del) { state[r] = (uint8_t) (state[r] | GP_ST_INDEL); n_indel++; }
            n_ins += ins; n_del += del;
        }
        __threadfence_block();
    }
    if (lane == 0) {
        if (n_indel) atomicAdd(&counters[GP_WITH_INDEL], n_indel);
        if (n_ins) atomicAdd(&counters[GP_INSERTIONS], n_ins);
        if (n_del) atomicAdd(&counters[GP_DELETIONS], n_del);
    }
}

__global__ void __launch_bounds__(GP_BLOCK) k_gp_cigar(const uint32_t *__restrict__ list, uint64_t n_list, const uint32_t *__restrict__ runs,
                                                       const uint32_t *__restrict__ cigar_off, uint32_t *__restrict__ cigar) {
    const uint64_t n = n_list * (uint64_t) GP_MAX_RUNS;
    for (uint64_t u = (uint64_t) blockIdx.x * GP_BLOCK + threadIdx.x; u < n; u += (uint64_t) gridDim.x * GP_BLOCK) {
        const uint64_t i = u / GP_MAX_RUNS;
        const uint32_t w = (uint32_t) (u % GP_MAX_RUNS), r = list[i];
        const uint32_t a = cigar_off[r], b = cigar_off[r + 1];
        if (w < b - a) cigar[a + w] = runs[u];
    }
}

__global__ void __launch_bounds__(GP_BLOCK) k_gp_depth_add(SeedSpace t, const uint32_t *__restrict__ list, uint64_t n_list, GpOut o, uint32_t *__restrict__ diff,
                                                           unsigned long long *__restrict__ tstat) {
    for (uint64_t i = (uint64_t) blockIdx.x * GP_BLOCK + threadIdx.x; i < n_list; i += (uint64_t) gridDim.x * GP_BLOCK) {
        const uint32_t r = list[i];
        if (!(o.state[r] & GP_ST_UNIQUE)) continue;
        const uint32_t tt = (uint32_t) o.target[r];
        const uint32_t gp = t.off[tt] + (uint32_t) o.pos[r], ge = t.off[tt] + (uint32_t) o.end[r];     // ge <= col_off[tt + 1] <= columns: the array has columns + 1 entries
        atomicAdd(&diff[gp], 1u);
        atomicAdd(&diff[ge], 0xFFFFFFFFu);
        atomicAdd(&tstat[tt], 1ull);
        atomicAdd(&tstat[(size_t) t.n + tt], (unsigned long long) (ge - gp));
        atomicAdd(&tstat[2 * (size_t) t.n + tt], (unsigned long long) o.edits[r]);
    }
}

__global__ void __launch_bounds__(GP_BLOCK) k_gp_cover(const uint32_t *__restrict__ pl_cover, const uint32_t *__restrict__ scan, uint64_t columns, uint32_t *__restrict__ cover) {
    for (uint64_t g = (uint64_t) blockIdx.x * GP_BLOCK + threadIdx.x; g < columns; g += (uint64_t) gridDim.x * GP_BLOCK) cover[g] = pl_cover[g] + scan[g + 1];
}

// ---- the TSV -------------------------------------------------------------------------------------------------------------------------------
// `<read>\t<target>\t<pos>\t<end>\t<strand>\t<edits>\t<unique>\t<cigar>\n`
struct GpRecord {
    static constexpr bool kPacked = false, kAligned = false;
    TextHeader<7> h;
    uint32_t hb, nr;                                                  // bytes before the CIGAR, its runs
    const uint32_t *rn;
    uint32_t cb;
    __device__ __forceinline__ bool set(const GpTsv &f, uint64_t r) {
        const uint8_t st = f.state[r];
        if (!(st & GP_ST_PLACED)) return false;
        h.f[0] = text_field("", r); h.f[1] = text_field("\t", (uint64_t) f.target[r]); h.f[2] = text_field("\t", (uint64_t) f.pos[r]);
        h.f[3] = text_field("\t", (uint64_t) f.end[r]);
        if (st & GP_ST_MINUS) h.f[4] = text_field("\t-\t", (uint64_t) f.edits[r]); else h.f[4] = text_field("\t+\t", (uint64_t) f.edits[r]);
        h.f[5] = text_field("\t", (st & GP_ST_UNIQUE) ? 1ull : 0ull); h.f[6] = text_lit("\t");
        hb = h.bytes() - 1u;
        rn = f.cigar + f.cigar_off[r]; nr = f.cigar_off[r + 1] - f.cigar_off[r];
        cb = 0;
        for (uint32_t u = 0; u < nr; u++) cb += (uint32_t) dec_width(rn[u] >> 2) + 1u;
        return true;
    }
    __device__ __forceinline__ uint32_t bytes() const { return hb + cb + 1u; }
    __device__ __forceinline__ char at(uint32_t p) const {
        if (p < hb) return h.at(p);
        p -= hb;
        for (uint32_t u = 0; u < nr; u++) {
            const uint32_t ln = rn[u] >> 2, w = (uint32_t) dec_width(ln);
            if (p < w) return dec_digit(ln, w, p);
            if (p == w) return (char) ((0x44494Du >> (8 * (rn[u] & 3u))) & 0xFF);       // "MID"
            p -= w + 1u;
        }
        return '\n';
    }
};

__global__ void __launch_bounds__(GP_BLOCK) k_gp_tsv_sizes(GpTsv f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<GpRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(GP_BLOCK) k_gp_tsv_write(GpTsv f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<GpRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_gp_target_check(const int32_t *tlen, const uint32_t *col_off, uint64_t T, uint64_t columns, int32_t k, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_gp_target_check, dim3(stage_grid(T, GP_BLOCK, 4096)), dim3(GP_BLOCK), 0, s, tlen, col_off, T, columns, k, counters);
}

void launch_gp_flag(const SeedReads &r, const uint8_t *pl_state, int32_t k, uint32_t *flag, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_gp_flag, dim3(stage_grid(r.R + 1, GP_BLOCK, 8192)), dim3(GP_BLOCK), 0, s, r, pl_state, k, flag, counters);
}

void launch_gp_scatter(const uint32_t *flag, const uint32_t *pos, uint64_t R, uint32_t *list, hipStream_t s) {
    if (R) hipLaunchKernelGGL(k_gp_scatter, dim3(stage_grid(R, GP_BLOCK, 8192)), dim3(GP_BLOCK), 0, s, flag, pos, R, list);
}

void launch_gp_score(const SeedReads &r, const SeedSpace &t, const SeedIndex &x, int32_t k, int32_t E, int32_t max_occ, const uint32_t *list, uint64_t n_list, const GpOut &o,
                     unsigned long long *best, int blocks, unsigned long long *counters, hipStream_t s) {
    if (n_list) hipLaunchKernelGGL(k_gp_score, dim3((unsigned) blocks), dim3(GP_BLOCK), 0, s, r, t, x, k, E, (uint32_t) max_occ, list, n_list, o, best, counters);
}

void launch_gp_trace(const SeedReads &r, const SeedSpace &t, int32_t k, int32_t E, const uint32_t *list, uint64_t n_list, const unsigned long long *best, uint8_t *state,
                     uint32_t *runs, uint32_t *n_runs, unsigned long long *counters, hipStream_t s) {
    if (!n_list) return;
    const uint64_t g = (n_list + GP_TR_WAVES - 1) / GP_TR_WAVES;
    hipLaunchKernelGGL(k_gp_trace, dim3((unsigned) std::min<uint64_t>(g, 8192)), dim3(GP_TR_BLOCK), 0, s, r, t, k, E, list, n_list, best, state, runs, n_runs, counters);
}

void launch_gp_cigar(const uint32_t *list, uint64_t n_list, const uint32_t *runs, const uint32_t *cigar_off, uint32_t *cigar, hipStream_t s) {
    if (n_list) hipLaunchKernelGGL(k_gp_cigar, dim3(stage_grid(n_list * GP_MAX_RUNS, GP_BLOCK, 8192)), dim3(GP_BLOCK), 0, s, list, n_list, runs, cigar_off, cigar);
}

void launch_gp_depth_add(const SeedSpace &t, const uint32_t *list, uint64_t n_list, const GpOut &o, uint32_t *diff, unsigned long long *tstat, hipStream_t s) {
    if (n_list && t.n) hipLaunchKernelGGL(k_gp_depth_add, dim3(stage_grid(n_list, GP_BLOCK, 8192)), dim3(GP_BLOCK), 0, s, t, list, n_list, o, diff, tstat);
}

void launch_gp_cover(const uint32_t *pl_cover, const uint32_t *scan, uint64_t columns, uint32_t *cover, hipStream_t s) {
    if (columns) hipLaunchKernelGGL(k_gp_cover, dim3(stage_grid(columns, GP_BLOCK, 8192)), dim3(GP_BLOCK), 0, s, pl_cover, scan, columns, cover);
}

void launch_gp_tsv_sizes(const GpTsv &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_gp_tsv_sizes, dim3(text_sizes_blocks(f.n, GP_BLOCK)), dim3(GP_BLOCK), 0, s, f, sizes, counters);
}

void launch_gp_tsv_write(const GpTsv &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_gp_tsv_write, dim3(text_write_blocks(i0, i1, GP_WAVES)), dim3(GP_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
