// alga_amd/csrc/contain_kernels.hip -- contigs contained in another contig dropped (include/alga_amd.h: alga_drop_contained_device; the
// definition is the comment there, host side in engine_contain.hip).
//
// The T targets are copied into one padded 2-bit array in a column space of their own (target t at off[t], a multiple of 16), and next to it
// their reverse complements at the same columns: both query strings of a target are word-aligned rows, and a container is a stretch of the
// forward array.  Integer work only, wave-64, nothing depends on thread order or on the sort's order among equal keys.
//   k_ct_check        a negative length -> the refusal flag; the column sum, the padded lengths and their sum, the indexed positions, the queries
//   (scan): off
//   k_ct_cols         the targets and their reverse complements, one thread per word
//   (the index over the forward columns: alga_seed_index, seed_index.hip)
//   k_ct_contain      one wave per (c, s): lanes look the at most 64 seeds up (one chunk: the scratch of seed_device.h is never touched), the
//                     usable mask is one ballot.  The (seed, occurrence) candidates are taken one after the other by the WHOLE wave: host, p,
//                     order and bounds are wave-uniform; lane j' < j asks whether usable seed j' matches at the same p (one ballot: a placement
//                     counts once and is verified once); then lane i compares words i, i + 64, ... of the query row with the funnel-shifted
//                     host words (verify_prefix's arithmetic), a wave sum follows each pass of 64 words and the wave leaves past M(n).  Best
//                     and hits are wave-uniform scalars.
//   k_ct_decide       one thread per target: the two orientations into item 4
//   k_ct_root_init / k_ct_root_jump   double-buffered pointer jumping over (root, pos, orient), one launch per round
//   k_ct_absorbed     an integer atomic per contained target
//   k_ct_number       (after the scan of the kept flags) new ids, old ids, the kept lengths
//   k_ct_build        (after the scan of the kept lengths) every output word gathered by one lane
//   k_ct_fasta_sizes / k_ct_fasta_write   one record per kept target, one wave per record
// The kernels carry the prefix k_ct_ inside this file's unnamed namespace (contig_kernels.hip has kernels of that prefix in its own); what the
// host sees of this stage is named Cn / CN_ / launch_cn_ / cn_, apart from the contig stage's Ct / CT_ / launch_ct_ / ct_.
// No LDS.  Block 256 and the grid caps are picked, not tuned; CnTargets::max_blocks lowers the cap of every grid that goes through stage_grid
// (option "contain_max_blocks": a knob of the tests, which make every grid-stride loop here take further passes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "contain_kernels.h"
#include "seed_device.h"
#include "text_record.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int CN_BLOCK = 256, CN_WAVES = CN_BLOCK / 64;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t) __shfl_xor((int) v, o);
    return v;
}

__global__ void __launch_bounds__(CN_BLOCK) k_ct_check(CnTargets t, int32_t k, uint32_t *__restrict__ pad, unsigned long long *__restrict__ counters) {
    unsigned long long sum = 0, psum = 0, idx = 0, queries = 0, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; i <= t.T; i += (uint64_t) gridDim.x * CN_BLOCK) {
        int32_t n = i < t.T ? t.len[i] : 0;
        if (n < 0) { bad = CN_BAD_LEN; n = 0; }
        const uint32_t p = ((uint32_t) n + 15u) & ~15u;
        pad[i] = p;                                                           // entry T: the place of the scan's total
        sum += (unsigned long long) n; psum += p;
        if (n >= k) { idx += (unsigned long long) (n - k + 1); queries++; }
    }
    sum = wave_sum(sum); psum = wave_sum(psum); idx = wave_sum(idx); queries = wave_sum(queries); bad = wave_max(bad);
    if ((threadIdx.x & 63) == 0) {
        if (sum) { atomicAdd(&counters[CN_COLUMNS], sum); atomicAdd(&counters[CN_PAD_COLUMNS], psum); }
        if (idx) { atomicAdd(&counters[CN_INDEX_POS], idx); atomicAdd(&counters[CN_QUERIES], queries); }
        if (bad) atomicOr(&counters[CN_BAD], bad);
    }
}

// (every target begins a word, so a word lies in one target; the words behind a target's last base and the two of the padding stay zero)
__global__ void __launch_bounds__(CN_BLOCK) k_ct_cols(CnTargets t, CnSpace sp, uint32_t *__restrict__ cols, uint32_t *__restrict__ rcols) {
    const uint64_t n_words = sp.columns >> 4;
    for (uint64_t w = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; w < n_words; w += (uint64_t) gridDim.x * CN_BLOCK) {
        const uint32_t g0 = (uint32_t) (w << 4), c = item_of(sp.off, sp.n, g0), q0 = g0 - sp.off[c], n = (uint32_t) sp.len[c];
        const uint64_t b0 = t.begin[c];
        uint32_t vf = 0, vr = 0;
        for (uint32_t j = 0; j < 16 && q0 + j < n; j++) {
            const uint32_t q = q0 + j;
            vf |= base_at(t.words, b0 + q) << (2 * j);
            vr |= (3u - base_at(t.words, b0 + (n - 1u - q))) << (2 * j);
        }
        cols[w] = vf; rcols[w] = vr;
    }
}

__global__ void __launch_bounds__(CN_BLOCK) k_ct_contain(CnSpace sp, SeedIndex ix, int32_t k, uint32_t max_permille, uint32_t max_occ, CnQueryOut out,
                                                         unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint32_t wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint64_t wave = (uint64_t) blockIdx.x * CN_WAVES + wv, n_waves = (uint64_t) gridDim.x * CN_WAVES;
    unsigned long long n_seeds = 0, n_over = 0, n_cand = 0;                     // wave-uniform
    for (uint64_t x = wave; x < 2ull * sp.n; x += n_waves) {
        const uint32_t c = (uint32_t) (x >> 1), s = (uint32_t) (x & 1ull);
        const int32_t n = sp.len[c];
        uint32_t best_mm = 0xFFFFFFFFu, best_p = 0, hits = 0;
        int32_t best_h = -1;
        if (n >= k) {                                        // (wave-uniform) a shorter target has no seed: no container
            const int S = std::min(n / k, 64);
            const uint32_t M = (uint32_t) (((unsigned long long) n * max_permille) / 1000ull);
            const uint32_t c0 = sp.off[c];
            const uint32_t *qrow = (s ? sp.rcols : sp.cols) + (c0 >> 4);
            const int nw = blocks_of(n);
            const bool act = lane < S;
            unsigned long long kmer = 0;
            uint32_t lb = 0, occ = 0;
            if (act) { kmer = row_kmer(qrow, nw, lane * k, k); seed_lookup(ix, kmer, max_occ, lb, occ); }
            const bool usable = act && occ >= 1u && occ <= max_occ;
            const unsigned long long umask = __ballot(usable);
            n_seeds += (unsigned long long) S;
            n_over += (unsigned long long) __popcll(__ballot(act && occ > max_occ));
            for (unsigned long long m = umask; m; m &= m - 1ull) {
                const int j = __builtin_ctzll(m);
                const uint32_t lb_j = (uint32_t) __builtin_amdgcn_readfirstlane(__shfl((int) lb, j)), occ_j = (uint32_t) __builtin_amdgcn_readfirstlane(__shfl((int) occ, j));
                const uint32_t jk = (uint32_t) (j * k);
                for (uint32_t o = 0; o < occ_j; o++) {
                    // geometry, wave-uniform: seed j at column g of host h puts the query's base 0 on p = g - off[h] - j k
                    const uint32_t g = ix.vals[lb_j + o];
                    if (g - c0 < (uint32_t) n) continue;     // the query's own k-mer (h == c), the usual occurrence: no bisection for it
                    const uint32_t h = item_of(sp.off, sp.n, g), h0 = sp.off[h], q = g - h0;
                    const int32_t hl = sp.len[h];
                    if (h == c || q < jk) continue;
                    if (!(hl > n || (hl == n && h < c))) continue;
                    const uint32_t p = q - jk;
                    if ((unsigned long long) p + (unsigned long long) n > (unsigned long long) hl) continue;
                    const uint32_t gp = h0 + p;
                    // an earlier usable seed finds this placement too: it counted there (lane j' < j: bases up to gp + j k are read)
                    const bool dup = lane < j && usable && kmer == col_kmer(sp.cols, gp + (uint32_t) (lane * k), k);
                    if (__ballot(dup)) continue;
                    n_cand++;
                    // the n bases, 64 words a pass; word (gp >> 4) + nw is the last one read: inside the padding
                    const uint32_t *tw = sp.cols + (gp >> 4);
                    const uint32_t sh = (gp & 15u) << 1;
                    uint32_t mm = 0;
                    for (int w0 = 0; w0 < nw && mm <= M; w0 += 64) {
                        const int w = w0 + lane;
                        uint32_t part = 0;
                        if (w < nw) {
                            uint32_t d = qrow[w] ^ __funnelshift_r(tw[w], tw[w + 1], sh);
                            if (w == nw - 1 && (n & 15)) d &= (1u << ((n & 15) << 1)) - 1u;
                            part = (uint32_t) __popc((d | (d >> 1)) & 0x55555555u);
                        }
                        mm += wave_sum_u32(part);
                    }
                    if (mm > M) continue;
                    hits = hits < CN_HITS_CAP ? hits + 1u : hits;
                    if (mm < best_mm || (mm == best_mm && ((int32_t) h < best_h || ((int32_t) h == best_h && p < best_p)))) { best_mm = mm; best_h = (int32_t) h; best_p = p; }
                }
            }
        }
        if (lane == 0) { out.mm[x] = best_mm; out.hits[x] = hits; out.host[x] = best_h; out.pos[x] = (int32_t) best_p; }
    }
    if (lane == 0) {
        if (n_seeds) atomicAdd(&counters[CN_SEEDS], n_seeds);
        if (n_over) atomicAdd(&counters[CN_SEEDS_OVER], n_over);
        if (n_cand) atomicAdd(&counters[CN_CANDIDATES], n_cand);
    }
}

// (after the check: no length is negative; host[x] < T wherever hits[x] > 0)
__global__ void __launch_bounds__(CN_BLOCK) k_ct_decide(CnTargets t, CnQueryOut q, CnOut o, uint32_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
    unsigned long long n_con = 0, n_minus = 0, n_dup = 0, n_amb = 0, n_sat = 0, n_kept = 0, removed = 0, longest = 0, after = 0, longest_kept = 0;
    for (uint64_t c = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; c <= t.T; c += (uint64_t) gridDim.x * CN_BLOCK) {
        if (c == t.T) { keep[c] = 0; continue; }                                // the place of the scan's total
        const uint32_t n = (uint32_t) t.len[c];
        const uint32_t h0 = q.hits[2 * c], h1 = q.hits[2 * c + 1], hits = h0 + h1;
        int32_t host = -1, pos = 0;
        uint32_t mm = 0;
        uint8_t orient = 0, st = 0;
        if (hits) {
            // the smallest (mm, h, p, s)
            const uint32_t m0 = q.mm[2 * c], m1 = q.mm[2 * c + 1];
            const int32_t a0 = q.host[2 * c], a1 = q.host[2 * c + 1], p0 = q.pos[2 * c], p1 = q.pos[2 * c + 1];
            const bool second = !h0 || (h1 && (m1 < m0 || (m1 == m0 && (a1 < a0 || (a1 == a0 && p1 < p0)))));
            host = second ? a1 : a0; pos = second ? p1 : p0; mm = second ? m1 : m0; orient = second ? 1 : 0;
            const bool dup = (uint32_t) t.len[host] == n;
            st = (uint8_t) (CN_CONTAINED_BIT | (second ? CN_MINUS_BIT : 0) | (hits > 1u ? CN_AMBIGUOUS_BIT : 0) | (dup ? CN_DUPLICATE_BIT : 0));
            n_con++; n_minus += second; n_dup += dup; n_amb += hits > 1u; n_sat += hits > 255u; removed += n; longest = n > longest ? n : longest;
        } else if (n) {
            st = CN_KEPT_BIT;
            n_kept++; after += n; longest_kept = n > longest_kept ? n : longest_kept;
        }
        o.host[c] = host; o.host_pos[c] = pos; o.host_orient[c] = orient; o.mm[c] = mm; o.hits[c] = (uint8_t) (hits > 255u ? 255u : hits); o.state[c] = st;
        keep[c] = (st & CN_KEPT_BIT) ? 1u : 0u;
    }
    n_con = wave_sum(n_con); n_minus = wave_sum(n_minus); n_dup = wave_sum(n_dup); n_amb = wave_sum(n_amb); n_sat = wave_sum(n_sat); n_kept = wave_sum(n_kept);
    removed = wave_sum(removed); after = wave_sum(after); longest = wave_max(longest); longest_kept = wave_max(longest_kept);
    if ((threadIdx.x & 63) == 0) {
        if (n_con) {
            atomicAdd(&counters[CN_CONTAINED], n_con); atomicAdd(&counters[CN_REMOVED], removed); atomicMax(&counters[CN_LONGEST_CONTAINED], longest);
            if (n_minus) atomicAdd(&counters[CN_MINUS], n_minus);
            if (n_dup) atomicAdd(&counters[CN_DUPLICATES], n_dup);
            if (n_amb) atomicAdd(&counters[CN_AMBIGUOUS], n_amb);
            if (n_sat) atomicAdd(&counters[CN_SATURATED], n_sat);
        }
        if (n_kept) { atomicAdd(&counters[CN_KEPT], n_kept); atomicAdd(&counters[CN_COLUMNS_AFTER], after); atomicMax(&counters[CN_LONGEST_KEPT], longest_kept); }
    }
}

// a kept target is its own root; a target of length 0 has none
__global__ void __launch_bounds__(CN_BLOCK) k_ct_root_init(CnTargets t, CnOut o, CnRoots a) {
    for (uint64_t c = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; c < t.T; c += (uint64_t) gridDim.x * CN_BLOCK) {
        const uint8_t st = o.state[c];
        const bool con = st & CN_CONTAINED_BIT;
        a.root[c] = con ? o.host[c] : ((st & CN_KEPT_BIT) ? (int32_t) c : -1);
        a.pos[c] = con ? o.host_pos[c] : 0;
        a.orient[c] = con ? o.host_orient[c] : (uint8_t) 0;
    }
}

// c lies in r = a.root[c] at (p, s) and r in g = a.root[r] at (p', s'): c lies in g at p' + p with s, or, where r is turned over, at
// p' + len[r] - p - len[c] with s xor 1.  Reads a, writes b: no thread reads what another writes.
__global__ void __launch_bounds__(CN_BLOCK) k_ct_root_jump(CnTargets t, CnRoots a, CnRoots b) {
    for (uint64_t c = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; c < t.T; c += (uint64_t) gridDim.x * CN_BLOCK) {
        int32_t r = a.root[c], p = a.pos[c];
        uint8_t s = a.orient[c];
        if (r >= 0 && (uint64_t) r != c) {
            const int32_t g = a.root[r];
            if (g != r) {
                const int32_t pp = a.pos[r];
                if (a.orient[r]) { p = pp + t.len[r] - p - t.len[c]; s ^= 1; }
                else p = pp + p;
                r = g;
            }
        }
        b.root[c] = r; b.pos[c] = p; b.orient[c] = s;
    }
}

__global__ void __launch_bounds__(CN_BLOCK) k_ct_absorbed(CnTargets t, CnOut o, CnRoots r, uint32_t *__restrict__ absorbed) {
    for (uint64_t c = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; c < t.T; c += (uint64_t) gridDim.x * CN_BLOCK)
        if (o.state[c] & CN_CONTAINED_BIT) atomicAdd(&absorbed[r.root[c]], 1u);
}

// (keep_scan: the exclusive scan of keep; a kept target writes its own entries of d_old and klen)
__global__ void __launch_bounds__(CN_BLOCK) k_ct_number(CnTargets t, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ keep_scan, int32_t *__restrict__ d_new,
                                                        int32_t *__restrict__ d_old, int32_t *__restrict__ klen) {
    for (uint64_t c = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; c < t.T; c += (uint64_t) gridDim.x * CN_BLOCK) {
        const bool kept = keep[c] != 0;
        const uint32_t j = keep_scan[c];
        d_new[c] = kept ? (int32_t) j : -1;
        if (kept) { d_old[j] = (int32_t) c; klen[j] = t.len[c]; }
    }
}

// (col_off is the scan of the kept lengths, columns its total; every kept target has a length)
__global__ void __launch_bounds__(CN_BLOCK) k_ct_build(CnTargets t, const int32_t *__restrict__ d_old, const uint32_t *__restrict__ col_off, uint32_t n_kept, uint64_t columns,
                                                       uint32_t *__restrict__ words, unsigned long long *__restrict__ begin) {
    for (uint64_t i = (uint64_t) blockIdx.x * CN_BLOCK + threadIdx.x; i < n_kept; i += (uint64_t) gridDim.x * CN_BLOCK) begin[i] = col_off[i];
    packed_words_body<CN_BLOCK>(col_off, n_kept, columns, ((columns + 15) >> 4) + 2, words, [&](uint32_t j, uint32_t q) { return base_at(t.words, t.begin[d_old[j]] + q); });
}

// ---- FASTA of the kept contigs ---------------------------------------------------------------------------------------------------------
// `>contig_id=<j>_length=<len>_absorbed=<m>\n<kept contig>\n`
struct CnRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const CnFasta &f, uint64_t j) {
        const int32_t len = f.len[j];
        if (len <= 0) return false;
        contig_head(j, (uint32_t) len);
        h.f[2] = text_field("_absorbed=", (uint64_t) f.absorbed[f.old[j]]); seal();
        seq.row = f.words; seq.q0 = f.col_off[j];
        return true;
    }
};

__global__ void __launch_bounds__(CN_BLOCK) k_ct_fasta_sizes(CnFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<CnRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(CN_BLOCK) k_ct_fasta_write(CnFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<CnRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_cn_check(const CnTargets &t, int32_t k, uint32_t *pad, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_ct_check, dim3(stage_grid((uint64_t) t.T + 1, CN_BLOCK, std::min<uint64_t>(4096, t.max_blocks))), dim3(CN_BLOCK), 0, s, t, k, pad, counters);
}

void launch_cn_cols(const CnTargets &t, const CnSpace &sp, uint32_t *cols, uint32_t *rcols, hipStream_t s) {
    if (sp.columns) hipLaunchKernelGGL(k_ct_cols, dim3(stage_grid(sp.columns >> 4, CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, sp, cols, rcols);
}

void launch_cn_contain(const CnSpace &sp, const SeedIndex &x, int32_t k, int32_t max_permille, int32_t max_occ, const CnQueryOut &q, int blocks, unsigned long long *counters,
                       hipStream_t s) {
    if (sp.n) hipLaunchKernelGGL(k_ct_contain, dim3((unsigned) blocks), dim3(CN_BLOCK), 0, s, sp, x, k, (uint32_t) max_permille, (uint32_t) max_occ, q, counters);
}

void launch_cn_decide(const CnTargets &t, const CnQueryOut &q, const CnOut &o, uint32_t *keep, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_ct_decide, dim3(stage_grid((uint64_t) t.T + 1, CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, q, o, keep, counters);
}

void launch_cn_root_init(const CnTargets &t, const CnOut &o, const CnRoots &a, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_ct_root_init, dim3(stage_grid(t.T, CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, o, a);
}

void launch_cn_root_jump(const CnTargets &t, const CnRoots &a, const CnRoots &b, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_ct_root_jump, dim3(stage_grid(t.T, CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, a, b);
}

void launch_cn_absorbed(const CnTargets &t, const CnOut &o, const CnRoots &r, uint32_t *absorbed, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_ct_absorbed, dim3(stage_grid(t.T, CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, o, r, absorbed);
}

void launch_cn_number(const CnTargets &t, const uint32_t *keep, const uint32_t *keep_scan, int32_t *d_new, int32_t *d_old, int32_t *klen, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_ct_number, dim3(stage_grid(t.T, CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, keep, keep_scan, d_new, d_old, klen);
}

void launch_cn_build(const CnTargets &t, const int32_t *d_old, const uint32_t *col_off, uint32_t n_kept, uint64_t columns, uint32_t *words, unsigned long long *begin,
                     hipStream_t s) {
    const uint64_t n_words = ((columns + 15) >> 4) + 2;
    hipLaunchKernelGGL(k_ct_build, dim3(stage_grid(std::max<uint64_t>(n_words, n_kept), CN_BLOCK, t.max_blocks)), dim3(CN_BLOCK), 0, s, t, d_old, col_off, n_kept, columns, words, begin);
}

void launch_cn_fasta_sizes(const CnFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_ct_fasta_sizes, dim3(text_sizes_blocks(f.n, CN_BLOCK)), dim3(CN_BLOCK), 0, s, f, sizes, counters);
}

void launch_cn_fasta_write(const CnFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_ct_fasta_write, dim3(text_write_blocks(i0, i1, CN_WAVES)), dim3(CN_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
