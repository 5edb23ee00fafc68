// alga_amd/csrc/seed_device.h -- device side of the seed index (seed_index.h): the k-mers of packed 2-bit arrays, the look-up, the
// verification, and the wave loop that seeds a query and verifies what the seeds find (item_of and base_at: packed_device.h).  Included by the
// *_kernels.hip files only; everything here is internal to the including file (the build has no relocatable device code).
//
// seed_and_verify: one wave, one query of S seeds (seed j is the k-mer at base j k of the query), one SeedIndex over a column array.  Lanes
// take seeds, 64 at a time: one directory read, a bisection to the lower bound, a scan of at most max_occ + 1 equal keys; a seed with 1 ..
// max_occ occurrences is usable.  The (seed, occurrence) candidates of the usable seeds go to the lanes in passes of 64 (a wave scan of the
// occurrence counts, a bisection over it by cross-lane reads).  The stage's geometry turns (seed, indexed column) into the first column gp the
// query would lie on and the bases to compare, or rejects it; a lane verifies its candidate by XOR and popcount over funnel-shifted column
// words and leaves past max_mm.  A candidate found through seed j counts only if no usable seed j' < j matches at gp too: every placement
// counts once, no duplicates, no sort.  The rows are read from memory (every lane reads the same word), so a query has no length cap; one
// with more than 64 seeds keeps the usable masks of its earlier chunks in a per-wave piece of global scratch.  What differs between the
// stages enters as
//   Query     kmer(j): the k-mer of seed j;  row: the query's packed bases, word aligned (what verify_prefix compares)
//   Geometry  operator()(js, g, gp, n, low): false, or gp, the n bases to verify, the key below the mismatches;  kMmShift: where they go
//   Tally     add(mm): what the lane keeps of a placement that counts
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seed_index.h"
#include "packed_device.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) v, o), hi = (uint32_t) __shfl_xor((int) (uint32_t) (v >> 32), o);
        const unsigned long long w = ((unsigned long long) hi << 32) | lo;
        v = w < v ? w : v;
    }
    return v;
}

// the k-mer at column g of a column array (two words of padding behind the last column)
__device__ __forceinline__ unsigned long long col_kmer(const uint32_t *__restrict__ cols, uint32_t g, int k) {
    const uint32_t w = g >> 4, sh = (g & 15u) << 1;
    const unsigned long long lo = (unsigned long long) cols[w] | ((unsigned long long) cols[w + 1] << 32);
    unsigned long long v = lo >> sh;
    if (sh) v |= (unsigned long long) cols[w + 2] << (64 - sh);
    return v & ((1ull << (2 * k)) - 1ull);
}

// the k-mer at base i of a row of nw words (i + k <= its length: nothing is read past word nw - 1)
__device__ __forceinline__ unsigned long long row_kmer(const uint32_t *__restrict__ row, int nw, int i, int k) {
    const int w = i >> 4, sh = (i & 15) << 1;
    const unsigned long long lo = (unsigned long long) row[w] | (w + 1 < nw ? (unsigned long long) row[w + 1] << 32 : 0ull);
    unsigned long long v = lo >> sh;
    if (sh && w + 2 < nw) v |= (unsigned long long) row[w + 2] << (64 - sh);
    return v & ((1ull << (2 * k)) - 1ull);
}

// lower bound of kmer among the indexed keys and its occurrences, counted up to max_occ + 1
__device__ __forceinline__ void seed_lookup(const SeedIndex &x, unsigned long long kmer, uint32_t max_occ, uint32_t &lb, uint32_t &occ) {
    const uint32_t b = (uint32_t) (kmer >> x.shift);
    uint32_t lo = x.dir[b], hi = x.dir[b + 1];
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (x.keys[mid] < kmer) lo = mid + 1; else hi = mid;
    }
    lb = lo;
    uint32_t c = 0;
    while (lo + c < end && c <= max_occ && x.keys[lo + c] == kmer) c++;
    occ = c;
}

// Hamming distance between the first n bases of a word-aligned row and the n columns from gp on; stops past max_mm.  Words 0 .. blocks_of(n) - 1
// of the row and up to one word more of the columns are read (gp + n <= the columns: inside the padding); the bases from n on are masked away
__device__ __forceinline__ uint32_t verify_prefix(const uint32_t *__restrict__ row, int n, const uint32_t *__restrict__ cols, uint32_t gp, uint32_t max_mm) {
    const uint32_t *tw = cols + (gp >> 4);
    const uint32_t sh = (gp & 15u) << 1;
    const int nw = blocks_of(n);
    uint32_t mm = 0, prev = tw[0];
    for (int w = 0; w < nw; w++) {
        const uint32_t next = tw[w + 1];
        uint32_t x = row[w] ^ __funnelshift_r(prev, next, sh);
        prev = next;
        if (w == nw - 1 && (n & 15)) x &= (1u << ((n & 15) << 1)) - 1u;
        mm += (uint32_t) __popc((x | (x >> 1)) & 0x55555555u);
        if (mm > max_mm) break;
    }
    return mm;
}

// Query: a row of nw words in memory
struct RowQuery {
    const uint32_t *row;
    int nw, k;
    __device__ __forceinline__ unsigned long long kmer(int j) const { return row_kmer(row, nw, j * k, k); }
};

// Tally: the smallest mm among the lane's placements and how many have it
struct MinMmTally {
    uint32_t mm = 0xFFFFFFFFu, cnt = 0;
    __device__ __forceinline__ void add(uint32_t m) {
        if (m < mm) { mm = m; cnt = 1u; }
        else if (m == mm) cnt++;
    }
};

// best: the minimum key of this lane's placements; n_seeds / n_over: the seeds looked up and those with more than max_occ occurrences
// (wave-uniform); ub: this wave's scratch, touched only where S > 64
template <class Query, class Geometry, class Tally>
__device__ __forceinline__ void seed_and_verify(const SeedIndex &x, const uint32_t *__restrict__ cols, int k, uint32_t max_mm, uint32_t max_occ, int S, const Query &q,
                                                const Geometry &geo, unsigned long long *ub, unsigned long long &best, Tally &tally, unsigned long long &n_seeds,
                                                unsigned long long &n_over) {
    const int lane = threadIdx.x & 63;
    for (int c0 = 0; c0 < S; c0 += 64) {
        const int j = c0 + lane;
        const bool act = j < S;
        uint32_t lb = 0, occ = 0;
        if (act) seed_lookup(x, q.kmer(j), max_occ, lb, occ);
        const bool usable = act && occ >= 1u && occ <= max_occ;
        const unsigned long long umask = __ballot(usable);
        n_seeds += (unsigned long long) __popcll(__ballot(act));
        n_over += (unsigned long long) __popcll(__ballot(act && occ > max_occ));
        if (S > 64) {                        // later chunks ask for this one's usable seeds
            if (lane == 0) __hip_atomic_store(&ub[c0 >> 6], umask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
        }
        const uint32_t mine = usable ? occ : 0u;
        uint32_t inc = mine;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t) __shfl_up((int) inc, d); if (lane >= d) inc += up; }
        const uint32_t C = (uint32_t) __shfl((int) inc, 63), exc = inc - mine;
        for (uint32_t p0 = 0; p0 < C; p0 += 64) {
            const bool cact = p0 + (uint32_t) lane < C;
            const uint32_t ci = cact ? p0 + (uint32_t) lane : C - 1u;
            int sl = 0;                      // the seed lane of candidate ci: the first with inc > ci
            for (int st = 32; st > 0; st >>= 1) if ((uint32_t) __shfl((int) inc, sl + st - 1) <= ci) sl += st;
            const uint32_t s_lb = (uint32_t) __shfl((int) lb, sl), s_exc = (uint32_t) __shfl((int) exc, sl);
            if (!cact) continue;
            const int js = c0 + sl;
            const uint32_t g = x.vals[s_lb + (ci - s_exc)];
            uint32_t gp;
            int n;
            unsigned long long low;
            if (!geo(js, g, gp, n, low)) continue;
            const uint32_t mm = verify_prefix(q.row, n, cols, gp, max_mm);
            if (mm > max_mm) continue;
            bool dup = false;                // an earlier usable seed finds this placement too
            for (int j2 = 0; j2 < js && !dup; j2++) {
                const unsigned long long m = j2 >= c0 ? umask : __hip_atomic_load(&ub[j2 >> 6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((m >> (j2 & 63)) & 1ull) dup = q.kmer(j2) == col_kmer(cols, gp + (uint32_t) (j2 * k), k);
            }
            if (dup) continue;
            const unsigned long long key = ((unsigned long long) mm << Geometry::kMmShift) | low;
            best = key < best ? key : best;
            tally.add(mm);
        }
    }
}

}  // namespace

}  // namespace alga
