// alga_amd/csrc/unitig_kernels.hip -- the unitig graph of an overlap graph (include/alga_amd.h: alga_unitigs_device).
//
// Integer work only, one thread per node / edge / output word.  The pipeline (host side: engine_unitig.hip):
//   k_ut_check        ids, live ends, dovetail offsets, twin lengths -> one flag word (nothing else is written on a refusal)
//   k_ut_twins        every edge and its twin as (src << 32 | dst, offset << 1 | is_twin) -> the engine's edge sort
//   k_ut_group_heads  first record of each (src, dst) and the group's smallest offset -> scan -> k_ut_compact_edges: E*
//   k_ut_next/_prev   the compactable edge out of / into every node (E* is twin-symmetric: indeg(v) = outdeg(v^1), prev[v] = next[v^1]^1)
//   k_ut_rank_jump    list ranking by pointer jumping towards the head: (ancestor, rank, pos, done) in ONE 16-byte record per node,
//                     ping-pong between two arrays (a round reads only the previous round's records: no torn or half-updated record
//                     is ever read), the host stops when the number of unresolved nodes no longer falls
//   k_ut_ruler_*      from 2^16 nodes on (option "unitig_ruling") a RULING SET is ranked first: the heads and one node in 64 walk along next[] to
//                     the next ruler, the rulers alone are ranked by k_ut_rank_jump (a list 1/64 as long, cache-resident), a second walk writes the
//                     final records of the nodes in between: ~3 gathers per node instead of one per node and round
//   k_ut_min_jump     what is still unresolved lies on cycles of compactable edges: the same jumping with min finds the smallest pair,
//   k_ut_cut          the two cuts are made and only those nodes are ranked again
//   k_ut_tails .. k_ut_layout   numbering (flag the heads that win, scan), sizes per pair, the path arrays by (pair, rank)
//   k_ut_sequence     one lane per output word of the ragged 2-bit rows: binary search of its pair, of its first node, then the at most
//                     16 bases from as many nodes as they span -- a gather, every word written once, no atomics
//   k_ut_edges        one thread per edge of E* that is not compactable -> (key, value) for the edge sort
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "unitig_kernels.h"

namespace alga {

namespace {

constexpr int UT_BLOCK = 256;

__device__ __forceinline__ unsigned long long ut_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long ut_wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ int32_t sat_add(int32_t a, int32_t b) {
    const int64_t s = (int64_t) a + b;
    return s > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t) s;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_check(const int32_t *__restrict__ len, int32_t n, const alga_edge_dev *__restrict__ e, uint64_t m,
                                                       unsigned long long *__restrict__ counters) {
    const uint64_t items = m > (uint64_t) n ? m : (uint64_t) n;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (uint64_t) gridDim.x * blockDim.x) {
        if (i < (uint64_t) n) {
            const int32_t L = len[i];
            if (L < 0 || L >= (1 << 30)) bad |= UT_BAD_LEN;
            if ((i & 1) && len[i - 1] != L) bad |= UT_BAD_TWIN_LEN;
        }
        if (i < m) {
            const alga_edge_dev x = e[i];
            if (x.src < 0 || x.src >= n || x.dst < 0 || x.dst >= n) { bad |= UT_BAD_ID; continue; }
            const int32_t la = len[x.src], lb = len[x.dst];
            if (la <= 0 || lb <= 0) { bad |= UT_BAD_DEAD; continue; }
            if (x.offset < 0 || x.offset >= la || (int64_t) x.offset + lb < (int64_t) la) bad |= UT_BAD_DOVETAIL;
        }
    }
    if (bad) atomicOr(&counters[UT_FLAGS], bad);
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_twins(const int32_t *__restrict__ len, const alga_edge_dev *__restrict__ e, uint64_t m,
                                                       unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t) gridDim.x * blockDim.x) {
        const alga_edge_dev x = e[i];
        keys[i] = ((unsigned long long) (uint32_t) x.src << 32) | (uint32_t) x.dst;
        vals[i] = (uint32_t) x.offset << 1;
        keys[m + i] = ((unsigned long long) (uint32_t) (x.dst ^ 1) << 32) | (uint32_t) (x.src ^ 1);
        vals[m + i] = ((uint32_t) (len[x.dst] - len[x.src] + x.offset) << 1) | 1u;
    }
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_group_heads(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t m2,
                                                             uint32_t *__restrict__ flag, uint32_t *__restrict__ best,
                                                             unsigned long long *__restrict__ counters) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long added = 0;
    if (i < m2) {
        const unsigned long long k = keys[i];
        const bool head = i == 0 || keys[i - 1] != k;
        flag[i] = head ? 1u : 0u;
        if (head) {
            uint32_t mn = vals[i], all_twin = mn & 1u;
            for (uint64_t j = i + 1; j < m2 && keys[j] == k; j++) { const uint32_t v = vals[j]; mn = v < mn ? v : mn; all_twin &= v; }
            best[i] = mn >> 1;
            added = all_twin;
        }
    }
    added = ut_wave_sum(added);
    if ((threadIdx.x & 63) == 0 && added) atomicAdd(&counters[UT_TWINS_ADDED], added);
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_compact_edges(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ flag,
                                                               const uint32_t *__restrict__ pos, const uint32_t *__restrict__ best, uint64_t m2,
                                                               alga_edge_dev *__restrict__ estar) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m2 || !flag[i]) return;
    alga_edge_dev x;
    x.src = (int32_t) (keys[i] >> 32); x.dst = (int32_t) (uint32_t) keys[i]; x.offset = (int32_t) best[i];
    estar[pos[i]] = x;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_next(const alga_edge_dev *__restrict__ estar, const uint32_t *__restrict__ rowptr, int32_t n,
                                                      int32_t *__restrict__ nxt, int32_t *__restrict__ noff) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    int32_t to = -1, off = 0;
    const uint32_t r0 = rowptr[v];
    if (rowptr[v + 1] - r0 == 1) {
        const alga_edge_dev x = estar[r0];
        const int32_t w = x.dst;
        // indeg(w) == outdeg(w ^ 1)
        if (w != v && w != (v ^ 1) && rowptr[(w ^ 1) + 1] - rowptr[w ^ 1] == 1) { to = w; off = x.offset; }
    }
    nxt[v] = to; noff[v] = off;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_prev(const int32_t *__restrict__ nxt, int32_t n, int32_t *__restrict__ prv) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    const int32_t t = nxt[v ^ 1];
    prv[v] = t < 0 ? -1 : (t ^ 1);
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_rank_init(const int32_t *__restrict__ len, const int32_t *__restrict__ prv, const int32_t *__restrict__ noff,
                                                           int32_t n, int only_unresolved, UtRank *__restrict__ a) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    if (only_unresolved && a[v].done) return;
    const int32_t p = len[v] > 0 ? prv[v] : -1;
    UtRank r;
    if (p < 0) { r.up = v; r.rank = 0; r.pos = 0; r.done = 1; }
    else { r.up = p; r.rank = 1; r.pos = noff[p]; r.done = 0; }
    a[v] = r;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_rank_jump(const UtRank *__restrict__ a, UtRank *__restrict__ b, int32_t n,
                                                           unsigned long long *__restrict__ unresolved) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    unsigned long long open = 0;
    if (v < n) {
        UtRank r = a[v];
        if (!r.done) {
            const UtRank u = a[r.up];                                 // one 16-byte load
            r.rank += u.rank; r.pos = sat_add(r.pos, u.pos); r.up = u.up; r.done = u.done;
            open = !r.done;
        }
        b[v] = r;
    }
    open = ut_wave_sum(open);
    if ((threadIdx.x & 63) == 0 && open) atomicAdd(unresolved, open);
}

// ---- ruling set ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ut_sampled(int32_t v) { return (((uint32_t) v * 0x9E3779B1u) >> 26) == 0; }      // one id in 64

__global__ void __launch_bounds__(UT_BLOCK) k_ut_ruler_flags(const int32_t *__restrict__ len, const int32_t *__restrict__ prv, int32_t n,
                                                             uint32_t *__restrict__ flag) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    flag[v] = len[v] > 0 && (prv[v] < 0 || ut_sampled(v));
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_links(const int32_t *__restrict__ nxt, const int32_t *__restrict__ noff, int32_t n, int2 *__restrict__ link) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    link[v] = make_int2(nxt[v], noff[v]);
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_ruler_list(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ ridx, const int32_t *__restrict__ prv,
                                                            int32_t n, int32_t *__restrict__ rnode, UtRank *__restrict__ rrec) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || !flag[v]) return;
    const uint32_t i = ridx[v];
    rnode[i] = v;
    if (prv[v] < 0) { UtRank r; r.up = (int32_t) i; r.rank = 0; r.pos = 0; r.done = 1; rrec[i] = r; }   // (every other ruler: by the walker before it)
}

// a node reached along next[] has a predecessor, so it is a ruler exactly when its id is sampled: no load decides it
__global__ void __launch_bounds__(UT_BLOCK) k_ut_ruler_walk1(const int2 *__restrict__ link, const int32_t *__restrict__ rnode, const uint32_t *__restrict__ ridx,
                                                             uint32_t R, UtRank *__restrict__ rrec) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    int32_t v = rnode[i], steps = 0, pos = 0;
    for (;;) {
        const int2 l = link[v];
        if (l.x < 0) return;
        steps++; pos = sat_add(pos, l.y); v = l.x;
        if (ut_sampled(v)) break;
    }
    UtRank r; r.up = (int32_t) i; r.rank = steps; r.pos = pos; r.done = 0;
    rrec[ridx[v]] = r;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_ruler_walk2(const int2 *__restrict__ link, const int32_t *__restrict__ rnode, const UtRank *__restrict__ rrec,
                                                             uint32_t R, UtRank *__restrict__ a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    const UtRank me = rrec[i];
    if (!me.done) return;                                             // a ruler on a cycle: its stretch keeps the initial records
    UtRank r; r.up = rnode[me.up]; r.rank = me.rank; r.pos = me.pos; r.done = 1;
    int32_t v = rnode[i];
    for (;;) {
        a[v] = r;
        const int2 l = link[v];
        if (l.x < 0 || ut_sampled(l.x)) return;
        v = l.x; r.rank++; r.pos = sat_add(r.pos, l.y);
    }
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_min_init(const UtRank *__restrict__ r, const int32_t *__restrict__ prv, int32_t n, UtMin *__restrict__ a) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || r[v].done) return;
    UtMin x; x.up = prv[v]; x.min_pair = v >> 1;
    a[v] = x;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_min_jump(const UtRank *__restrict__ r, const UtMin *__restrict__ a, UtMin *__restrict__ b, int32_t n) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || r[v].done) return;
    UtMin x = a[v];
    const UtMin u = a[x.up];                                          // a node of the same cycle: unresolved too, its record is set
    x.up = u.up; x.min_pair = u.min_pair < x.min_pair ? u.min_pair : x.min_pair;
    b[v] = x;
}

// m = 2 * (smallest pair) lies in the cycle or in its twin cycle: the one thread that IS m makes both cuts
__global__ void __launch_bounds__(UT_BLOCK) k_ut_cut(const UtRank *__restrict__ r, const UtMin *__restrict__ a, int32_t n, int32_t *__restrict__ nxt,
                                                     int32_t *__restrict__ prv, unsigned long long *__restrict__ counters) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || r[v].done || v != 2 * a[v].min_pair) return;
    const int32_t p = prv[v];
    prv[v] = -1; nxt[p] = -1;
    nxt[v ^ 1] = -1; prv[p ^ 1] = -1;
    atomicAdd(&counters[UT_CYCLES], 1ull);
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_tails(const UtRank *__restrict__ r, const int32_t *__restrict__ len, const int32_t *__restrict__ nxt, int32_t n,
                                                       int32_t *__restrict__ tail_of) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || len[v] <= 0 || nxt[v] >= 0) return;
    tail_of[r[v].up] = v;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_winners(const UtRank *__restrict__ r, const int32_t *__restrict__ len, const int32_t *__restrict__ prv,
                                                         const int32_t *__restrict__ tail_of, const uint32_t *__restrict__ rowptr, int32_t n, int skip_isolated,
                                                         uint32_t *__restrict__ win, unsigned long long *__restrict__ counters) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    unsigned long long skipped = 0;
    if (v < n) {
        uint32_t w = 0;
        if (len[v] > 0 && prv[v] < 0) {
            const int32_t t = tail_of[v];
            w = v < (t ^ 1);
            if (w && skip_isolated && t == v && rowptr[v + 1] == rowptr[v] && rowptr[(v ^ 1) + 1] == rowptr[v ^ 1]) { w = 0; skipped = 1; }
        }
        win[v] = w;
    }
    skipped = ut_wave_sum(skipped);
    if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(&counters[UT_ISOLATED], skipped);
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_pair_sizes(const UtRank *__restrict__ r, const int32_t *__restrict__ len, const int32_t *__restrict__ tail_of,
                                                            const uint32_t *__restrict__ win, const uint32_t *__restrict__ pair_of, int32_t n,
                                                            uint32_t *__restrict__ cnt, int32_t *__restrict__ ulen, int32_t *__restrict__ ulen2,
                                                            uint32_t *__restrict__ uwords,
                                                            unsigned long long *__restrict__ counters) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    unsigned long long nodes = 0, bases = 0, over = 0;
    if (v < n && win[v]) {
        const int32_t t = tail_of[v];
        const UtRank rt = r[t];
        int64_t L = (int64_t) rt.pos + len[t];
        if (rt.pos == 0x7FFFFFFF || L > 0x7FFFFFFFll) { over = 1; L = 0; }
        const uint32_t k = pair_of[v];
        nodes = (unsigned long long) rt.rank + 1; bases = (unsigned long long) L;
        cnt[k] = (uint32_t) nodes; ulen[k] = (int32_t) L; ulen2[2 * k] = (int32_t) L; ulen2[2 * k + 1] = (int32_t) L;   // (per oriented id: what the GFA kernels index)
        uwords[k] = (uint32_t) ((L + 15) >> 4);
    }
    const unsigned long long sn = ut_wave_sum(nodes), sb = ut_wave_sum(bases), mn = ut_wave_max(nodes), mb = ut_wave_max(bases);
    over = ut_wave_sum(over);
    if ((threadIdx.x & 63) == 0 && sn) {
        atomicAdd(&counters[UT_TOTAL_NODES], sn); atomicAdd(&counters[UT_TOTAL_BASES], sb);
        atomicMax(&counters[UT_LONGEST_NODES], mn); atomicMax(&counters[UT_LONGEST_BASES], mb);
        if (over) atomicAdd(&counters[UT_OVERFLOW], over);
    }
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_layout(const UtRank *__restrict__ r, const int32_t *__restrict__ len, const int32_t *__restrict__ tail_of,
                                                        const uint32_t *__restrict__ win, const uint32_t *__restrict__ pair_of,
                                                        const unsigned long long *__restrict__ path_off, int32_t n, int32_t *__restrict__ path_node,
                                                        int32_t *__restrict__ path_pos, int32_t *__restrict__ uid) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    int32_t id = -1;
    if (len[v] > 0) {
        const UtRank rv = r[v];
        const int32_t h = rv.up;
        if (win[h]) {
            const uint32_t k = pair_of[h];
            const unsigned long long at = path_off[k] + (unsigned long long) rv.rank;
            path_node[at] = v; path_pos[at] = rv.pos;
            id = (int32_t) (2 * k + 1);
        } else {
            const int32_t th = tail_of[h] ^ 1;                        // the head of the twin path
            if (win[th]) id = (int32_t) (2 * pair_of[th]);
        }
    }
    uid[v] = id;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_sequence(const uint32_t *__restrict__ words, int32_t stride, const int32_t *__restrict__ path_node,
                                                          const int32_t *__restrict__ path_pos, const unsigned long long *__restrict__ path_off,
                                                          const unsigned long long *__restrict__ word_off, const int32_t *__restrict__ ulen, uint32_t n_pairs,
                                                          uint64_t n_words, uint32_t *__restrict__ out) {
    for (uint64_t w = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_pairs;                               // the last pair k with word_off[k] <= w (no pair is empty)
        while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (word_off[mid] <= w) lo = mid; else hi = mid; }
        const uint32_t k = lo;
        const int32_t L = ulen[k];
        const int32_t j0 = (int32_t) ((w - word_off[k]) << 4), j1 = L - j0 < 16 ? L : j0 + 16;
        const unsigned long long p0 = path_off[k];
        const int32_t *pn = path_node + p0, *pp = path_pos + p0;
        const uint32_t cnt = (uint32_t) (path_off[k + 1] - p0);
        uint32_t a = 0, b = cnt;                                      // the last node i with pos[i] <= j0 (pos[0] = 0)
        while (b - a > 1) { const uint32_t mid = a + ((b - a) >> 1); if (pp[mid] <= j0) a = mid; else b = mid; }
        uint32_t i = a, acc = 0;
        int32_t j = j0;
        while (j < j1) {
            while (i + 1 < cnt && pp[i + 1] <= j) i++;
            const int32_t stop = i + 1 < cnt ? pp[i + 1] : L;
            const int32_t e = stop < j1 ? stop : j1;
            const int32_t q = j - pp[i], c = e - j;                   // bases q .. q + c of node i, 1 <= c <= 16
            const uint32_t *row = words + (uint64_t) pn[i] * (uint64_t) stride;
            const int32_t wq = q >> 4, sh = q & 15;
            uint64_t x = row[wq];
            if (((q + c - 1) >> 4) != wq) x |= (uint64_t) row[wq + 1] << 32;
            uint32_t codes = (uint32_t) (x >> (2 * sh));
            if (c < 16) codes &= (1u << (2 * c)) - 1u;
            acc |= codes << (2 * (j - j0));
            j = e;
        }
        out[w] = acc;
    }
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_edge_flags(const alga_edge_dev *__restrict__ estar, uint64_t ms, const int32_t *__restrict__ nxt,
                                                            uint32_t *__restrict__ flag) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ms) return;
    const alga_edge_dev x = estar[i];
    flag[i] = nxt[x.src] != x.dst;
}

__global__ void __launch_bounds__(UT_BLOCK) k_ut_edges(const alga_edge_dev *__restrict__ estar, uint64_t ms, const uint32_t *__restrict__ flag,
                                                       const uint32_t *__restrict__ pos, const int32_t *__restrict__ uid, const UtRank *__restrict__ r,
                                                       unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ms || !flag[i]) return;
    const alga_edge_dev x = estar[i];
    // x.src is the last node of its oriented unitig, x.dst the first of its own: the offset counts from the source unitig's start
    keys[pos[i]] = ((unsigned long long) (uint32_t) uid[x.src] << 32) | (uint32_t) uid[x.dst];
    vals[pos[i]] = (uint32_t) (r[x.src].pos + x.offset);
}

inline unsigned ut_grid(uint64_t items) { return (unsigned) ((items + UT_BLOCK - 1) / UT_BLOCK); }

}  // namespace

void launch_ut_check(const int32_t *len, int32_t n, const alga_edge_dev *e, uint64_t m, unsigned long long *counters, hipStream_t s) {
    const uint64_t items = m > (uint64_t) n ? m : (uint64_t) n;
    if (!items) return;
    hipLaunchKernelGGL(k_ut_check, dim3(std::min<unsigned>(ut_grid(items), 65536u)), dim3(UT_BLOCK), 0, s, len, n, e, m, counters);
}
void launch_ut_twins(const int32_t *len, const alga_edge_dev *e, uint64_t m, unsigned long long *keys, uint32_t *vals, hipStream_t s) {
    if (!m) return;
    hipLaunchKernelGGL(k_ut_twins, dim3(std::min<unsigned>(ut_grid(m), 65536u)), dim3(UT_BLOCK), 0, s, len, e, m, keys, vals);
}
void launch_ut_group_heads(const unsigned long long *keys, const uint32_t *vals, uint64_t m2, uint32_t *flag, uint32_t *best, unsigned long long *counters,
                           hipStream_t s) {
    if (!m2) return;
    hipLaunchKernelGGL(k_ut_group_heads, dim3(ut_grid(m2)), dim3(UT_BLOCK), 0, s, keys, vals, m2, flag, best, counters);
}
void launch_ut_compact_edges(const unsigned long long *keys, const uint32_t *flag, const uint32_t *pos, const uint32_t *best, uint64_t m2,
                             alga_edge_dev *estar, hipStream_t s) {
    if (!m2) return;
    hipLaunchKernelGGL(k_ut_compact_edges, dim3(ut_grid(m2)), dim3(UT_BLOCK), 0, s, keys, flag, pos, best, m2, estar);
}
void launch_ut_next(const alga_edge_dev *estar, const uint32_t *rowptr, int32_t n, int32_t *nxt, int32_t *noff, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_next, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, estar, rowptr, n, nxt, noff);
}
void launch_ut_prev(const int32_t *nxt, int32_t n, int32_t *prv, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_prev, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, nxt, n, prv);
}
void launch_ut_rank_init(const int32_t *len, const int32_t *prv, const int32_t *noff, int32_t n, int only_unresolved, UtRank *a, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_rank_init, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, len, prv, noff, n, only_unresolved, a);
}
void launch_ut_rank_jump(const UtRank *a, UtRank *b, int32_t n, unsigned long long *unresolved, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_rank_jump, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, a, b, n, unresolved);
}
void launch_ut_ruler_flags(const int32_t *len, const int32_t *prv, int32_t n, uint32_t *flag, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_ruler_flags, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, len, prv, n, flag);
}
void launch_ut_links(const int32_t *nxt, const int32_t *noff, int32_t n, int2 *link, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_links, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, nxt, noff, n, link);
}
void launch_ut_ruler_list(const uint32_t *flag, const uint32_t *ridx, const int32_t *prv, int32_t n, int32_t *rnode, UtRank *rrec, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_ruler_list, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, flag, ridx, prv, n, rnode, rrec);
}
void launch_ut_ruler_walk1(const int2 *link, const int32_t *rnode, const uint32_t *ridx, uint32_t R, UtRank *rrec, hipStream_t s) {
    if (!R) return;
    hipLaunchKernelGGL(k_ut_ruler_walk1, dim3(ut_grid(R)), dim3(UT_BLOCK), 0, s, link, rnode, ridx, R, rrec);
}
void launch_ut_ruler_walk2(const int2 *link, const int32_t *rnode, const UtRank *rrec, uint32_t R, UtRank *a, hipStream_t s) {
    if (!R) return;
    hipLaunchKernelGGL(k_ut_ruler_walk2, dim3(ut_grid(R)), dim3(UT_BLOCK), 0, s, link, rnode, rrec, R, a);
}
void launch_ut_min_init(const UtRank *r, const int32_t *prv, int32_t n, UtMin *a, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_min_init, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, prv, n, a);
}
void launch_ut_min_jump(const UtRank *r, const UtMin *a, UtMin *b, int32_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_min_jump, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, a, b, n);
}
void launch_ut_cut(const UtRank *r, const UtMin *a, int32_t n, int32_t *nxt, int32_t *prv, unsigned long long *counters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_cut, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, a, n, nxt, prv, counters);
}
void launch_ut_tails(const UtRank *r, const int32_t *len, const int32_t *nxt, int32_t n, int32_t *tail_of, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_tails, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, len, nxt, n, tail_of);
}
void launch_ut_winners(const UtRank *r, const int32_t *len, const int32_t *prv, const int32_t *tail_of, const uint32_t *rowptr, int32_t n, int skip_isolated,
                       uint32_t *win, unsigned long long *counters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_winners, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, len, prv, tail_of, rowptr, n, skip_isolated, win, counters);
}
void launch_ut_pair_sizes(const UtRank *r, const int32_t *len, const int32_t *tail_of, const uint32_t *win, const uint32_t *pair_of, int32_t n,
                          uint32_t *cnt, int32_t *ulen, int32_t *ulen2, uint32_t *uwords, unsigned long long *counters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_pair_sizes, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, len, tail_of, win, pair_of, n, cnt, ulen, ulen2, uwords, counters);
}
void launch_ut_layout(const UtRank *r, const int32_t *len, const int32_t *tail_of, const uint32_t *win, const uint32_t *pair_of,
                      const unsigned long long *path_off, int32_t n, int32_t *path_node, int32_t *path_pos, int32_t *uid, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ut_layout, dim3(ut_grid((uint64_t) n)), dim3(UT_BLOCK), 0, s, r, len, tail_of, win, pair_of, path_off, n, path_node, path_pos, uid);
}
void launch_ut_sequence(const uint32_t *words, int32_t stride, const int32_t *path_node, const int32_t *path_pos,
                        const unsigned long long *path_off, const unsigned long long *word_off, const int32_t *ulen, uint32_t n_pairs, uint64_t n_words,
                        uint32_t *out, hipStream_t s) {
    if (!n_words || !n_pairs) return;
    hipLaunchKernelGGL(k_ut_sequence, dim3(std::min<unsigned>(ut_grid(n_words), 1u << 20)), dim3(UT_BLOCK), 0, s, words, stride, path_node, path_pos, path_off,
                       word_off, ulen, n_pairs, n_words, out);
}
void launch_ut_edge_flags(const alga_edge_dev *estar, uint64_t ms, const int32_t *nxt, uint32_t *flag, hipStream_t s) {
    if (!ms) return;
    hipLaunchKernelGGL(k_ut_edge_flags, dim3(ut_grid(ms)), dim3(UT_BLOCK), 0, s, estar, ms, nxt, flag);
}
void launch_ut_edges(const alga_edge_dev *estar, uint64_t ms, const uint32_t *flag, const uint32_t *pos, const int32_t *uid, const UtRank *r,
                     unsigned long long *keys, uint32_t *vals, hipStream_t s) {
    if (!ms) return;
    hipLaunchKernelGGL(k_ut_edges, dim3(ut_grid(ms)), dim3(UT_BLOCK), 0, s, estar, ms, flag, pos, uid, r, keys, vals);
}

}  // namespace alga
