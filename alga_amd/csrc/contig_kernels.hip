// alga_amd/csrc/contig_kernels.hip -- contigs of an overlap graph: contract, cut the contracted graph, contract again
// (include/alga_amd.h: alga_contigs_device; host side: engine_contig.hip).
//
// Integer work only, one thread per node / edge / chain / group.  B is the base graph of a round: E* at first, sorted by (src, dst), one edge per
// (src, dst), twin-symmetric; every round leaves a subset in the same order.  A round:
//   k_ct_pflags / k_ct_next   P (in = out = 1, neither neighbour the node or its twin), next[] between two P nodes
//   (the unitig ranking)      every P node gets (head of its run of P nodes, steps, bases); k_ct_open_cycles takes m and m^1 of a cycle out of P
//   k_ct_run_info             per run: its last node, its smallest read index (one atomicMin per P node)
//   k_ct_chains               one thread per edge out of a node outside P: that edge, the run it enters, the edge that leaves the run -> (c, w, nodes, key)
//   k_ct_open_keys -> sort    the open chains by (a, c)
//   k_ct_groups               one thread per group head walks its group: the smallest (w, key), the parallel drops; H = one edge per group
//   (k_cut_triangles on H)    the triangle cut's own kernel
//   k_ct_cut_back             one thread per group head: its H edge and its twin's among the survivors of their rows?
//   k_ct_edge_keep/_compact   an edge of B goes with its chain or its twin's chain
// After the last round: k_ct_winners, k_ct_pair_sizes, k_ct_layout_*, (k_ut_sequence), k_ct_join_*.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "contig_kernels.h"

namespace alga {

namespace {

constexpr int CT_BLOCK = 256;

__device__ __forceinline__ unsigned long long ct_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long ct_wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// index of the edge a -> b in B (rows sorted by dst; the edge exists: B is twin-symmetric)
__device__ __forceinline__ uint32_t ct_find(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ rowptr, int32_t a, int32_t b) {
    uint32_t lo = rowptr[a], hi = rowptr[a + 1];
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (B[mid].dst < b) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_pflags(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ rowptr, int32_t n,
                                                        uint32_t *__restrict__ pflag) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    const int32_t t = v ^ 1;
    const uint32_t r0 = rowptr[v], q0 = rowptr[t];
    uint32_t p = 0;
    if (rowptr[v + 1] - r0 == 1 && rowptr[t + 1] - q0 == 1) {         // indeg(v) == outdeg(v^1), pred(v) == succ(v^1)^1
        const int32_t s1 = B[r0].dst, s2 = B[q0].dst;
        p = s1 != v && s1 != t && s2 != v && s2 != t;
    }
    pflag[v] = p;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_next(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ pflag,
                                                      int32_t n, int32_t *__restrict__ nxt, int32_t *__restrict__ noff) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n) return;
    int32_t to = -1, off = 0;
    if (pflag[v]) {
        const alga_edge_dev x = B[rowptr[v]];
        if (pflag[x.dst]) { to = x.dst; off = x.offset; }
    }
    nxt[v] = to; noff[v] = off;
}

// the one thread that IS m = 2 * (smallest pair) -- in its cycle or in the twin cycle -- takes m and m^1 out of P and removes their four links
__global__ void __launch_bounds__(CT_BLOCK) k_ct_open_cycles(const UtRank *__restrict__ r, const UtMin *__restrict__ a, int32_t n, int32_t *__restrict__ nxt,
                                                             int32_t *__restrict__ prv, uint32_t *__restrict__ pflag,
                                                             unsigned long long *__restrict__ ut_counters) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || r[v].done || v != 2 * a[v].min_pair) return;
    for (int k = 0; k < 2; k++) {
        const int32_t u = v ^ k;
        const int32_t p = prv[u], q = nxt[u];
        if (p >= 0) nxt[p] = -1;
        if (q >= 0) prv[q] = -1;
        nxt[u] = -1; prv[u] = -1; pflag[u] = 0;
    }
    atomicAdd(&ut_counters[UT_CYCLES], 1ull);
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_run_info(const UtRank *__restrict__ r, const uint32_t *__restrict__ pflag, const int32_t *__restrict__ nxt,
                                                          const uint32_t *__restrict__ rowptr, int32_t n, int32_t *__restrict__ tail_of,
                                                          uint32_t *__restrict__ runkey, unsigned long long *__restrict__ counters) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    unsigned long long pn = 0, touched = 0;
    if (v < n) {
        touched = rowptr[v + 1] > rowptr[v] || rowptr[(v ^ 1) + 1] > rowptr[v ^ 1];
        if (pflag[v]) {
            pn = 1;
            const int32_t h = r[v].up;
            atomicMin(&runkey[h], (uint32_t) v >> 1);
            if (nxt[v] < 0) tail_of[h] = v;
        }
    }
    pn = ct_wave_sum(pn); touched = ct_wave_sum(touched);
    if ((threadIdx.x & 63) == 0) {
        if (pn) atomicAdd(&counters[CT_PATH_NODES], pn);
        if (touched) atomicAdd(&counters[CT_TOUCHED], touched);
    }
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_chains(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ rowptr, uint64_t mb,
                                                        const uint32_t *__restrict__ pflag, const UtRank *__restrict__ r, const int32_t *__restrict__ tail_of,
                                                        const uint32_t *__restrict__ runkey, CtChain *__restrict__ chain, uint32_t *__restrict__ headchain,
                                                        uint32_t *__restrict__ openflag, unsigned long long *__restrict__ counters) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long chains = 0, closed = 0, over = 0;
    if (i < mb) {
        const alga_edge_dev x = B[i];
        uint32_t open = 0;
        if (!pflag[x.src]) {
            CtChain c;
            int64_t w = x.offset;
            if (!pflag[x.dst]) { c.end = x.dst; c.nodes = 2; c.x = x.src; c.key = CT_NO_KEY; }
            else {
                const int32_t t = tail_of[x.dst];
                const UtRank rt = r[t];
                const alga_edge_dev y = B[rowptr[t]];                 // the one edge out of the run's last node
                w += (int64_t) rt.pos + y.offset;
                c.end = y.dst; c.nodes = rt.rank + 3; c.x = t; c.key = runkey[x.dst];
                headchain[x.dst] = (uint32_t) i;
            }
            if (w > 0x7FFFFFFFll) { over = 1; w = 0x7FFFFFFFll; }
            c.w = (int32_t) w;
            c.tw = (int32_t) ct_find(B, rowptr, c.end ^ 1, c.x ^ 1);
            c.pad0 = 0; c.pad1 = 0;
            chain[i] = c;
            chains = 1;
            open = c.end != x.src && c.end != (x.src ^ 1);
            closed = !open;
        }
        openflag[i] = open;
    }
    chains = ct_wave_sum(chains); closed = ct_wave_sum(closed); over = ct_wave_sum(over);
    if ((threadIdx.x & 63) == 0 && chains) {
        atomicAdd(&counters[CT_CHAINS], chains);
        if (closed) atomicAdd(&counters[CT_CLOSED], closed);
        if (over) atomicAdd(&counters[CT_OVERFLOW], over);
    }
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_open_keys(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ openflag,
                                                           const uint32_t *__restrict__ opos, const CtChain *__restrict__ chain, uint64_t mb,
                                                           unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mb || !openflag[i]) return;
    const uint32_t at = opos[i];
    keys[at] = ((unsigned long long) (uint32_t) B[i].src << 32) | (uint32_t) chain[i].end;
    vals[at] = (uint32_t) i;
}

__device__ __forceinline__ bool ct_less(uint32_t w1, uint32_t k1, uint32_t w2, uint32_t k2) { return w1 < w2 || (w1 == w2 && k1 < k2); }

__global__ void __launch_bounds__(CT_BLOCK) k_ct_groups(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t no,
                                                        const CtChain *__restrict__ chain, int32_t max_offset, uint32_t *__restrict__ hflag,
                                                        uint32_t *__restrict__ hw, uint32_t *__restrict__ hk, uint8_t *__restrict__ drop,
                                                        unsigned long long *__restrict__ counters) {
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long dropped = 0;
    if (j < no) {
        const unsigned long long k = keys[j];
        const bool head = j == 0 || keys[j - 1] != k;
        hflag[j] = head ? 1u : 0u;
        if (head) {
            const CtChain c0 = chain[vals[j]];
            uint32_t bw = (uint32_t) c0.w, bk = c0.key;
            uint64_t end = j + 1;
            for (; end < no && keys[end] == k; end++) {
                const CtChain c = chain[vals[end]];
                if (ct_less((uint32_t) c.w, c.key, bw, bk)) { bw = (uint32_t) c.w; bk = c.key; }
            }
            hw[j] = bw; hk[j] = bk;
            if (end - j > 1)
                for (uint64_t q = j; q < end; q++) {
                    const uint32_t id = vals[q];
                    const CtChain c = chain[id];
                    if (((uint32_t) c.w != bw || c.key != bk) && c.w <= max_offset) { drop[id] = 1; dropped++; }
                }
        }
    }
    dropped = ct_wave_sum(dropped);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&counters[CT_PARALLEL], dropped);
}

__device__ __forceinline__ bool ct_survives(const uint32_t *__restrict__ hrow, const alga_edge_dev *__restrict__ hlist, const uint32_t *__restrict__ hcnt,
                                            int32_t a, int32_t c) {
    const uint32_t r0 = hrow[a], cnt = hcnt[a];
    for (uint32_t k = 0; k < cnt; k++) if (hlist[r0 + k].dst == c) return true;
    return false;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_cut_back(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t no,
                                                          const uint32_t *__restrict__ hflag, const uint32_t *__restrict__ hw, const uint32_t *__restrict__ hk,
                                                          const CtChain *__restrict__ chain, const uint32_t *__restrict__ hrow,
                                                          const alga_edge_dev *__restrict__ hlist, const uint32_t *__restrict__ hcnt,
                                                          uint8_t *__restrict__ drop, unsigned long long *__restrict__ counters) {
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cut = 0;
    if (j < no && hflag[j]) {
        const unsigned long long k = keys[j];
        const int32_t a = (int32_t) (k >> 32), c = (int32_t) (uint32_t) k;
        const bool mine = ct_survives(hrow, hlist, hcnt, a, c);
        cut = !mine;
        if (!mine || !ct_survives(hrow, hlist, hcnt, c ^ 1, a ^ 1)) {
            const uint32_t bw = hw[j], bk = hk[j];
            for (uint64_t q = j; q < no && keys[q] == k; q++) {
                const uint32_t id = vals[q];
                const CtChain x = chain[id];
                if ((uint32_t) x.w == bw && x.key == bk) drop[id] = 1;
            }
        }
    }
    cut = ct_wave_sum(cut);
    if ((threadIdx.x & 63) == 0 && cut) atomicAdd(&counters[CT_GROUPS_CUT], cut);
}

// the chain of edge u -> v: the edge itself when u is outside P, else the chain that enters u's run
__device__ __forceinline__ uint32_t ct_chain_of(uint32_t i, int32_t u, const uint32_t *__restrict__ pflag, const UtRank *__restrict__ r,
                                                const uint32_t *__restrict__ headchain) {
    return pflag[u] ? headchain[r[u].up] : i;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_edge_keep(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ rowptr, uint64_t mb,
                                                           const uint32_t *__restrict__ pflag, const UtRank *__restrict__ r,
                                                           const uint32_t *__restrict__ headchain, const uint8_t *__restrict__ drop,
                                                           uint32_t *__restrict__ keep) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mb) return;
    const alga_edge_dev x = B[i];
    const uint32_t ti = ct_find(B, rowptr, x.dst ^ 1, x.src ^ 1);
    const uint32_t c1 = ct_chain_of((uint32_t) i, x.src, pflag, r, headchain), c2 = ct_chain_of(ti, x.dst ^ 1, pflag, r, headchain);
    keep[i] = !(drop[c1] | drop[c2]);
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_compact(const alga_edge_dev *__restrict__ B, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kpos,
                                                         uint64_t mb, alga_edge_dev *__restrict__ out) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mb || !keep[i]) return;
    out[kpos[i]] = B[i];
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_winners(const alga_edge_dev *__restrict__ B, uint64_t mb, const uint32_t *__restrict__ pflag,
                                                         const CtChain *__restrict__ chain, uint32_t *__restrict__ win) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mb) return;
    const alga_edge_dev x = B[i];
    uint32_t w = 0;
    if (!pflag[x.src]) {
        const CtChain c = chain[i];
        const int32_t ta = c.end ^ 1, tb = c.x ^ 1;                   // first and second node of the twin chain
        w = x.src < ta || (x.src == ta && x.dst <= tb);
    }
    win[i] = w;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_pair_sizes(const alga_edge_dev *__restrict__ B, const CtChain *__restrict__ chain, const int32_t *__restrict__ len,
                                                            const uint32_t *__restrict__ win, const uint32_t *__restrict__ pair_of, uint64_t mb,
                                                            uint32_t *__restrict__ pcnt, int32_t *__restrict__ ulen, int32_t *__restrict__ ulen2,
                                                            uint32_t *__restrict__ uwords, uint32_t *__restrict__ oid, uint32_t *__restrict__ cid,
                                                            unsigned long long *__restrict__ counters) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long nodes = 0, bases = 0, over = 0;
    if (i < mb && win[i]) {
        const CtChain c = chain[i];
        int64_t L = (int64_t) c.w + len[c.end];
        if (c.w == 0x7FFFFFFF || L > 0x7FFFFFFFll) { over = 1; L = 0; }
        const uint32_t k = pair_of[i];
        nodes = (unsigned long long) c.nodes; bases = (unsigned long long) L;
        pcnt[k] = (uint32_t) c.nodes; ulen[k] = (int32_t) L; ulen2[2 * k] = (int32_t) L; ulen2[2 * k + 1] = (int32_t) L;
        uwords[k] = (uint32_t) ((L + 15) >> 4);
        oid[i] = 2 * k + 1; cid[2 * k + 1] = (uint32_t) i; cid[2 * k] = (uint32_t) c.tw;
        if ((uint64_t) c.tw != i) oid[c.tw] = 2 * k;                  // (a self-twin chain: both oriented ids are this chain)
    }
    const unsigned long long sn = ct_wave_sum(nodes), sb = ct_wave_sum(bases), mn = ct_wave_max(nodes), mx = ct_wave_max(bases);
    over = ct_wave_sum(over);
    if ((threadIdx.x & 63) == 0 && sn) {
        atomicAdd(&counters[CT_TOTAL_BASES], sb);
        atomicMax(&counters[CT_LONGEST_NODES], mn); atomicMax(&counters[CT_LONGEST_BASES], mx);
        if (over) atomicAdd(&counters[CT_OVERFLOW], over);
    }
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_layout_ends(const alga_edge_dev *__restrict__ B, uint64_t mb, const CtChain *__restrict__ chain,
                                                             const uint32_t *__restrict__ win, const uint32_t *__restrict__ pair_of,
                                                             const unsigned long long *__restrict__ path_off, int32_t *__restrict__ path_node,
                                                             int32_t *__restrict__ path_pos) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mb || !win[i]) return;
    const CtChain c = chain[i];
    const unsigned long long p0 = path_off[pair_of[i]], p1 = p0 + (unsigned long long) c.nodes - 1;
    path_node[p0] = B[i].src; path_pos[p0] = 0;
    path_node[p1] = c.end; path_pos[p1] = c.w;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_layout_inner(const alga_edge_dev *__restrict__ B, int32_t n, const uint32_t *__restrict__ pflag,
                                                              const UtRank *__restrict__ r, const uint32_t *__restrict__ headchain,
                                                              const uint32_t *__restrict__ win, const uint32_t *__restrict__ pair_of,
                                                              const unsigned long long *__restrict__ path_off, int32_t *__restrict__ path_node,
                                                              int32_t *__restrict__ path_pos) {
    const int32_t v = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= n || !pflag[v]) return;
    const UtRank rv = r[v];
    const uint32_t ch = headchain[rv.up];
    if (!win[ch]) return;                                             // (the twin node writes the `+` orientation)
    const unsigned long long at = path_off[pair_of[ch]] + 1ull + (unsigned long long) rv.rank;
    path_node[at] = v; path_pos[at] = B[ch].offset + rv.pos;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_join_count(const uint32_t *__restrict__ cid, const CtChain *__restrict__ chain, const uint32_t *__restrict__ rowptr,
                                                            uint64_t n_oriented, uint32_t *__restrict__ deg) {
    const uint64_t X = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= n_oriented) return;
    const int32_t c = chain[cid[X]].end;
    uint32_t d = 0;
    for (uint32_t j = rowptr[c]; j < rowptr[c + 1]; j++) d += 1u + ((uint32_t) chain[j].tw == j);
    deg[X] = d;
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_join_fill(const uint32_t *__restrict__ cid, const CtChain *__restrict__ chain, const uint32_t *__restrict__ rowptr,
                                                           const uint32_t *__restrict__ oid, const uint32_t *__restrict__ epos, uint64_t n_oriented,
                                                           unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t X = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= n_oriented) return;
    const CtChain me = chain[cid[X]];
    uint32_t at = epos[X];
    for (uint32_t j = rowptr[me.end]; j < rowptr[me.end + 1]; j++) {
        const uint32_t Y = oid[j];
        keys[at] = ((unsigned long long) X << 32) | Y; vals[at] = (uint32_t) me.w; at++;
        if ((uint32_t) chain[j].tw == j) { keys[at] = ((unsigned long long) X << 32) | (Y ^ 1u); vals[at] = (uint32_t) me.w; at++; }
    }
}

__global__ void __launch_bounds__(CT_BLOCK) k_ct_fasta_select(const int32_t *__restrict__ len, uint64_t n_pairs, int32_t min_length, uint32_t *__restrict__ sel) {
    const uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pairs) return;
    const int32_t L = len[k];
    sel[k] = L > 0 && L >= min_length;
}

inline unsigned ct_grid(uint64_t items) { return (unsigned) ((items + CT_BLOCK - 1) / CT_BLOCK); }

}  // namespace

void launch_ct_pflags(const alga_edge_dev *B, const uint32_t *rowptr, int32_t n, uint32_t *pflag, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ct_pflags, dim3(ct_grid((uint64_t) n)), dim3(CT_BLOCK), 0, s, B, rowptr, n, pflag);
}
void launch_ct_next(const alga_edge_dev *B, const uint32_t *rowptr, const uint32_t *pflag, int32_t n, int32_t *nxt, int32_t *noff, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ct_next, dim3(ct_grid((uint64_t) n)), dim3(CT_BLOCK), 0, s, B, rowptr, pflag, n, nxt, noff);
}
void launch_ct_open_cycles(const UtRank *r, const UtMin *a, int32_t n, int32_t *nxt, int32_t *prv, uint32_t *pflag, unsigned long long *ut_counters,
                           hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ct_open_cycles, dim3(ct_grid((uint64_t) n)), dim3(CT_BLOCK), 0, s, r, a, n, nxt, prv, pflag, ut_counters);
}
void launch_ct_run_info(const UtRank *r, const uint32_t *pflag, const int32_t *nxt, const uint32_t *rowptr, int32_t n, int32_t *tail_of, uint32_t *runkey,
                        unsigned long long *counters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ct_run_info, dim3(ct_grid((uint64_t) n)), dim3(CT_BLOCK), 0, s, r, pflag, nxt, rowptr, n, tail_of, runkey, counters);
}
void launch_ct_chains(const alga_edge_dev *B, const uint32_t *rowptr, uint64_t mb, const uint32_t *pflag, const UtRank *r, const int32_t *tail_of,
                      const uint32_t *runkey, CtChain *chain, uint32_t *headchain, uint32_t *openflag, unsigned long long *counters, hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_chains, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, rowptr, mb, pflag, r, tail_of, runkey, chain, headchain, openflag, counters);
}
void launch_ct_open_keys(const alga_edge_dev *B, const uint32_t *openflag, const uint32_t *opos, const CtChain *chain, uint64_t mb,
                         unsigned long long *keys, uint32_t *vals, hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_open_keys, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, openflag, opos, chain, mb, keys, vals);
}
void launch_ct_groups(const unsigned long long *keys, const uint32_t *vals, uint64_t no, const CtChain *chain, int32_t max_offset, uint32_t *hflag,
                      uint32_t *hw, uint32_t *hk, uint8_t *drop, unsigned long long *counters, hipStream_t s) {
    if (!no) return;
    hipLaunchKernelGGL(k_ct_groups, dim3(ct_grid(no)), dim3(CT_BLOCK), 0, s, keys, vals, no, chain, max_offset, hflag, hw, hk, drop, counters);
}
void launch_ct_cut_back(const unsigned long long *keys, const uint32_t *vals, uint64_t no, const uint32_t *hflag, const uint32_t *hw, const uint32_t *hk,
                        const CtChain *chain, const uint32_t *hrow, const alga_edge_dev *hlist, const uint32_t *hcnt, uint8_t *drop,
                        unsigned long long *counters, hipStream_t s) {
    if (!no) return;
    hipLaunchKernelGGL(k_ct_cut_back, dim3(ct_grid(no)), dim3(CT_BLOCK), 0, s, keys, vals, no, hflag, hw, hk, chain, hrow, hlist, hcnt, drop, counters);
}
void launch_ct_edge_keep(const alga_edge_dev *B, const uint32_t *rowptr, uint64_t mb, const uint32_t *pflag, const UtRank *r, const uint32_t *headchain,
                         const uint8_t *drop, uint32_t *keep, hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_edge_keep, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, rowptr, mb, pflag, r, headchain, drop, keep);
}
void launch_ct_compact(const alga_edge_dev *B, const uint32_t *keep, const uint32_t *kpos, uint64_t mb, alga_edge_dev *out, hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_compact, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, keep, kpos, mb, out);
}
void launch_ct_winners(const alga_edge_dev *B, uint64_t mb, const uint32_t *pflag, const CtChain *chain, uint32_t *win, hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_winners, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, mb, pflag, chain, win);
}
void launch_ct_pair_sizes(const alga_edge_dev *B, const CtChain *chain, const int32_t *len, const uint32_t *win, const uint32_t *pair_of, uint64_t mb,
                          uint32_t *pcnt, int32_t *ulen, int32_t *ulen2, uint32_t *uwords, uint32_t *oid, uint32_t *cid, unsigned long long *counters,
                          hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_pair_sizes, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, chain, len, win, pair_of, mb, pcnt, ulen, ulen2, uwords, oid, cid, counters);
}
void launch_ct_layout_ends(const alga_edge_dev *B, uint64_t mb, const CtChain *chain, const uint32_t *win, const uint32_t *pair_of,
                           const unsigned long long *path_off, int32_t *path_node, int32_t *path_pos, hipStream_t s) {
    if (!mb) return;
    hipLaunchKernelGGL(k_ct_layout_ends, dim3(ct_grid(mb)), dim3(CT_BLOCK), 0, s, B, mb, chain, win, pair_of, path_off, path_node, path_pos);
}
void launch_ct_layout_inner(const alga_edge_dev *B, int32_t n, const uint32_t *pflag, const UtRank *r, const uint32_t *headchain, const uint32_t *win,
                            const uint32_t *pair_of, const unsigned long long *path_off, int32_t *path_node, int32_t *path_pos, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ct_layout_inner, dim3(ct_grid((uint64_t) n)), dim3(CT_BLOCK), 0, s, B, n, pflag, r, headchain, win, pair_of, path_off, path_node, path_pos);
}
void launch_ct_join_count(const uint32_t *cid, const CtChain *chain, const uint32_t *rowptr, uint64_t n_oriented, uint32_t *deg, hipStream_t s) {
    if (!n_oriented) return;
    hipLaunchKernelGGL(k_ct_join_count, dim3(ct_grid(n_oriented)), dim3(CT_BLOCK), 0, s, cid, chain, rowptr, n_oriented, deg);
}
void launch_ct_join_fill(const uint32_t *cid, const CtChain *chain, const uint32_t *rowptr, const uint32_t *oid, const uint32_t *epos, uint64_t n_oriented,
                         unsigned long long *keys, uint32_t *vals, hipStream_t s) {
    if (!n_oriented) return;
    hipLaunchKernelGGL(k_ct_join_fill, dim3(ct_grid(n_oriented)), dim3(CT_BLOCK), 0, s, cid, chain, rowptr, oid, epos, n_oriented, keys, vals);
}
void launch_ct_fasta_select(const int32_t *len, uint64_t n_pairs, int32_t min_length, uint32_t *sel, hipStream_t s) {
    if (!n_pairs) return;
    hipLaunchKernelGGL(k_ct_fasta_select, dim3(ct_grid(n_pairs)), dim3(CT_BLOCK), 0, s, len, n_pairs, min_length, sel);
}

}  // namespace alga
