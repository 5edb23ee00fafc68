// alga_amd/csrc/tip_kernels.hip -- dangling-branch removal on the overlap graph (include/alga_amd.h: alga_remove_dangling_branches_device).
//
// Integer work only.  The graph is built once (host side: engine_simplify.hip): the edges reduced to one per (src, dst) and sorted (the
// engine's edge sort, k_ut_group_heads / k_ut_compact_edges of the unitig path), the forward CSR over them, the reverse CSR by one more sort
// with the forward id of every slot, one `alive` byte per edge.  A pass never rebuilds it:
//   k_tip_degrees        per node and direction: live degree and the first live edge (one 16-byte record: the walk gathers one per step),
//                        and the list of the nodes that branch in the direction of the pass
//   k_tip_find           one thread per branching node walks its chains (tip_walk.h: tip_walk_junction, its short list in LDS, one column per
//                        lane) and sets kill[] of the edges on the branches that go: idempotent byte stores, no removal list, no sort
//   k_tip_find_overflow  the nodes whose list did not fit (rows of hundreds of edges, neighbourhoods full of joins): the literal walk with
//                        per-node arrays in a workspace, one thread per workspace, the nodes of the overflow list dealt out over them
//   k_tip_apply          alive &= ~kill and the count of the pass -- every walk of a pass has read the same unmodified graph
// The up pass is the same kernels with the two directions exchanged.  At the end k_tip_flags -> scan -> k_tip_emit compact the survivors.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "tip_kernels.h"

namespace alga {

namespace {

constexpr int TIP_BLOCK = 256;
constexpr int TIP_WALK_BLOCK = 64;                                  // one wave: 8 KB of LDS per block, 20 blocks per CU
constexpr int TIP_WORDS = 3 * TIP_LIST + 2 * TIP_ENDS;

__device__ __forceinline__ unsigned long long tip_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_check(const alga_edge_dev *__restrict__ e, uint64_t m, int32_t n, unsigned long long *__restrict__ counters) {
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t) gridDim.x * blockDim.x) {
        const alga_edge_dev x = e[i];
        if (x.src < 0 || x.src >= n || x.dst < 0 || x.dst >= n) bad |= TIP_BAD_ID;
        if (x.offset < 0) bad |= TIP_BAD_OFFSET;
    }
    if (bad) atomicOr(&counters[TIP_FLAGS], bad);
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_keys(const alga_edge_dev *__restrict__ e, uint64_t m, unsigned long long *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t) gridDim.x * blockDim.x) {
        const alga_edge_dev x = e[i];
        keys[i] = ((unsigned long long) (uint32_t) x.src << 32) | (uint32_t) x.dst;
        vals[i] = (uint32_t) x.offset << 1;
    }
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_rev_keys(const alga_edge_dev *__restrict__ est, uint64_t ms, unsigned long long *__restrict__ keys,
                                                            uint32_t *__restrict__ vals) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < ms; i += (uint64_t) gridDim.x * blockDim.x) {
        const alga_edge_dev x = est[i];
        keys[i] = ((unsigned long long) (uint32_t) x.dst << 32) | (uint32_t) x.src;
        vals[i] = (uint32_t) i;
    }
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_rev_edges(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                             const alga_edge_dev *__restrict__ est, uint64_t ms, alga_edge_dev *__restrict__ rev,
                                                             uint32_t *__restrict__ rfid) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < ms; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t f = vals[i];
        alga_edge_dev x;
        x.src = (int32_t) (keys[i] >> 32); x.dst = (int32_t) (uint32_t) keys[i]; x.offset = est[f].offset;
        rev[i] = x;
        rfid[i] = f;
    }
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_degrees(TipDir fwd, TipDir rev, const uint8_t *__restrict__ alive, int32_t n, int dir,
                                                           TipRec *__restrict__ frec, TipRec *__restrict__ rrec, int32_t *__restrict__ branch,
                                                           unsigned long long *__restrict__ counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2u * (uint32_t) n) return;
    const int k = i >= (uint32_t) n;
    const int32_t v = (int32_t) (k ? i - (uint32_t) n : i);
    const TipDir g = k ? rev : fwd;
    TipRec r{0, -1, 0, 0};
    for (uint32_t s = g.rowptr[v], end = g.rowptr[v + 1]; s < end; s++) {
        const uint32_t f = g.fid ? g.fid[s] : s;
        if (!alive[f]) continue;
        if (r.deg == 0) { const alga_edge_dev x = g.E[s]; r.nbr = x.dst; r.off = x.offset; r.fid = f; }
        r.deg++;
    }
    (k ? rrec : frec)[v] = r;
    if (k == dir && r.deg >= 2) branch[atomicAdd(&counters[TIP_N_BRANCH], 1ull)] = v;
}

__global__ void __launch_bounds__(TIP_WALK_BLOCK) k_tip_find(TipGraph g, const int32_t *__restrict__ branch, int32_t max_offset, uint8_t *kill,
                                                             int32_t *__restrict__ overflow, unsigned long long *counters) {
    __shared__ uint32_t lst[TIP_WORDS * TIP_WALK_BLOCK];
    const unsigned long long nb = counters[TIP_N_BRANCH];
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters[TIP_BRANCH_TOTAL], nb);
    for (unsigned long long i = (unsigned long long) blockIdx.x * TIP_WALK_BLOCK + threadIdx.x; i < nb; i += (unsigned long long) gridDim.x * TIP_WALK_BLOCK) {
        const int32_t beg = branch[i];
        if (!tip_walk_junction(g, beg, max_offset, lst + threadIdx.x, TIP_WALK_BLOCK, kill)) overflow[atomicAdd(&counters[TIP_N_OVERFLOW], 1ull)] = beg;
    }
}

__global__ void __launch_bounds__(TIP_WALK_BLOCK) k_tip_find_overflow(TipGraph g, const int32_t *__restrict__ overflow, int32_t max_offset, uint8_t *kill,
                                                                      int32_t *ws, int32_t n, int32_t n_ws, unsigned long long *counters) {
    const unsigned long long no = counters[TIP_N_OVERFLOW];
    const uint32_t w = blockIdx.x * TIP_WALK_BLOCK + threadIdx.x;
    if (w == 0 && no) atomicAdd(&counters[TIP_OVERFLOW_TOTAL], no);
    if (w >= (uint32_t) n_ws) return;
    for (unsigned long long i = w; i < no; i += (unsigned long long) n_ws) tip_walk_full(g, overflow[i], max_offset, ws + (size_t) w * 5 * (size_t) n, (size_t) n, kill);
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_apply(uint8_t *__restrict__ alive, uint8_t *__restrict__ kill, uint64_t ms, unsigned long long *__restrict__ removed) {
    unsigned long long c = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < ms; i += (uint64_t) gridDim.x * blockDim.x)
        if (kill[i]) { kill[i] = 0; alive[i] = 0; c++; }
    c = tip_wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(removed, c);
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_flags(const uint8_t *__restrict__ alive, uint64_t ms, uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < ms; i += (uint64_t) gridDim.x * blockDim.x) flag[i] = alive[i];
}

__global__ void __launch_bounds__(TIP_BLOCK) k_tip_emit(const alga_edge_dev *__restrict__ est, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                        uint64_t ms, alga_edge_dev *__restrict__ out) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < ms; i += (uint64_t) gridDim.x * blockDim.x)
        if (flag[i]) out[pos[i]] = est[i];
}

unsigned tip_grid(uint64_t items, int block) { return (unsigned) std::min<uint64_t>(std::max<uint64_t>((items + block - 1) / block, 1), 8192); }

}  // namespace

void launch_tip_check(const alga_edge_dev *e, uint64_t m, int32_t n, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_tip_check, dim3(tip_grid(m, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, e, m, n, counters);
}
void launch_tip_keys(const alga_edge_dev *e, uint64_t m, unsigned long long *keys, uint32_t *vals, hipStream_t s) {
    hipLaunchKernelGGL(k_tip_keys, dim3(tip_grid(m, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, e, m, keys, vals);
}
void launch_tip_rev_keys(const alga_edge_dev *est, uint64_t ms, unsigned long long *keys, uint32_t *vals, hipStream_t s) {
    hipLaunchKernelGGL(k_tip_rev_keys, dim3(tip_grid(ms, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, est, ms, keys, vals);
}
void launch_tip_rev_edges(const unsigned long long *keys, const uint32_t *vals, const alga_edge_dev *est, uint64_t ms, alga_edge_dev *rev, uint32_t *rfid,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_tip_rev_edges, dim3(tip_grid(ms, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, keys, vals, est, ms, rev, rfid);
}
void launch_tip_degrees(const TipDir &fwd, const TipDir &rev, const uint8_t *alive, int32_t n, int dir, TipRec *frec, TipRec *rrec, int32_t *branch,
                        unsigned long long *counters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_tip_degrees, dim3((unsigned) ((2ull * (uint64_t) n + TIP_BLOCK - 1) / TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, fwd, rev, alive, n, dir, frec,
                       rrec, branch, counters);
}
void launch_tip_find(const TipGraph &g, const int32_t *branch, int32_t n, int32_t max_offset, uint8_t *kill, int32_t *overflow, unsigned long long *counters,
                     hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_tip_find, dim3(tip_grid((uint64_t) n, TIP_WALK_BLOCK)), dim3(TIP_WALK_BLOCK), 0, s, g, branch, max_offset, kill, overflow, counters);
}
void launch_tip_find_overflow(const TipGraph &g, const int32_t *overflow, int32_t max_offset, uint8_t *kill, int32_t *ws, int32_t n, int32_t n_ws,
                              unsigned long long *counters, hipStream_t s) {
    if (n <= 0 || n_ws <= 0) return;
    hipLaunchKernelGGL(k_tip_find_overflow, dim3((unsigned) ((n_ws + TIP_WALK_BLOCK - 1) / TIP_WALK_BLOCK)), dim3(TIP_WALK_BLOCK), 0, s, g, overflow, max_offset,
                       kill, ws, n, n_ws, counters);
}
void launch_tip_apply(uint8_t *alive, uint8_t *kill, uint64_t ms, unsigned long long *removed, hipStream_t s) {
    hipLaunchKernelGGL(k_tip_apply, dim3(tip_grid(ms, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, alive, kill, ms, removed);
}
void launch_tip_flags(const uint8_t *alive, uint64_t ms, uint32_t *flag, hipStream_t s) {
    hipLaunchKernelGGL(k_tip_flags, dim3(tip_grid(ms, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, alive, ms, flag);
}
void launch_tip_emit(const alga_edge_dev *est, const uint32_t *flag, const uint32_t *pos, uint64_t ms, alga_edge_dev *out, hipStream_t s) {
    hipLaunchKernelGGL(k_tip_emit, dim3(tip_grid(ms, TIP_BLOCK)), dim3(TIP_BLOCK), 0, s, est, flag, pos, ms, out);
}

}  // namespace alga
