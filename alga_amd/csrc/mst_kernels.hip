// alga_amd/csrc/mst_kernels.hip -- removal of short parallel paths on the overlap graph (include/alga_amd.h:
// alga_remove_short_parallel_paths_device; the reference: GraphSimplifier::removeShortParallelPaths / tryToRemoveShortPathsMST).
//
// Integer work only.  The reference runs the nodes in ascending order, each on the graph the earlier ones left; a beg touches only the rows of
// the nodes within max_offset of it and only ever removes edges, so begs with disjoint balls commute (the argument is in the header).  The
// host (engine_simplify.hip) runs rounds over mutable rows of fixed capacity (the input's CSR, a length per row):
//   k_mst_claim    every pending beg that still has >= 2 entries: its ball (mst_walk.h: mst_ball), each node of it claimed with an atomicMin
//                  of (round tag, beg) into owner[] -- the tag makes every earlier round's claim larger, so owner[] is never cleared
//   k_mst_select   the ball again (nothing has changed): a beg that holds every node of its ball wins -> win[]; every other one that still
//                  branches -> the next round's pending list.  The smallest pending id always wins.
//   k_mst_run      every winner: the literal step (mst_run) on the live rows.  Winners' balls are disjoint, so are the rows they touch.
// One unit of work per beg, and the walk is sequential by definition (list order, dst[] overwritten).  A beg's state -- a map of 256 slots,
// 192 nodes, 256 collected edges, 5.75 KB -- is in LDS, one state per wave, and lane 0 walks: 27 states fit into a CU's 160 KB whatever
// the block shape, so the LDS, not the idle lanes, bounds the begs in flight (27 per CU = 6.75 per SIMD; the compiler's report rounds it to 7 waves per
// SIMD -- a figure of the compiler, not a measured one), and the wave's other lanes would only
// multiply a state that is already the limit.  The kernels wait on dependent gathers of short rows; what hides that latency is the number
// of resident walks.
//   k_mst_*_overflow   the begs whose state does not fit (rows of hundreds of edges, balls of several hundred nodes): the same functions on
//                  a state in a device workspace, one thread per workspace, in two tiers: many states of a few thousand nodes and edges, then
//                  a few sized for the whole graph, which cannot fail.  A form that gives up has written nothing outside its own state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mst_kernels.h"

namespace alga {

namespace {

constexpr int MST_BLOCK = 256;
constexpr int MST_WAVE = 64;                                        // a block of the walk kernels: one wave, one state
constexpr uint32_t MST_LDS_WORDS = 2 * (1u << MST_LDS_HBITS) + MST_LDS_NODES + 3 * MST_LDS_EDGES;
enum { MST_CLAIM = 0, MST_SELECT = 1, MST_RUN = 2 };

__global__ void __launch_bounds__(MST_BLOCK) k_mst_check(const alga_edge_dev *__restrict__ e, uint64_t m, int32_t n, unsigned long long *__restrict__ counters) {
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t) gridDim.x * blockDim.x) {
        const alga_edge_dev x = e[i];
        if (x.src < 0 || x.src >= n || x.dst < 0 || x.dst >= n) bad |= MST_BAD_ID;
        if (x.offset < 0) bad |= MST_BAD_OFFSET;
        if (i && e[i - 1].src > x.src) bad |= MST_BAD_ORDER;
    }
    if (bad) atomicOr(&counters[MST_FLAGS], bad);
}

__global__ void __launch_bounds__(MST_BLOCK) k_mst_init(const uint32_t *__restrict__ rowptr, int32_t n, uint32_t *__restrict__ len,
                                                        unsigned long long *__restrict__ owner, int32_t *__restrict__ pend,
                                                        unsigned long long *__restrict__ counters) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (uint32_t) n) return;
    const uint32_t l = rowptr[v + 1] - rowptr[v];
    len[v] = l;
    owner[v] = ~0ull;
    if (l >= 2) pend[atomicAdd(&counters[MST_N_PEND0], 1ull)] = (int32_t) v;
}

// what one beg does in the phase MODE on the state `st` -> false: the state is too small (nothing outside it has been written)
template <int MODE>
__device__ __forceinline__ bool mst_unit(const MstRound &r, int32_t beg, const MstState &st, uint32_t &ball_max) {
    if (MODE == MST_RUN) {
        uint32_t n_map, n_col;
        return mst_run(r.g, beg, r.max_offset, st, n_map, n_col);
    }
    if (r.g.len[beg] < 2) return true;                              // no longer branches: dropped, its degree never rises again
    uint32_t ns;
    const bool ok = mst_ball(r.g, beg, r.max_offset, st, ns);
    const unsigned long long mine = r.tag | (uint32_t) beg;
    if (ok && MODE == MST_CLAIM) {
        for (uint32_t i = 0; i < ns; i++) atomicMin(&r.owner[st.key[st.slots[i]] & ~MST_FLAG], mine);
        ball_max = ns > ball_max ? ns : ball_max;
    }
    if (ok && MODE == MST_SELECT) {
        bool wins = true;
        for (uint32_t i = 0; i < ns && wins; i++) wins = r.owner[st.key[st.slots[i]] & ~MST_FLAG] == mine;
        if (wins) r.win[atomicAdd(&r.counters[MST_N_WIN], 1ull)] = beg;
        else r.pend_next[atomicAdd(&r.counters[MST_N_PEND0 + r.next], 1ull)] = beg;
    }
    mst_clear(st, ns);
    return ok;
}

template <int MODE>
__device__ __forceinline__ void mst_short(const MstRound &r, const int32_t *__restrict__ list, int count_at, uint32_t *lds) {
    for (uint32_t i = threadIdx.x; i < (1u << MST_LDS_HBITS); i += MST_WAVE) lds[i] = MST_EMPTY;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const MstState st{lds, lds + (1u << MST_LDS_HBITS), MST_LDS_HBITS, lds + 2 * (1u << MST_LDS_HBITS), MST_LDS_NODES,
                      lds + 2 * (1u << MST_LDS_HBITS) + MST_LDS_NODES, MST_LDS_EDGES};
    const unsigned long long count = r.counters[count_at];
    uint32_t ball_max = 0;
    for (unsigned long long i = blockIdx.x; i < count; i += gridDim.x) {
        const int32_t beg = list[i];
        if (!mst_unit<MODE>(r, beg, st, ball_max)) r.overflow[atomicAdd(&r.counters[MST_N_OVF_CLAIM + MODE], 1ull)] = beg;
    }
    if (MODE == MST_CLAIM && ball_max) atomicMax(&r.counters[MST_BALL_MAX], (unsigned long long) ball_max);
}

// tier 0: the begs of r.overflow on the states of `t`, what does not fit -> r.overflow2; tier 1: the begs of r.overflow2 (its states hold anything)
template <int MODE>
__device__ __forceinline__ void mst_long(const MstRound &r, const MstTier &t, int tier) {
    const int32_t *list = tier ? r.overflow2 : r.overflow;
    const unsigned long long no = r.counters[(tier ? MST_N_OVF2_CLAIM : MST_N_OVF_CLAIM) + MODE];
    const uint32_t w = blockIdx.x * MST_WAVE + threadIdx.x;
    if (MODE == MST_RUN && tier == 0 && w == 0 && no) atomicAdd(&r.counters[MST_OVERFLOW_TOTAL], no);
    if (w >= (uint32_t) t.n_ws) return;
    const size_t H = (size_t) 1 << t.hbits;
    uint32_t *base = t.ws + (size_t) w * (2 * H + (size_t) t.cap_nodes + 3 * (size_t) t.cap_edges);
    const MstState st{base, base + H, t.hbits, base + 2 * H, t.cap_nodes, base + 2 * H + (size_t) t.cap_nodes, t.cap_edges};
    uint32_t ball_max = 0;
    for (unsigned long long i = w; i < no; i += (unsigned long long) t.n_ws) {
        const int32_t beg = list[i];
        if (!mst_unit<MODE>(r, beg, st, ball_max) && tier == 0) r.overflow2[atomicAdd(&r.counters[MST_N_OVF2_CLAIM + MODE], 1ull)] = beg;
    }
    if (MODE == MST_CLAIM && ball_max) atomicMax(&r.counters[MST_BALL_MAX], (unsigned long long) ball_max);
}

__global__ void __launch_bounds__(MST_WAVE) k_mst_claim(MstRound r, const int32_t *__restrict__ pend, int cur) {
    __shared__ uint32_t lds[MST_LDS_WORDS];
    mst_short<MST_CLAIM>(r, pend, MST_N_PEND0 + cur, lds);
}
__global__ void __launch_bounds__(MST_WAVE) k_mst_select(MstRound r, const int32_t *__restrict__ pend, int cur) {
    __shared__ uint32_t lds[MST_LDS_WORDS];
    mst_short<MST_SELECT>(r, pend, MST_N_PEND0 + cur, lds);
}
__global__ void __launch_bounds__(MST_WAVE) k_mst_run(MstRound r) {
    __shared__ uint32_t lds[MST_LDS_WORDS];
    mst_short<MST_RUN>(r, r.win, MST_N_WIN, lds);
}
__global__ void __launch_bounds__(MST_WAVE) k_mst_claim_overflow(MstRound r, MstTier t, int tier) { mst_long<MST_CLAIM>(r, t, tier); }
__global__ void __launch_bounds__(MST_WAVE) k_mst_select_overflow(MstRound r, MstTier t, int tier) { mst_long<MST_SELECT>(r, t, tier); }
__global__ void __launch_bounds__(MST_WAVE) k_mst_run_overflow(MstRound r, MstTier t, int tier) { mst_long<MST_RUN>(r, t, tier); }

unsigned mst_grid(uint64_t items, int block) { return (unsigned) std::min<uint64_t>(std::max<uint64_t>((items + block - 1) / block, 1), 8192); }

template <typename K>
void mst_launch_tiers(K kernel, const MstRound &r, const MstTiers &t, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((unsigned) ((t.mid.n_ws + MST_WAVE - 1) / MST_WAVE)), dim3(MST_WAVE), 0, s, r, t.mid, 0);
    if (t.big.n_ws > 0) hipLaunchKernelGGL(kernel, dim3((unsigned) ((t.big.n_ws + MST_WAVE - 1) / MST_WAVE)), dim3(MST_WAVE), 0, s, r, t.big, 1);
}

}  // namespace

uint32_t mst_hbits_for(uint64_t nodes) {
    uint32_t b = 2;
    while (b < 31 && ((uint64_t) 1 << b) < 2 * nodes) b++;
    return b;
}

void launch_mst_check(const alga_edge_dev *e, uint64_t m, int32_t n, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_mst_check, dim3(mst_grid(m, MST_BLOCK)), dim3(MST_BLOCK), 0, s, e, m, n, counters);
}
void launch_mst_init(const uint32_t *rowptr, int32_t n, uint32_t *len, unsigned long long *owner, int32_t *pend, unsigned long long *counters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_mst_init, dim3((unsigned) (((uint64_t) n + MST_BLOCK - 1) / MST_BLOCK)), dim3(MST_BLOCK), 0, s, rowptr, n, len, owner, pend, counters);
}
void launch_mst_claim(const MstRound &r, const int32_t *pend, int cur, uint64_t n_pend, const MstTiers &t, hipStream_t s) {
    hipLaunchKernelGGL(k_mst_claim, dim3(mst_grid(n_pend, 1)), dim3(MST_WAVE), 0, s, r, pend, cur);
    mst_launch_tiers(k_mst_claim_overflow, r, t, s);
}
void launch_mst_select(const MstRound &r, const int32_t *pend, int cur, uint64_t n_pend, const MstTiers &t, hipStream_t s) {
    hipLaunchKernelGGL(k_mst_select, dim3(mst_grid(n_pend, 1)), dim3(MST_WAVE), 0, s, r, pend, cur);
    mst_launch_tiers(k_mst_select_overflow, r, t, s);
}
void launch_mst_run(const MstRound &r, uint64_t n_win, const MstTiers &t, hipStream_t s) {
    hipLaunchKernelGGL(k_mst_run, dim3(mst_grid(n_win, 1)), dim3(MST_WAVE), 0, s, r);
    mst_launch_tiers(k_mst_run_overflow, r, t, s);
}

}  // namespace alga
