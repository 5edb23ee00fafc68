// alga_amd/csrc/chain_kernels.hip -- the chain core of chain_kernels.h: the jump kernels, in which no stage has a say, and the host side of
// the two phases, the workspace and the scans.  Integer work only, nothing depends on thread order.  Block 256 and the grid cap are picked, not
// tuned; the calling stage's max_blocks lowers the cap (a knob of the tests, which make every grid-stride loop here take further passes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "chain_kernels.h"
#include "engine_internal.h"

namespace alga {

namespace {

__global__ void __launch_bounds__(CHAIN_BLOCK) k_ch_cycle_init(const uint32_t *__restrict__ join, uint64_t n_states, ChainLists l) {
    for (uint64_t x = (uint64_t) blockIdx.x * CHAIN_BLOCK + threadIdx.x; x < n_states; x += (uint64_t) gridDim.x * CHAIN_BLOCK) {
        l.nxt[x] = join[x ^ 1]; l.aux[x] = (uint32_t) (x >> 1);
    }
}

__global__ void __launch_bounds__(CHAIN_BLOCK) k_ch_cycle_jump(uint64_t n_states, ChainLists from, ChainLists to) {
    for (uint64_t x = (uint64_t) blockIdx.x * CHAIN_BLOCK + threadIdx.x; x < n_states; x += (uint64_t) gridDim.x * CHAIN_BLOCK) {
        const uint32_t y = from.nxt[x];
        uint32_t m = from.aux[x], z = CHAIN_NONE;
        if (y != CHAIN_NONE) { const uint32_t my = from.aux[y]; m = my < m ? my : m; z = from.nxt[y]; }
        to.nxt[x] = z; to.aux[x] = m;
    }
}

__global__ void __launch_bounds__(CHAIN_BLOCK) k_ch_rank_jump(uint64_t n_states, ChainLists from, ChainLists to) {
    for (uint64_t x = (uint64_t) blockIdx.x * CHAIN_BLOCK + threadIdx.x; x < n_states; x += (uint64_t) gridDim.x * CHAIN_BLOCK) {
        const uint32_t y = from.nxt[x];
        uint32_t d = from.aux[x], tl = from.tail[x], z = CHAIN_NONE;
        unsigned long long w = from.wsum[x];
        if (y != CHAIN_NONE) { d += from.aux[y]; w += from.wsum[y]; tl = from.tail[y]; z = from.nxt[y]; }
        to.nxt[x] = z; to.aux[x] = d; to.tail[x] = tl; to.wsum[x] = w;
    }
}

inline unsigned ch_grid(uint64_t items, uint64_t cap) {
    const uint64_t g = (items + CHAIN_BLOCK - 1) / CHAIN_BLOCK;
    return (unsigned) std::max<uint64_t>(1, std::min<uint64_t>(g, cap));
}

}  // namespace

static int chain_rounds(uint64_t n_states) {                              // ceil(log2(n_states)) + 1
    int rounds = 1;
    while (rounds < 33 && (1ull << rounds) < n_states) rounds++;
    return rounds + 1;
}
void launch_ch_cycle_init(const uint32_t *join, uint64_t n_states, const ChainLists &l, uint32_t max_blocks, hipStream_t s) {
    if (n_states) hipLaunchKernelGGL(k_ch_cycle_init, dim3(ch_grid(n_states, max_blocks)), dim3(CHAIN_BLOCK), 0, s, join, n_states, l);
}
void launch_ch_cycle_jump(uint64_t n_states, const ChainLists &from, const ChainLists &to, uint32_t max_blocks, hipStream_t s) {
    if (n_states) hipLaunchKernelGGL(k_ch_cycle_jump, dim3(ch_grid(n_states, max_blocks)), dim3(CHAIN_BLOCK), 0, s, n_states, from, to);
}
void launch_ch_rank_jump(uint64_t n_states, const ChainLists &from, const ChainLists &to, uint32_t max_blocks, hipStream_t s) {
    if (n_states) hipLaunchKernelGGL(k_ch_rank_jump, dim3(ch_grid(n_states, max_blocks)), dim3(CHAIN_BLOCK), 0, s, n_states, from, to);
}

}  // namespace alga

using namespace alga;

// (the 64-bit sums first, so that every array is aligned to its entries)
int alga_chain_work(alga_engine *e, uint64_t T, ChainWork *w) {
    const uint64_t ns = 2 * T + 2, nc = T + 2;
    int rc;
    if ((rc = alga_ensure(e, e->chain_work, ns * (2 * sizeof(unsigned long long) + 7 * sizeof(uint32_t)) + nc * 5 * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(nc)))) return rc;
    unsigned long long *p64 = (unsigned long long *) e->chain_work.p;
    for (ChainLists &l : w->set) { l.wsum = p64; p64 += ns; }
    uint32_t *p = (uint32_t *) p64;
    for (ChainLists &l : w->set) { l.nxt = p; l.aux = p + ns; l.tail = p + 2 * ns; p += 3 * ns; }
    w->join = p; p += ns;
    w->head = p; w->first = p + nc; w->members = p + 2 * nc; w->first_scan = p + 3 * nc; w->members_scan = p + 4 * nc;
    return ALGA_OK;
}

int alga_chain_cycles(alga_engine *e, const ChainWork &w, const uint32_t *join, uint64_t n_states, bool may_join, uint32_t max_blocks, hipStream_t s,
                      const ChainLists **res) {
    int cur = 0;
    if (may_join) launch_ch_cycle_init(join, n_states, w.set[0], max_blocks, s);
    for (int k = may_join ? chain_rounds(n_states) : 0; k > 0; k--, cur ^= 1) launch_ch_cycle_jump(n_states, w.set[cur], w.set[cur ^ 1], max_blocks, s);
    *res = may_join ? &w.set[cur] : nullptr;
    return alga_check_launch(e, "k_ch_cycle_jump");
}

int alga_chain_ranks(alga_engine *e, const ChainWork &w, uint64_t n_states, bool may_join, uint32_t max_blocks, hipStream_t s, const ChainLists **res) {
    int cur = 0;
    for (int k = may_join ? chain_rounds(n_states) : 0; k > 0; k--, cur ^= 1) launch_ch_rank_jump(n_states, w.set[cur], w.set[cur ^ 1], max_blocks, s);
    *res = &w.set[cur];
    return alga_check_launch(e, "k_ch_rank_jump");
}

int alga_chain_scans(alga_engine *e, const ChainWork &w, uint64_t T, const char *what, hipStream_t s) {
    launch_exclusive_scan(w.first, T + 1, w.first_scan, (uint64_t *) e->scan_scratch.p, s);
    launch_exclusive_scan(w.members, T + 1, w.members_scan, (uint64_t *) e->scan_scratch.p, s);
    return alga_check_launch(e, what);
}
