// alga_amd/csrc/chain_device.h -- device side of the chain core (chain_kernels.h): the bodies of the kernels in which a stage has a say, and a
// contig's position from the ranked lists.  Included by the *_kernels.hip files only, behind text_record.h (wave_sum); everything here is
// internal to the including file (the build has no relocatable device code).  What differs between the stages enters as
//   Drop     operator()(x, y): the join between the ends x = 2c (64-bit, as the loop counts) and y is dropped (join[] is cleared here): what the stage marks
//   Weight   operator()(x, joined): the weight of state x, joined = the end x ^ 1 it is left at has a join
//   First    operator()(c, id, at, bases, members): contig c is the first of path `id`, whose `members` contigs are listed from `at` on and weigh
//            `bases`: the stage writes the path's length in its own width and counts
#pragma once
#include "chain_kernels.h"

namespace alga {

namespace {

// one thread per contig; only the smallest contig of a cycle writes, and only the two ends of the join at its end 2c
template <class Drop>
__device__ __forceinline__ void chain_cycle_drop_body(const ChainLists &l, uint32_t T, uint32_t *__restrict__ join, const Drop &drop, unsigned long long *__restrict__ dropped) {
    unsigned long long n = 0;
    for (uint64_t c = (uint64_t) blockIdx.x * CHAIN_BLOCK + threadIdx.x; c < T; c += (uint64_t) gridDim.x * CHAIN_BLOCK) {
        if (l.nxt[2 * c] == CHAIN_NONE || l.aux[2 * c] != (uint32_t) c) continue;
        const uint32_t y = join[2 * c];
        join[2 * c] = CHAIN_NONE; join[y] = CHAIN_NONE;
        drop(2 * c, y);
        n++;
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(dropped, n);
}

template <class Weight>
__device__ __forceinline__ void chain_rank_init_body(const uint32_t *__restrict__ join, uint64_t n_states, const ChainLists &l, const Weight &weight) {
    for (uint64_t x = (uint64_t) blockIdx.x * CHAIN_BLOCK + threadIdx.x; x < n_states; x += (uint64_t) gridDim.x * CHAIN_BLOCK) {
        const uint32_t y = join[x ^ 1];
        l.nxt[x] = y; l.aux[x] = 1u; l.tail[x] = (uint32_t) x;
        l.wsum[x] = weight((uint32_t) x, y != CHAIN_NONE);
    }
}

// Contig c in the direction whose first contig has the smaller id: entered at end e (its orientation), as state x; its path has m contigs, c is
// number `rank` of them, hx is the state of the first, and c is left at end `out`.  start = wsum[hx] - wsum[x].
struct ChainPos { uint32_t e, x, m, rank, hx, out; };
__device__ __forceinline__ ChainPos chain_position(const ChainLists &l, uint32_t c) {
    // the list of state 2c + e begins at the contig the other direction ends at
    const uint32_t f0 = l.tail[2 * c + 1] >> 1, l0 = l.tail[2 * c] >> 1;       // first and last contig of the direction that enters c at end 0
    const uint32_t e = f0 <= l0 ? 0u : 1u, x = 2 * c + e;                      // (f0 == l0: a path of one contig, orientation +)
    const uint32_t m = l.aux[x] + l.aux[x ^ 1] - 1u;
    return ChainPos{e, x, m, m - l.aux[x], l.tail[x ^ 1] ^ 1u, x ^ 1u};
}

// ids by ascending first contig, off[] and the member lists by (path, rank) from the two scans (T + 1 entries: the totals are entry T);
// `first` is called for every contig of rank 0
template <class First>
__device__ __forceinline__ void chain_layout_body(const ChainLists &l, uint32_t T, const int32_t *rank_of, const uint8_t *orient, const uint32_t *__restrict__ head,
                                                   const uint32_t *__restrict__ first_scan, const uint32_t *__restrict__ members_scan, int32_t *id_of, uint32_t *off,
                                                   int32_t *members, First first) {
    if (blockIdx.x == 0 && threadIdx.x == 0) off[first_scan[T]] = members_scan[T];
    for (uint64_t c = (uint64_t) blockIdx.x * CHAIN_BLOCK + threadIdx.x; c < T; c += (uint64_t) gridDim.x * CHAIN_BLOCK) {
        const int32_t rank = rank_of[c];
        if (rank < 0) continue;
        const uint32_t h = head[c], id = first_scan[h], at = members_scan[h];
        id_of[c] = (int32_t) id;
        members[at + (uint32_t) rank] = (int32_t) c;
        if (rank == 0) {
            const uint32_t x = 2 * (uint32_t) c + orient[c];
            const unsigned long long bases = l.wsum[x];
            off[id] = at;
            first((uint32_t) c, id, at, bases, l.aux[x]);
        }
    }
}

}  // namespace

}  // namespace alga
