// alga_amd/csrc/seed_index.hip -- the seed index of seed_index.h, built in one place for the placement, the grow and the merge stage.
//   k_seed_keys   (k-mer, column) of every column; a column that is no indexed position gets a key above every k-mer
//   k_seed_dir    directory of the sorted keys on the top bits of the k-mer, one thread per key fills the buckets between its predecessor's and
//                 its own (as k_cr_dir); the distinct k-mers where the caller counts them
// Block 256 and the grid caps are picked, not tuned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "engine_internal.h"
#include "ingest_kernels.h"
#include "seed_device.h"
#include "text_record.h"

namespace alga {

namespace {

__global__ void __launch_bounds__(SEED_BLOCK) k_seed_keys(SeedSpace sp, int32_t k, unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
    for (uint64_t g = (uint64_t) blockIdx.x * SEED_BLOCK + threadIdx.x; g < sp.columns; g += (uint64_t) gridDim.x * SEED_BLOCK) {
        const uint32_t i = item_of(sp.off, sp.n, (uint32_t) g);
        const uint64_t q = g - (uint64_t) sp.off[i];
        keys[g] = q + (uint64_t) k <= (uint64_t) sp.len[i] ? col_kmer(sp.cols, (uint32_t) g, k) : 1ull << (2 * k);      // above every k-mer, inside the 2k + 1 sorted bits
        vals[g] = (uint32_t) g;
    }
}

__global__ void __launch_bounds__(SEED_BLOCK) k_seed_dir(const unsigned long long *__restrict__ keys, uint64_t n, int shift, uint32_t n_buckets, uint32_t *__restrict__ dir,
                                                         unsigned long long *__restrict__ distinct) {
    const uint64_t j = (uint64_t) blockIdx.x * SEED_BLOCK + threadIdx.x;
    unsigned long long head = 0;
    if (j <= n) {
        const uint32_t lo = j == 0 ? 0u : (uint32_t) (keys[j - 1] >> shift) + 1u;
        const uint32_t hi = j < n ? (uint32_t) (keys[j] >> shift) : n_buckets;
        for (uint32_t b = lo; b <= hi && b <= n_buckets; b++) dir[b] = (uint32_t) j;
        head = j < n && (j == 0 || keys[j - 1] != keys[j]) ? 1ull : 0ull;
    }
    if (!distinct) return;
    head = wave_sum(head);
    if ((threadIdx.x & 63) == 0 && head) atomicAdd(distinct, head);
}

}  // namespace

int seed_blocks(uint64_t queries, int n_cu) {
    return (int) std::max<uint64_t>(1, std::min<uint64_t>((queries + SEED_WAVES - 1) / SEED_WAVES, (uint64_t) std::max(1, n_cu) * 8u));
}

size_t seed_scratch_words(int blocks, int64_t max_query_len, int32_t k) {
    const size_t per_wave = (size_t) std::max<int64_t>(1, (max_query_len / k + 63) / 64);
    return (size_t) blocks * SEED_WAVES * per_wave;
}

}  // namespace alga

using namespace alga;

// (a space without columns launches no key kernel and sorts nothing; the directory is filled for n_index = 0 too: every look-up finds an empty bucket)
int alga_seed_index(alga_engine *e, const SeedSpace &sp, int32_t k, uint64_t n_index, unsigned long long *d_distinct, hipStream_t s, SeedIndex *out) {
    int rc, bits = e->opt_place_dir_bits;
    if (bits <= 0) { bits = 1; while (bits < SEED_DIR_BITS_MAX && (n_index >> bits) > 2) bits++; }
    bits = std::min(bits, 2 * k);
    for (int j = 0; j < 2; j++) {
        if ((rc = alga_ensure(e, e->seed_keys[j], (sp.columns + 2) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->seed_vals[j], (sp.columns + 2) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->seed_dir, (((size_t) 1 << bits) + 2) * sizeof(uint32_t)))) return rc;
    const size_t temp = sort_u64_u32_temp_bytes(sp.columns);
    if ((rc = alga_ensure(e, e->sort_temp, temp))) return rc;
    unsigned long long *keys = (unsigned long long *) e->seed_keys[0].p, *sorted = (unsigned long long *) e->seed_keys[1].p;
    uint32_t *vals = (uint32_t *) e->seed_vals[0].p, *sorted_vals = (uint32_t *) e->seed_vals[1].p, *dir = (uint32_t *) e->seed_dir.p;
    const uint64_t key_blocks = std::min<uint64_t>((sp.columns + SEED_BLOCK - 1) / SEED_BLOCK, 1u << 16);
    if (sp.columns) hipLaunchKernelGGL(k_seed_keys, dim3((unsigned) key_blocks), dim3(SEED_BLOCK), 0, s, sp, k, keys, vals);
    if ((rc = alga_check_launch(e, "k_seed_keys"))) return rc;
    HIP_TRY(e, sort_u64_u32(e->sort_temp.p, temp, keys, sorted, vals, sorted_vals, sp.columns, 2 * k + 1, s));
    *out = SeedIndex{sorted, sorted_vals, dir, 2 * k - bits, (uint32_t) n_index};
    hipLaunchKernelGGL(k_seed_dir, dim3((unsigned) ((n_index + 1 + SEED_BLOCK - 1) / SEED_BLOCK)), dim3(SEED_BLOCK), 0, s, sorted, n_index, out->shift, 1u << bits, dir,
                       d_distinct);
    return alga_check_launch(e, "k_seed_dir");
}
