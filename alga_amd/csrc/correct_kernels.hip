// alga_amd/csrc/correct_kernels.hip -- read error correction by the k-mer spectrum (include/alga_amd.h: alga_correct_reads_device; the definition is
// the comment there, host side in engine_correct.hip).
//
// A k-mer (k <= 31: at most 62 bits, base j in bits 2j, 2j + 1) is taken straight from the row words; its canonical form is the smaller of the
// value and its reverse complement's value; the MIXED key is an invertible 64-bit mix of that, so equal keys are equal k-mers and the top bits
// spread evenly (they are the histogram bin, the slice order and the directory bucket).
//   k_cr_twin     row 2r is the reverse complement of row 2r + 1, lengths equal and within the stride: one wave per read, one lane per word
//   k_cr_hist     occurrences per bin (top 12 bits), in LDS; one table row per block, no global atomics
//   k_cr_sum      column sums of such a table
//   k_cr_emit     keys of the occurrences of one slice of bins, block-compacted: counted, one atomicAdd per block, written
//   k_cr_runs     over the sorted keys of a slice: heads of the runs of >= solid_min equal keys (key[j + solid_min - 1] == key[j]), run heads counted
//   k_cr_append   the solid keys of a slice behind those of the slices before it: the solid array is sorted as a whole
//   k_cr_dir      directory of the solid array on the top bits of the key, one thread per key: it fills the buckets between its predecessor's and its own
//   k_cr_fix      one wave per forward read.  Rows of up to 64 words (1024 nt) are held one word per lane and read by cross-lane moves, longer ones
//                 come from memory.  Lanes take k-mers, 64 at a time; the weak bits are a ballot, walked as a wave-uniform bit mask with the open
//                 run carried to the next chunk.  A closed run's candidates are (k-mer of the run) x (3 other bases) on the lanes, in passes of
//                 64; lane 0 writes the one base that works into both rows.  Membership: one directory read, a bisection while the bucket is
//                 longer than 8 keys, then a scan of the rest.
// Four waves per block everywhere; k_cr_fix runs 8 blocks per CU (the lookups are dependent random reads: occupancy is what hides them).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "correct_kernels.h"
#include "prefsuf_common.h"

namespace alga {

namespace {

constexpr int CR_BLOCK = 256, CR_WAVES = CR_BLOCK / 64;
constexpr int CR_LANE_WORDS = 64;            // a row of at most this many words lives in the wave's registers
constexpr int CR_SCAN_MAX = 8;               // a bucket is bisected down to this many keys, then scanned

__device__ __forceinline__ unsigned long long cr_mix(unsigned long long x) {      // invertible (xor-shifts and odd multipliers)
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// mixed key of the canonical form of the k-mer value v (2k bits)
__device__ __forceinline__ unsigned long long cr_key(unsigned long long v, int k) {
    unsigned long long x = __brevll(v);
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);   // base j now in slot 31 - j
    const unsigned long long rc = (~x) >> (64 - 2 * k);
    return cr_mix(v < rc ? v : rc);
}

// the k-mer at base i of a row of nw words; word(w) is called for three clamped indices by every lane (it may be a cross-lane move)
template <class W>
__device__ __forceinline__ unsigned long long cr_kmer(W word, int nw, int i, int k) {
    const int w = i >> 4, sh = (i & 15) << 1;
    const uint32_t w0 = word(w), w1 = word(min(w + 1, nw - 1)), w2 = word(min(w + 2, nw - 1));
    const unsigned long long lo = (unsigned long long) w0 | (w + 1 < nw ? (unsigned long long) w1 << 32 : 0ull);
    unsigned long long v = lo >> sh;
    if (sh && w + 2 < nw) v |= (unsigned long long) w2 << (64 - sh);
    return v & ((1ull << (2 * k)) - 1ull);
}

__device__ __forceinline__ bool cr_is_solid(const unsigned long long *__restrict__ solid, const uint32_t *__restrict__ dir, int shift, unsigned long long key) {
    const uint32_t b = (uint32_t) (key >> shift);
    uint32_t lo = dir[b], hi = dir[b + 1];
    while (hi - lo > (uint32_t) CR_SCAN_MAX && hi > lo) {        // if the key is there, it is in [lo, hi)
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (solid[mid] <= key) lo = mid; else hi = mid;
    }
    bool found = false;
    for (uint32_t j = lo; j < hi; j++) found |= solid[j] == key;
    return found;
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_twin(CrReads c, uint32_t *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t) blockIdx.x * CR_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * CR_WAVES;
    for (uint64_t r = wave; r < c.R; r += n_waves) {
        const int32_t lf = c.len[2 * r + 1], lr = c.len[2 * r];
        if (lf != lr) { if (lane == 0) *bad = 1u; continue; }
        if (lf <= 0) continue;
        const int nw = blocks_of(lf);
        if (nw > c.stride) { if (lane == 0) *bad = 1u; continue; }
        const uint32_t *fw = c.rows + (2 * r + 1) * (size_t) c.stride, *rv = c.rows + (2 * r) * (size_t) c.stride;
        bool differs = false;
        for (int w = lane; w < nw; w += 64) {
            uint32_t v = 0;
            for (int j = 0; j < 16; j++) {
                const int pos = 16 * w + j;
                if (pos < lf) {
                    const int q = lf - 1 - pos;
                    v |= (3u - ((fw[q >> 4] >> ((q & 15) << 1)) & 3u)) << (2 * j);
                }
            }
            differs |= v != rv[w];
        }
        if (differs) *bad = 1u;
    }
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_hist(CrReads c, uint32_t *__restrict__ table) {
    __shared__ uint32_t sh[CR_HIST_COLS];
    for (int j = threadIdx.x; j < CR_HIST_COLS; j += CR_BLOCK) sh[j] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t) blockIdx.x * CR_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * CR_WAVES;
    for (uint64_t r = wave; r < c.R; r += n_waves) {
        const int32_t len = c.len[2 * r + 1];
        if (len < c.k) continue;
        const int nk = len - c.k + 1, nw = blocks_of(len);
        const uint32_t *fw = c.rows + (2 * r + 1) * (size_t) c.stride;
        auto word = [&](int w) { return fw[w]; };
        if (lane == 0) atomicAdd(&sh[CR_HIST_READS], 1u);
        for (int i = lane; i < nk; i += 64) atomicAdd(&sh[(uint32_t) (cr_key(cr_kmer(word, nw, i, c.k), c.k) >> (64 - CR_BIN_BITS))], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < CR_HIST_COLS; j += CR_BLOCK) table[(size_t) blockIdx.x * CR_HIST_COLS + j] = sh[j];
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_sum(const uint32_t *__restrict__ table, int rows, int cols, unsigned long long *__restrict__ out, int accumulate) {
    const int col = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (col >= cols) return;
    unsigned long long sum = accumulate ? out[col] : 0ull;
    for (int r = 0; r < rows; r++) sum += table[(size_t) r * cols + col];
    out[col] = sum;
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_emit(CrReads c, uint32_t bin_lo, uint32_t bin_hi, unsigned long long *__restrict__ keys, uint64_t cap,
                                                      unsigned long long *__restrict__ cursor) {
    __shared__ unsigned long long wave_cnt[CR_WAVES], wave_base[CR_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t) blockIdx.x * CR_WAVES + wv, n_waves = (uint64_t) gridDim.x * CR_WAVES;
    unsigned long long off = 0;
    // two passes over the wave's reads: count, then (with the block's base known) write
    for (int pass = 0; pass < 2; pass++) {
        for (uint64_t r = wave; r < c.R; r += n_waves) {
            const int32_t len = c.len[2 * r + 1];
            if (len < c.k) continue;
            const int nk = len - c.k + 1, nw = blocks_of(len);
            const uint32_t *fw = c.rows + (2 * r + 1) * (size_t) c.stride;
            auto word = [&](int w) { return fw[w]; };
            for (int i0 = 0; i0 < nk; i0 += 64) {
                const int i = i0 + lane;
                unsigned long long key = 0;
                bool in = false;
                if (i < nk) {
                    key = cr_key(cr_kmer(word, nw, i, c.k), c.k);
                    const uint32_t bin = (uint32_t) (key >> (64 - CR_BIN_BITS));
                    in = bin >= bin_lo && bin < bin_hi;
                }
                const unsigned long long m = __ballot(in);
                if (pass == 1 && in) {
                    const unsigned long long at = off + (unsigned long long) __popcll(m & ((1ull << lane) - 1ull));
                    if (at < cap) keys[at] = key;
                }
                off += (unsigned long long) __popcll(m);
            }
        }
        if (pass == 0) {
            if (lane == 0) wave_cnt[wv] = off;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long total = 0;
                for (int j = 0; j < CR_WAVES; j++) { wave_base[j] = total; total += wave_cnt[j]; }
                const unsigned long long base = total ? atomicAdd(cursor, total) : 0ull;
                for (int j = 0; j < CR_WAVES; j++) wave_base[j] += base;
            }
            __syncthreads();
            off = wave_base[wv];
        }
    }
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_runs(const unsigned long long *__restrict__ keys, uint64_t n, int32_t solid_min, uint32_t *__restrict__ flags,
                                                      uint32_t *__restrict__ table) {
    __shared__ uint32_t heads_sh;
    if (threadIdx.x == 0) heads_sh = 0u;
    __syncthreads();
    uint32_t heads = 0;
    for (uint64_t j = (uint64_t) blockIdx.x * CR_BLOCK + threadIdx.x; j < n; j += (uint64_t) gridDim.x * CR_BLOCK) {
        const unsigned long long x = keys[j];
        const bool head = j == 0 || keys[j - 1] != x;
        const uint64_t last = j + (uint64_t) solid_min - 1u;
        flags[j] = head && last < n && keys[last] == x ? 1u : 0u;
        heads += head ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) heads += __shfl_xor(heads, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&heads_sh, heads);
    __syncthreads();
    if (threadIdx.x == 0) table[blockIdx.x] = heads_sh;
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_append(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ pos,
                                                        uint64_t n, unsigned long long *__restrict__ solid, uint64_t base, uint64_t cap) {
    for (uint64_t j = (uint64_t) blockIdx.x * CR_BLOCK + threadIdx.x; j < n; j += (uint64_t) gridDim.x * CR_BLOCK) {
        if (!flags[j]) continue;
        const uint64_t at = base + pos[j];
        if (at < cap) solid[at] = keys[j];
    }
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_dir(const unsigned long long *__restrict__ solid, uint64_t n, int shift, uint32_t n_buckets, uint32_t *__restrict__ dir,
                                                     uint32_t *__restrict__ bad) {
    const uint64_t j = (uint64_t) blockIdx.x * CR_BLOCK + threadIdx.x;
    if (j > n) return;
    // fail closed: over keys that do not ascend the directory would name buckets that hold other keys (nothing faults: every bucket index is
    // below 2^bits whatever the keys are)
    if (j >= 1 && j < n && solid[j] <= solid[j - 1]) *bad = 1u;
    const uint32_t lo = j == 0 ? 0u : (uint32_t) (solid[j - 1] >> shift) + 1u;
    const uint32_t hi = j < n ? (uint32_t) (solid[j] >> shift) : n_buckets;
    for (uint32_t b = lo; b <= hi && b <= n_buckets; b++) dir[b] = (uint32_t) j;
}

__global__ void __launch_bounds__(CR_BLOCK) k_cr_fix(CrReads c, CrFix f, uint32_t *__restrict__ table) {
    __shared__ uint32_t cnt_sh[CR_COLS];
    if (threadIdx.x < CR_COLS) cnt_sh[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, k = c.k, shift = 64 - f.dir_bits;
    const uint64_t wave = (uint64_t) blockIdx.x * CR_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * CR_WAVES;
    uint32_t n_runs = 0, n_fixed = 0, n_amb = 0, n_none = 0, n_skip = 0, n_changed = 0;     // wave-uniform
    for (uint64_t r = wave; r < c.R; r += n_waves) {
        const int32_t len = c.len[2 * r + 1];
        if (len < k) continue;
        const int nk = len - k + 1, nw = blocks_of(len);
        uint32_t *fw = c.rows + (2 * r + 1) * (size_t) c.stride, *rv = c.rows + (2 * r) * (size_t) c.stride;
        const bool in_lanes = nw <= CR_LANE_WORDS;
        const uint32_t mine = in_lanes && lane < nw ? fw[lane] : 0u;
        auto word = [&](int w) -> uint32_t { return in_lanes ? (uint32_t) __shfl((int) mine, w) : fw[w]; };
        bool changed = false;

        // one maximal run of weak k-mers [a, b], closed
        auto run = [&](int a, int b) {
            n_runs++;
            const int L = b - a + 1;
            int p = -1;
            if (L < f.min_run || (a == 0 && b == nk - 1)) p = -1;
            else if (a > 0 && b < nk - 1) { if (L == k) p = b; }
            else if (a == 0) { if (b <= k - 1) p = b; }
            else { if (L <= k) p = a + k - 1; }
            if (p < 0) { n_skip++; return; }
            const uint32_t orig = (word(p >> 4) >> ((p & 15) << 1)) & 3u;
            unsigned long long fail0 = 0, fail1 = 0, fail2 = 0;
            for (int t0 = 0; t0 < 3 * L; t0 += 64) {
                const int t = t0 + lane;
                const bool act = t < 3 * L;
                const int tc = act ? t : 0, alt = tc / L, i = a + (tc - alt * L);
                unsigned long long v = cr_kmer(word, nw, i, k);
                const uint32_t nb = (orig + 1u + (uint32_t) alt) & 3u;
                v ^= (unsigned long long) (orig ^ nb) << (2 * (p - i));          // 0 <= p - i <= k - 1: every k-mer of the run holds p
                const bool bad = act && !cr_is_solid(f.solid, f.dir, shift, cr_key(v, k));
                fail0 |= __ballot(bad && alt == 0);
                fail1 |= __ballot(bad && alt == 1);
                fail2 |= __ballot(bad && alt == 2);
            }
            const int works = (fail0 == 0) + (fail1 == 0) + (fail2 == 0);
            if (works == 0) { n_none++; return; }
            if (works > 1) { n_amb++; return; }
            n_fixed++;
            changed = true;
            if (lane == 0) {
                const uint32_t nb = (orig + 1u + (fail0 == 0 ? 0u : (fail1 == 0 ? 1u : 2u))) & 3u;
                const int q = len - 1 - p, sp = (p & 15) << 1, sq = (q & 15) << 1;
                fw[p >> 4] = (fw[p >> 4] & ~(3u << sp)) | (nb << sp);
                rv[q >> 4] = (rv[q >> 4] & ~(3u << sq)) | ((3u - nb) << sq);
            }
        };

        bool open = false;
        int a = 0;
        for (int base = 0; base < nk; base += 64) {
            const int i = base + lane;
            const bool act = i < nk;
            const unsigned long long key = cr_key(cr_kmer(word, nw, act ? i : nk - 1, k), k);
            const unsigned long long m = __ballot(act && !cr_is_solid(f.solid, f.dir, shift, key));
            const int cnt = min(64, nk - base);
            int pos = 0;
            while (pos < cnt) {                        // from one change of the weak bit to the next: wave-uniform
                const unsigned long long rest = (open ? ~m : m) >> pos;
                if (!rest) break;
                const int z = __ffsll((long long) rest) - 1;
                if (pos + z >= cnt) break;
                if (open) { run(a, base + pos + z - 1); open = false; }
                else { a = base + pos + z; open = true; }
                pos += z;
            }
        }
        if (open) run(a, nk - 1);
        if (changed) n_changed++;
    }
    if (lane == 0) {
        atomicAdd(&cnt_sh[CR_RUNS], n_runs); atomicAdd(&cnt_sh[CR_FIXED], n_fixed); atomicAdd(&cnt_sh[CR_AMBIGUOUS], n_amb);
        atomicAdd(&cnt_sh[CR_NO_CANDIDATE], n_none); atomicAdd(&cnt_sh[CR_SKIPPED], n_skip); atomicAdd(&cnt_sh[CR_CHANGED], n_changed);
    }
    __syncthreads();
    if (threadIdx.x < CR_COLS) table[(size_t) blockIdx.x * CR_COLS + threadIdx.x] = cnt_sh[threadIdx.x];
}

unsigned cr_read_blocks(uint64_t R, unsigned cap) { return (unsigned) std::max<uint64_t>(1, std::min<uint64_t>((R + CR_WAVES - 1) / CR_WAVES, cap)); }

}  // namespace

void launch_cr_twin(const CrReads &c, uint32_t *bad, hipStream_t s) {
    hipLaunchKernelGGL(k_cr_twin, dim3(cr_read_blocks(c.R, 4096)), dim3(CR_BLOCK), 0, s, c, bad);
}

int launch_cr_hist(const CrReads &c, uint32_t *table, hipStream_t s) {
    const unsigned g = cr_read_blocks(c.R, CR_HIST_BLOCKS);
    hipLaunchKernelGGL(k_cr_hist, dim3(g), dim3(CR_BLOCK), 0, s, c, table);
    return (int) g;
}

void launch_cr_sum(const uint32_t *table, int rows, int cols, unsigned long long *out, bool accumulate, hipStream_t s) {
    hipLaunchKernelGGL(k_cr_sum, dim3((unsigned) ((cols + CR_BLOCK - 1) / CR_BLOCK)), dim3(CR_BLOCK), 0, s, table, rows, cols, out, accumulate ? 1 : 0);
}

void launch_cr_emit(const CrReads &c, uint32_t bin_lo, uint32_t bin_hi, unsigned long long *keys, uint64_t cap, unsigned long long *cursor, hipStream_t s) {
    hipLaunchKernelGGL(k_cr_emit, dim3(cr_read_blocks(c.R, 2048)), dim3(CR_BLOCK), 0, s, c, bin_lo, bin_hi, keys, cap, cursor);
}

int launch_cr_runs(const unsigned long long *keys, uint64_t n, int32_t solid_min, uint32_t *flags, uint32_t *table, hipStream_t s) {
    const unsigned g = (unsigned) std::max<uint64_t>(1, std::min<uint64_t>((n + CR_BLOCK - 1) / CR_BLOCK, CR_RUNS_BLOCKS));
    hipLaunchKernelGGL(k_cr_runs, dim3(g), dim3(CR_BLOCK), 0, s, keys, n, solid_min, flags, table);
    return (int) g;
}

void launch_cr_append(const unsigned long long *keys, const uint32_t *flags, const uint32_t *pos, uint64_t n, unsigned long long *solid, uint64_t base, uint64_t cap,
                      hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_cr_append, dim3((unsigned) std::min<uint64_t>((n + CR_BLOCK - 1) / CR_BLOCK, 4096)), dim3(CR_BLOCK), 0, s, keys, flags, pos, n, solid, base, cap);
}

void launch_cr_dir(const unsigned long long *solid, uint64_t n_solid, int bits, uint32_t *dir, uint32_t *bad, hipStream_t s) {
    hipLaunchKernelGGL(k_cr_dir, dim3((unsigned) ((n_solid + 1 + CR_BLOCK - 1) / CR_BLOCK)), dim3(CR_BLOCK), 0, s, solid, n_solid, 64 - bits, 1u << bits, dir, bad);
}

int cr_fix_blocks(uint64_t R, int n_cu) { return (int) cr_read_blocks(R, (unsigned) std::max(1, n_cu) * 8u); }

int launch_cr_fix(const CrReads &c, const CrFix &f, int n_cu, uint32_t *table, hipStream_t s) {
    const int g = cr_fix_blocks(c.R, n_cu);
    hipLaunchKernelGGL(k_cr_fix, dim3((unsigned) g), dim3(CR_BLOCK), 0, s, c, f, table);
    return g;
}

}  // namespace alga
