// alga_amd/csrc/correct_kernels.h -- launchers of correct_kernels.hip: read error correction by the k-mer spectrum (include/alga_amd.h:
// alga_correct_reads_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

// the occurrences are histogrammed (and sliced) by the top CR_BIN_BITS bits of the mixed key
constexpr int CR_BIN_BITS = 12, CR_BINS = 1 << CR_BIN_BITS;
// columns of a block's row of the histogram table: the bins, then the number of forward reads with len >= k
constexpr int CR_HIST_READS = CR_BINS, CR_HIST_COLS = CR_BINS + 8;
// columns of a block's row of k_cr_fix's table (and of its sums)
enum { CR_RUNS = 0, CR_FIXED, CR_AMBIGUOUS, CR_NO_CANDIDATE, CR_SKIPPED, CR_CHANGED, CR_COLS = 8 };
// grids of the kernels that leave one table row per block
constexpr int CR_HIST_BLOCKS = 1024, CR_RUNS_BLOCKS = 1024;
// directory of the solid keys: bits of the mixed key it is made on
constexpr int CR_DIR_BITS_MAX = 28;

// the node arrays in the parser's layout: row 2r + 1 = read r, row 2r = its reverse complement
struct CrReads {
    uint32_t *rows;
    int32_t stride;
    const int32_t *len;
    uint64_t R;                       // reads (pairs of nodes)
    int32_t k;
};

// *bad = 1 where len[2r] != len[2r + 1], blocks_of(len) > stride, or row 2r is not the reverse complement of row 2r + 1 (tail bits zero)
void launch_cr_twin(const CrReads &c, uint32_t *bad, hipStream_t s);
// table[block][CR_HIST_COLS]: occurrences per bin of the k-mers of the block's reads, its reads with len >= k; returns the blocks
int  launch_cr_hist(const CrReads &c, uint32_t *table, hipStream_t s);
// out[col] (+)= sum over the rows of table[rows][cols]: one thread per column, no atomics
void launch_cr_sum(const uint32_t *table, int rows, int cols, unsigned long long *out, bool accumulate, hipStream_t s);
// the mixed keys of every occurrence with bin in [bin_lo, bin_hi), block-compacted (one atomicAdd on *cursor per block); writes below cap only
void launch_cr_emit(const CrReads &c, uint32_t bin_lo, uint32_t bin_hi, unsigned long long *keys, uint64_t cap, unsigned long long *cursor, hipStream_t s);
// over sorted keys: flags[j] = j is the head of a run of >= solid_min equal keys; table[block][0] = run heads of the block; returns the blocks
int  launch_cr_runs(const unsigned long long *keys, uint64_t n, int32_t solid_min, uint32_t *flags, uint32_t *table, hipStream_t s);
// solid[base + pos[j]] = keys[j] where flags[j] (below cap only)
void launch_cr_append(const unsigned long long *keys, const uint32_t *flags, const uint32_t *pos, uint64_t n, unsigned long long *solid, uint64_t base, uint64_t cap,
                      hipStream_t s);
// dir[b] = first solid key with (key >> (64 - bits)) >= b, b = 0 .. 2^bits; *bad = 1 where the keys do not ascend strictly
void launch_cr_dir(const unsigned long long *solid, uint64_t n_solid, int bits, uint32_t *dir, uint32_t *bad, hipStream_t s);
// the correction itself, in place; table[block][CR_COLS]; returns the blocks
struct CrFix {
    const unsigned long long *solid;
    const uint32_t *dir;
    int32_t dir_bits, min_run;
};
int  launch_cr_fix(const CrReads &c, const CrFix &f, int n_cu, uint32_t *table, hipStream_t s);
int  cr_fix_blocks(uint64_t R, int n_cu);

}  // namespace alga
