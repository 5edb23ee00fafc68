// alga_amd/csrc/break_kernels.hip -- contigs broken where no proper pair spans them (include/alga_amd.h: alga_break_placed_device; the
// definition is the comment there, host side in engine_break.hip).
//
// Integer work only, wave-64, no LDS, nothing depends on thread order: the difference array takes 32-bit integer atomics, the counters a
// wave sum and one atomic per wave.
//   k_br_check        n_columns == col_off[T], pair_off as the placement checks it, every UNIQUE read as the polish checks a voter -> the refusal flags
//   k_br_pairs        one thread per read: the judge of a proper pair does +1 at the first column the pair spans and -1 behind the last
//   (span)            launch_exclusive_scan over the columns + 1 differences: entry g + 1 is the span of column g
//   k_br_flags        one thread per column: candidate, weak, "a run starts here", "a run ends here", whether the neighbour that closes the
//                     run on that side exists; a wave whose columns lie in one target takes the target once, else every lane bisects
//   (runs)            the scan of the starts numbers the runs: the end at g belongs to run scan[g] + start[g] - 1 (starts and ends alternate)
//   k_br_runs         first and last column of every run, scattered by the lanes that hold a start or an end
//   k_br_closed       closed[i] = both neighbours exist; their count
//   k_br_cuts         every closed run at the place the scan of closed[] gives: the cut column, the run, t_cuts[target]++
//   k_br_pieces       T + n_cuts items: a target start finds the cuts before it, a cut the targets up to it, by bisection over the other list
//   k_br_copy         the column array into the result's own copy
//   k_br_fasta_sizes / k_br_fasta_write   one record per piece with a length, one wave per record, a lane a byte
// Block 256 and the grid caps are picked, not tuned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "break_kernels.h"
#include "packed_device.h"
#include "text_record.h"

namespace alga {

namespace {

constexpr int BR_BLOCK = 256, BR_WAVES = BR_BLOCK / 64;
constexpr uint8_t BR_ST_UNIQUE = 2, BR_ST_MINUS = 4;                    // ALGA_PLACE_UNIQUE, ALGA_PLACE_MINUS

__device__ __forceinline__ uint32_t br_wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t) __shfl_xor((int) v, o);
    return v;
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_check(BrReads r, BrTargets t, unsigned long long *__restrict__ counters) {
    uint32_t bad = 0;
    const uint64_t n = 2 * r.R, step = (uint64_t) gridDim.x * BR_BLOCK;
    // every column array of the stage has the caller's `columns`: it has to be the placement's
    if (blockIdx.x == 0 && threadIdx.x == 0 && (uint64_t) t.col_off[t.T] != t.columns) bad |= BR_BAD_COLUMNS;
    if (r.pair_off)
        for (uint64_t v = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; v < n; v += step) {
            const uint8_t po = r.pair_off[v];
            if (po > 2 || po != r.pair_off[v ^ 1]) bad |= BR_BAD_PAIR;
            else if (po == 1 && (v + 2 >= n || r.pair_off[v + 2] != 2)) bad |= BR_BAD_PAIR;
            else if (po == 2 && (v < 2 || r.pair_off[v - 2] != 1)) bad |= BR_BAD_PAIR;
        }
    for (uint64_t i = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; i < r.R; i += step) {
        if (!(r.state[i] & BR_ST_UNIQUE)) continue;
        const int32_t L = r.len[2 * i + 1];
        if (L < 1 || (int64_t) L > 16ll * r.stride) { bad |= BR_BAD_LEN; continue; }
        const int32_t tt = r.target[i], p = r.pos[i];
        if (tt < 0 || (uint32_t) tt >= t.T || p < 0 || (int64_t) p + L > (int64_t) t.col_off[tt + 1] - (int64_t) t.col_off[tt]) bad |= BR_BAD_PLACE;
    }
    bad = br_wave_or(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(&counters[BR_BAD], (unsigned long long) bad);
}

// (after the check: columns is col_off[T], every UNIQUE read lies inside its target, a judge's mate is read r + 1 < R; so a + inset >= 0 and b + lb - inset <= the
// target's length, and both writes land in the columns + 1 entries)
__global__ void __launch_bounds__(BR_BLOCK) k_br_pairs(BrReads r, BrTargets t, int32_t max_insert, int32_t inset, uint32_t *__restrict__ diff,
                                                       unsigned long long *__restrict__ counters) {
    unsigned long long n_proper = 0, n_span = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * BR_BLOCK) {
        if (r.pair_off[2 * i + 1] != 1) continue;                              // the mate with the smaller index judges: its mate is read i + 1
        const uint64_t j = i + 1;
        const uint8_t s1 = r.state[i], s2 = r.state[j];
        if (!(s1 & BR_ST_UNIQUE) || !(s2 & BR_ST_UNIQUE)) continue;
        const int32_t tt = r.target[i];
        if (tt != r.target[j] || (s1 & BR_ST_MINUS) == (s2 & BR_ST_MINUS)) continue;
        const uint64_t rp = (s1 & BR_ST_MINUS) ? j : i, rm = (s1 & BR_ST_MINUS) ? i : j;
        const long long a = r.pos[rp], la = r.len[2 * rp + 1], b = r.pos[rm], lb = r.len[2 * rm + 1];
        const long long ins = b + lb - a;
        if (!(a <= b && a + la <= b + lb && ins <= (long long) max_insert)) continue;
        n_proper++;
        const long long lo = a + inset, hi = b + lb - inset;                   // the pair spans lo .. hi - 1
        if (hi <= lo) continue;
        n_span++;
        const uint32_t c0 = t.col_off[tt];
        atomicAdd(&diff[c0 + (uint32_t) lo], 1u);
        atomicAdd(&diff[c0 + (uint32_t) hi], 0xFFFFFFFFu);
    }
    n_proper = wave_sum(n_proper); n_span = wave_sum(n_span);
    if ((threadIdx.x & 63) == 0 && n_proper) {
        atomicAdd(&counters[BR_PROPER], n_proper);
        if (n_span) atomicAdd(&counters[BR_SPANNING], n_span);
    }
}

// whole waves stride: lane l of a pass holds column g0 + l
__global__ void __launch_bounds__(BR_BLOCK) k_br_flags(BrTargets t, const uint32_t *__restrict__ span, uint32_t min_span, uint32_t margin, uint32_t *__restrict__ starts,
                                                       uint8_t *__restrict__ marks, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    unsigned long long n_cand = 0, n_weak = 0, n_runs = 0, mx = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) starts[t.columns] = 0;             // the place of the scan's total
    for (uint64_t g0 = ((uint64_t) blockIdx.x * BR_BLOCK + (threadIdx.x & ~63u)); g0 < t.columns; g0 += (uint64_t) gridDim.x * BR_BLOCK) {
        const uint64_t g = g0 + (uint64_t) lane;
        if (g >= t.columns) continue;
        const uint64_t glast = g0 + 63 < t.columns ? g0 + 63 : t.columns - 1;
        uint32_t tt = item_of(t.col_off, t.T, (uint32_t) g0);               // the same in all lanes
        if ((uint64_t) t.col_off[tt + 1] <= glast) tt = item_of(t.col_off, t.T, (uint32_t) g);   // the wave's columns lie in several targets
        const uint32_t c0 = t.col_off[tt];
        const long long j = (long long) g - c0, hi = (long long) t.col_off[tt + 1] - c0 - (long long) margin;   // candidates: margin <= j < hi
        const uint32_t sp = span[g];
        mx = sp > mx ? sp : mx;
        uint32_t st = 0;
        uint8_t m = 0;
        if (j >= (long long) margin && j < hi) {
            n_cand++;
            if (sp < min_span) {
                n_weak++;
                const bool left = j - 1 >= (long long) margin, right = j + 1 < hi;     // the neighbours are candidates of this target
                if (!left || span[g - 1] >= min_span) { st = 1; m |= BR_M_START | (left ? BR_M_LEFT : 0); n_runs++; }
                if (!right || span[g + 1] >= min_span) m |= BR_M_END | (right ? BR_M_RIGHT : 0);
            }
        }
        starts[g] = st; marks[g] = m;
    }
    n_cand = wave_sum(n_cand); n_weak = wave_sum(n_weak); n_runs = wave_sum(n_runs); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        if (n_cand) atomicAdd(&counters[BR_CANDIDATES], n_cand);
        if (n_weak) atomicAdd(&counters[BR_WEAK], n_weak);
        if (n_runs) atomicAdd(&counters[BR_RUNS], n_runs);
        if (mx) atomicMax(&counters[BR_MAX_SPAN], mx);
    }
}

// (starts and ends alternate, a start first: the end at g closes the run of the last start at or before g)
__global__ void __launch_bounds__(BR_BLOCK) k_br_runs(BrTargets t, const uint32_t *__restrict__ run_pos, const uint8_t *__restrict__ marks, uint64_t n_runs,
                                                      uint32_t *__restrict__ run_first, uint32_t *__restrict__ run_last) {
    for (uint64_t g = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; g < t.columns; g += (uint64_t) gridDim.x * BR_BLOCK) {
        const uint8_t m = marks[g];
        if (!(m & (BR_M_START | BR_M_END))) continue;
        const uint32_t id = run_pos[g] - ((m & BR_M_START) ? 0u : 1u);          // a start: the starts before g; an end alone: one less
        if (id >= n_runs) continue;                                             // (cannot be: the scan counted the starts)
        if (m & BR_M_START) run_first[id] = (uint32_t) g;
        if (m & BR_M_END) run_last[id] = (uint32_t) g;
    }
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_closed(const uint32_t *__restrict__ run_first, const uint32_t *__restrict__ run_last, const uint8_t *__restrict__ marks,
                                                        uint64_t n_runs, uint32_t *__restrict__ closed, unsigned long long *__restrict__ counters) {
    unsigned long long n = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; i <= n_runs; i += (uint64_t) gridDim.x * BR_BLOCK) {
        uint32_t c = 0;
        if (i < n_runs) c = (marks[run_first[i]] & BR_M_LEFT) && (marks[run_last[i]] & BR_M_RIGHT) ? 1u : 0u;
        closed[i] = c; n += c;                                                  // entry n_runs: the place of the scan's total
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&counters[BR_CUTS], n);
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_cuts(BrTargets t, const uint32_t *__restrict__ run_first, const uint32_t *__restrict__ run_last,
                                                      const uint32_t *__restrict__ closed, const uint32_t *__restrict__ cut_pos, uint64_t n_runs, BrCuts c) {
    for (uint64_t i = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; i < n_runs; i += (uint64_t) gridDim.x * BR_BLOCK) {
        if (!closed[i]) continue;
        const uint32_t at = cut_pos[i];
        if (at >= c.n) continue;                                                // (cannot be: the count came from closed[])
        const uint32_t s = run_first[i], e = run_last[i];
        c.cols[at] = (uint32_t) (((uint64_t) s + e + 1) >> 1); c.first[at] = s; c.last[at] = e;
        atomicAdd(&c.t_cuts[item_of(t.col_off, t.T, s)], 1u);
    }
}

// item x < T: the start of target x; item T + i: cut i.  The pieces in column order: target t starts piece t + (the cuts before col_off[t]),
// cut i starts piece i + (the targets that begin at or before it)
__global__ void __launch_bounds__(BR_BLOCK) k_br_pieces(BrTargets t, BrCuts c, BrPieces p, unsigned long long *__restrict__ counters) {
    unsigned long long longest = 0, n_tcut = 0;
    const uint64_t items = (uint64_t) t.T + c.n;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.piece_off[items] = (uint32_t) t.columns;
    for (uint64_t x = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; x < items; x += (uint64_t) gridDim.x * BR_BLOCK) {
        uint32_t tt, col, next_cut;                                            // its target, its first column, the cut behind it
        uint64_t id;
        if (x < t.T) {
            tt = (uint32_t) x; col = t.col_off[tt];
            uint64_t lo = 0, hi = c.n;                                          // the first cut at or behind col (a cut is never a target's first column)
            while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (c.cols[mid] < col) lo = mid + 1; else hi = mid; }
            id = x + lo; next_cut = (uint32_t) lo;
            n_tcut += lo < c.n && c.cols[lo] < t.col_off[tt + 1];
        } else {
            const uint64_t i = x - t.T;
            col = c.cols[i]; tt = item_of(t.col_off, t.T, col);
            id = i + (uint64_t) tt + 1; next_cut = (uint32_t) (i + 1);
        }
        const uint32_t end_t = t.col_off[tt + 1];
        const uint32_t end = next_cut < c.n && c.cols[next_cut] < end_t ? c.cols[next_cut] : end_t;
        const uint32_t len = end - col;
        p.piece_off[id] = col; p.begin[id] = col; p.len[id] = (int32_t) len; p.piece_target[id] = (int32_t) tt; p.piece_start[id] = col - t.col_off[tt];
        longest = len > longest ? len : longest;
    }
    longest = wave_max(longest); n_tcut = wave_sum(n_tcut);
    if ((threadIdx.x & 63) == 0) {
        if (longest) atomicMax(&counters[BR_LONGEST], longest);
        if (n_tcut) atomicAdd(&counters[BR_TARGETS_CUT], n_tcut);
    }
}

__global__ void __launch_bounds__(BR_BLOCK) k_br_copy(const uint32_t *__restrict__ src, uint64_t columns, uint64_t n_words, uint32_t *__restrict__ dst) {
    for (uint64_t w = (uint64_t) blockIdx.x * BR_BLOCK + threadIdx.x; w < n_words; w += (uint64_t) gridDim.x * BR_BLOCK) {
        const uint64_t g0 = w << 4;
        uint32_t v = 0;
        if (g0 < columns) {
            v = src[w];
            if (columns - g0 < 16) v &= (1u << (2 * (uint32_t) (columns - g0))) - 1u;
        }
        dst[w] = v;
    }
}

// ---- FASTA of the pieces ---------------------------------------------------------------------------------------------------------------
// `>contig_id=<j>_length=<len>_from=<t>_start=<s>\n<piece>\n`
struct BrRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const BrFasta &f, uint64_t j) {
        const int32_t len = f.len[j];
        if (len <= 0) return false;
        contig_head(j, (uint32_t) len);
        h.f[2] = text_field("_from=", (uint64_t) f.piece_target[j]); h.f[3] = text_field("_start=", f.piece_start[j]); seal();
        seq.row = f.words; seq.q0 = f.piece_off[j];
        return true;
    }
};

__global__ void __launch_bounds__(BR_BLOCK) k_br_fasta_sizes(BrFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<BrRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(BR_BLOCK) k_br_fasta_write(BrFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<BrRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_br_check(const BrReads &r, const BrTargets &t, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_br_check, dim3(stage_grid(2 * r.R, BR_BLOCK, 4096)), dim3(BR_BLOCK), 0, s, r, t, counters);
}

void launch_br_pairs(const BrReads &r, const BrTargets &t, int32_t max_insert, int32_t inset, uint32_t *diff, unsigned long long *counters, hipStream_t s) {
    if (r.R && r.pair_off && t.T) hipLaunchKernelGGL(k_br_pairs, dim3(stage_grid(r.R, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, r, t, max_insert, inset, diff, counters);
}

void launch_br_flags(const BrTargets &t, const uint32_t *span, uint32_t min_span, uint32_t margin, uint32_t *starts, uint8_t *marks, unsigned long long *counters,
                     hipStream_t s) {
    if (t.columns) hipLaunchKernelGGL(k_br_flags, dim3(stage_grid(t.columns, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, t, span, min_span, margin, starts, marks, counters);
}

void launch_br_runs(const BrTargets &t, const uint32_t *run_pos, const uint8_t *marks, uint64_t n_runs, uint32_t *run_first, uint32_t *run_last, hipStream_t s) {
    if (t.columns && n_runs) hipLaunchKernelGGL(k_br_runs, dim3(stage_grid(t.columns, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, t, run_pos, marks, n_runs, run_first, run_last);
}

void launch_br_closed(const uint32_t *run_first, const uint32_t *run_last, const uint8_t *marks, uint64_t n_runs, uint32_t *closed, unsigned long long *counters,
                      hipStream_t s) {
    if (n_runs) hipLaunchKernelGGL(k_br_closed, dim3(stage_grid(n_runs + 1, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, run_first, run_last, marks, n_runs, closed, counters);
}

void launch_br_cuts(const BrTargets &t, const uint32_t *run_first, const uint32_t *run_last, const uint32_t *closed, const uint32_t *cut_pos, uint64_t n_runs, const BrCuts &c,
                    hipStream_t s) {
    if (n_runs && c.n) hipLaunchKernelGGL(k_br_cuts, dim3(stage_grid(n_runs, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, t, run_first, run_last, closed, cut_pos, n_runs, c);
}

void launch_br_pieces(const BrTargets &t, const BrCuts &c, const BrPieces &p, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_br_pieces, dim3(stage_grid((uint64_t) t.T + c.n + 1, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, t, c, p, counters);
}

void launch_br_copy(const uint32_t *src, uint64_t columns, uint32_t *dst, hipStream_t s) {
    const uint64_t n_words = ((columns + 15) >> 4) + 2;
    hipLaunchKernelGGL(k_br_copy, dim3(stage_grid(n_words, BR_BLOCK, 8192)), dim3(BR_BLOCK), 0, s, src, columns, n_words, dst);
}

void launch_br_fasta_sizes(const BrFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_br_fasta_sizes, dim3(text_sizes_blocks(f.n, BR_BLOCK)), dim3(BR_BLOCK), 0, s, f, sizes, counters);
}

void launch_br_fasta_write(const BrFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_br_fasta_write, dim3(text_write_blocks(i0, i1, BR_WAVES)), dim3(BR_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
