// alga_amd/csrc/final_kernels.hip -- the final contig set on the GPU (include/alga_amd.h: alga_contig_trim_device, alga_final_contigs_device,
// alga_write_final_fasta_device): what the reference does between ContigCreatorSinglePath::getAllContigs and its output FASTA
// (OutputWriterNew::filterContigs, the trim of src/main.cpp:633-725, writeContigsNoFilter).
//
// Integer work and byte movement, and one IEEE double comparison per verdict.
//   k_fc_len_check     lengths >= 0, the longest capped length
//   k_fc_gather        ragged sequences (any base index as their start) -> rows of one stride in the cap form: one lane per output word, two source
//                      words funnel-shifted by begin & 15; the seam at base 501 lies inside word 31 (501 = 31 * 16 + 5)
//   k_fc_rank_keys     sort keys of the rank order (length descending; the stable sort keeps the pair order inside a length)
//   k_fc_init          rank[], SHORT, and ACCEPTED for every pair that is accepted even when both its end reads are marked; the rest is undecided
//   k_fc_round_min     every undecided pair registers its rank at its end reads (64-bit atomicMax on (round, ~rank): no clearing between rounds)
//   k_fc_round_decide  a pair is decidable when each end read is marked by an accepted pair of smaller rank or has no undecided pair of smaller rank
//   k_fc_accept_flags / k_fc_number   ids = exclusive scan of the accepted flags in rank order; new_reads from the final marks; the windows in id order
//   k_fc_apply_trim    begin / len after the trim, TRIMMED_AWAY
//   k_fc_fasta_sizes / k_fc_fasta_write   the records `>contig_id=<id>_length=<len>\n<window>\n`, one wave per record, 16-byte aligned stores
// Only the first and the last path entry of a pair can be shared with another pair (the junction reads of a contig result; a unitig result shares
// nothing), so the marks are kept for end entries alone.  Of an extended result (alga_extend_contigs_device) the junction reads inside a pair are
// shared too: its end entries are its seam list.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "final_kernels.h"
#include "packed_device.h"
#include "text_record.h"

namespace alga {

namespace {

constexpr int FC_BLOCK = 256;
constexpr uint32_t FC_NONE = 0xFFFFFFFFu;

// slot of this lane in a list that the whole wave appends to (every lane of the wave calls it)
__device__ __forceinline__ uint32_t fc_wave_append(bool want, unsigned long long *counter) {
    const unsigned long long m = __ballot(want);
    if (!m) return 0;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long) m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long) __popcll(m));
    base = __shfl(base, leader);
    return (uint32_t) base + (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
}

// OutputWriterNew::filterContig: 100 * ratio < NEW_READS_PER_CONTIG_PERCENTAGE with ratio = (double) new / all
__device__ __forceinline__ bool fc_rejects(int64_t nw, int64_t all, int32_t percent) {
    const double ratio = (double) nw / (double) all;
    return 100.0 * ratio < (double) percent;
}

// 16 bases from base index q of the packed array; words behind `last_word` (the last word the sequence touches) are not read
__device__ __forceinline__ uint32_t fc_fetch16(const uint32_t *__restrict__ words, uint64_t q, uint64_t last_word) {
    const uint64_t w = q >> 4;
    const uint32_t sh = (uint32_t) (q & 15);
    const uint32_t lo = w <= last_word ? words[w] : 0u;
    if (!sh) return lo;
    const uint32_t hi = w + 1 <= last_word ? words[w + 1] : 0u;
    return (uint32_t) ((((uint64_t) hi << 32) | lo) >> (2 * sh));
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_len_check(const int32_t *__restrict__ len, uint64_t n, unsigned long long *__restrict__ counters) {
    unsigned long long bad = 0, mx = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const int32_t L = len[i];
        if (L < 0) bad = FC_BAD_LEN;
        else { const unsigned long long c = (unsigned long long) (L < FC_CAP ? L : FC_CAP); mx = c > mx ? c : mx; }
    }
    bad = wave_max(bad);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&counters[FC_FLAGS], bad);
        if (mx) atomicMax(&counters[FC_MAX_LEN], mx);
    }
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_gather(const uint32_t *__restrict__ words, const unsigned long long *__restrict__ begin,
                                                        const int32_t *__restrict__ len, uint64_t n, int32_t stride, uint32_t *__restrict__ rows,
                                                        int32_t *__restrict__ rlen) {
    const uint64_t total = n * (uint64_t) stride;
    for (uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t i = t / (uint64_t) stride;
        const int32_t wq = (int32_t) (t - i * (uint64_t) stride);
        const int32_t L = len[i], Lc = L < FC_CAP ? L : FC_CAP;
        const int32_t j0 = 16 * wq;
        uint32_t v = 0;
        if (j0 < Lc) {
            const uint64_t b = begin[i], last_word = (b + (uint64_t) L - 1) >> 4;
            if (L <= FC_CAP || j0 + 16 <= FC_CAP_HALF) v = fc_fetch16(words, b + (uint64_t) j0, last_word);
            else {
                const uint64_t tail = b + (uint64_t) (L - FC_CAP);            // capped base j >= 501 is base tail + j of the array
                if (j0 >= FC_CAP_HALF) v = fc_fetch16(words, tail + (uint64_t) j0, last_word);
                else {                                                        // the seam: the first k bases from the head, the rest from the tail
                    const int k = FC_CAP_HALF - j0;
                    v = (fc_fetch16(words, b + (uint64_t) j0, last_word) & ((1u << (2 * k)) - 1u)) |
                        (fc_fetch16(words, tail + (uint64_t) FC_CAP_HALF, last_word) << (2 * k));
                }
            }
            const int32_t valid = Lc - j0;
            if (valid < 16) v &= (1u << (2 * valid)) - 1u;
        }
        rows[t] = v;
        if (wq == 0) rlen[i] = Lc;
    }
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_rank_keys(const int32_t *__restrict__ cons_len, uint32_t P, uint32_t *__restrict__ keys) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < P) keys[k] = 0x7FFFFFFFu - (uint32_t) cons_len[k];
}

// the end entries of pair k, the ones another pair can share: one for a pair of one entry, else the first and the last (they may be the same
// read); of an extended result the entries of its seam list.  -> their number; fc_end_read: the read index of end entry j
__device__ __forceinline__ uint32_t fc_ends(const FcCfg &c, uint32_t k, int64_t &all) {
    all = (int64_t) (c.path_off[k + 1] - c.path_off[k]);
    if (all <= 0) return 0;
    if (c.seam_off) return (uint32_t) (c.seam_off[k + 1] - c.seam_off[k]);
    return all == 1 ? 1u : 2u;
}
__device__ __forceinline__ uint32_t fc_end_read(const FcCfg &c, uint32_t k, uint32_t j) {
    const unsigned long long a = c.path_off[k];
    if (c.seam_off) return (uint32_t) c.path_node[a + (unsigned long long) c.seam_entry[c.seam_off[k] + j]] >> 1;
    return (uint32_t) c.path_node[j ? c.path_off[k + 1] - 1 : a] >> 1;
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_init(FcCfg c, uint32_t *__restrict__ list, unsigned long long *__restrict__ counters) {
    const uint32_t rho = blockIdx.x * blockDim.x + threadIdx.x;
    bool undecided = false;
    uint32_t k = 0;
    if (rho < c.P) {
        k = c.by_rank[rho];
        c.rank[k] = (int32_t) rho;
        const int32_t L = c.cons_len[k];
        uint8_t v = FC_V_UNDECIDED;
        if (L < c.min_length || L == 0) v = FC_V_SHORT;
        else {
            int64_t all;
            const uint32_t ne = fc_ends(c, k, all);
            if (!fc_rejects(all - ne, all, c.percent)) {                      // accepted whatever came before
                v = FC_V_ACCEPTED;
                for (uint32_t j = 0; j < ne; j++) atomicMin(&c.first_acc[fc_end_read(c, k, j)], rho);
            } else undecided = true;
        }
        c.verdict[k] = v;
    }
    const uint32_t at = fc_wave_append(undecided, &counters[FC_UNDECIDED]);
    if (undecided) list[at] = k;
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_round_min(FcCfg c, const uint32_t *__restrict__ list, uint32_t n_in, uint32_t round) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_in) return;
    const uint32_t k = list[t], rho = (uint32_t) c.rank[k];
    int64_t all;
    const uint32_t ne = fc_ends(c, k, all);
    const unsigned long long key = ((unsigned long long) round << 32) | (unsigned long long) (~rho);
    for (uint32_t j = 0; j < ne; j++) atomicMax(&c.min_und[fc_end_read(c, k, j)], key);
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_round_decide(FcCfg c, const uint32_t *__restrict__ list, uint32_t n_in, uint32_t round,
                                                              uint32_t *__restrict__ list_out, unsigned long long *__restrict__ n_out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool again = false;
    uint32_t k = 0;
    if (t < n_in) {
        k = list[t];
        const uint32_t rho = (uint32_t) c.rank[k];
        int64_t all;
        const uint32_t ne = fc_ends(c, k, all);
        int64_t marked = 0;
        bool settled = true;
        for (uint32_t j = 0; j < ne; j++) {
            const uint32_t rd = fc_end_read(c, k, j);
            // an accepted pair of smaller rank is final whenever it is seen; without one the read's state is final once no undecided pair of
            // smaller rank touches it (this pair registered itself: the entry of this round exists)
            const uint32_t fa = __hip_atomic_load(&c.first_acc[rd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (fa < rho) { marked++; continue; }
            const unsigned long long mu = c.min_und[rd];
            const uint32_t lowest = (uint32_t) (mu >> 32) == round ? ~(uint32_t) mu : FC_NONE;
            if (lowest < rho) settled = false;
        }
        if (settled) {
            const bool rej = fc_rejects(all - marked, all, c.percent);
            c.verdict[k] = rej ? FC_V_REJECTED : FC_V_ACCEPTED;
            if (!rej) for (uint32_t j = 0; j < ne; j++) atomicMin(&c.first_acc[fc_end_read(c, k, j)], rho);
        } else again = true;
    }
    const uint32_t at = fc_wave_append(again, n_out);
    if (again) list_out[at] = k;
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_accept_flags(FcCfg c, uint32_t *__restrict__ flags) {
    const uint32_t rho = blockIdx.x * blockDim.x + threadIdx.x;
    if (rho <= c.P) flags[rho] = rho < c.P && c.verdict[c.by_rank[rho]] == FC_V_ACCEPTED;
}

__global__ void __launch_bounds__(FC_BLOCK) k_fc_number(FcCfg c, const uint32_t *__restrict__ ids, unsigned long long *__restrict__ wbegin,
                                                        int32_t *__restrict__ wlen, unsigned long long *__restrict__ counters) {
    const uint32_t rho = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long n_short = 0, n_rej = 0, n_acc = 0, mx = 0;
    if (rho < c.P) {
        const uint32_t k = c.by_rank[rho];
        const uint8_t v = c.verdict[k];
        int32_t nw = -1, id = -1, begin = 0, L = 0;
        if (v != FC_V_SHORT) {
            int64_t all;
            const uint32_t ne = fc_ends(c, k, all);
            int64_t marked = 0;
            for (uint32_t j = 0; j < ne; j++) marked += c.first_acc[fc_end_read(c, k, j)] < rho;
            nw = (int32_t) (all - marked);
        }
        if (v == FC_V_ACCEPTED) {
            id = (int32_t) ids[rho];
            begin = c.cons_trim[k]; L = c.cons_len[k];
            c.order[id] = (int32_t) k;
            wbegin[id] = 16ull * c.word_off[k] + (unsigned long long) begin;
            wlen[id] = L;
            mx = (unsigned long long) (L < FC_CAP ? L : FC_CAP);
            n_acc = 1;
        } else if (v == FC_V_SHORT) n_short = 1;
        else n_rej = 1;
        c.id[k] = id; c.new_reads[k] = nw; c.trim_left[k] = 0; c.begin[k] = begin; c.len[k] = L;
    }
    n_short = wave_sum(n_short); n_rej = wave_sum(n_rej); n_acc = wave_sum(n_acc); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        if (n_short) atomicAdd(&counters[FC_SHORT], n_short);
        if (n_rej) atomicAdd(&counters[FC_REJECTED], n_rej);
        if (n_acc) atomicAdd(&counters[FC_ACCEPTED], n_acc);
        if (mx) atomicMax(&counters[FC_MAX_LEN], mx);
    }
}

// src/main.cpp:700-712 with trimRight = 0: the contig keeps s.substr(trimLeft) when trimLeft + 10 < |s|
__global__ void __launch_bounds__(FC_BLOCK) k_fc_apply_trim(FcCfg c, const int32_t *__restrict__ trim_by_id, uint32_t n_accepted,
                                                            unsigned long long *__restrict__ counters) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long away = 0;
    if (j < n_accepted) {
        const uint32_t k = (uint32_t) c.order[j];
        const int32_t t = trim_by_id[j], L = c.len[k];
        c.trim_left[k] = t;
        if (t + 10 < L) { c.begin[k] += t; c.len[k] = L - t; }
        else { c.verdict[k] = FC_V_TRIMMED_AWAY; c.begin[k] = 0; c.len[k] = 0; away = 1; }
    }
    away = wave_sum(away);
    if ((threadIdx.x & 63) == 0 && away) atomicAdd(&counters[FC_TRIMMED_AWAY], away);
}

// ---- FASTA ---------------------------------------------------------------------------------------------------------------------
// `>contig_id=<id>_length=<len>\n<window>\n` of the accepted pair of id j
struct FcRecord : FastaRecord<PackedSeq> {
    __device__ __forceinline__ bool set(const FcFasta &f, uint64_t j) {
        const uint32_t k = (uint32_t) f.order[j];
        if (f.verdict[k] != FC_V_ACCEPTED) return false;
        contig_head(j, (uint32_t) f.len[k]); seal();
        seq.row = f.words + f.word_off[k]; seq.q0 = (uint32_t) f.begin[k];
        return true;
    }
};

__global__ void __launch_bounds__(FC_BLOCK) k_fc_fasta_sizes(FcFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<FcRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(FC_BLOCK) k_fc_fasta_write(FcFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1,
                                                             char *__restrict__ buf) {
    text_write_body<FcRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_fc_len_check(const int32_t *len, uint64_t n, unsigned long long *counters, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_fc_len_check, dim3(stage_grid(n, FC_BLOCK, 4096)), dim3(FC_BLOCK), 0, s, len, n, counters);
}

void launch_fc_gather(const uint32_t *words, const unsigned long long *begin, const int32_t *len, uint64_t n, int32_t stride, uint32_t *rows, int32_t *rlen,
                      hipStream_t s) {
    if (n && stride > 0) hipLaunchKernelGGL(k_fc_gather, dim3(stage_grid(n * (uint64_t) stride, FC_BLOCK, 1u << 20)), dim3(FC_BLOCK), 0, s, words, begin, len, n, stride, rows, rlen);
}

void launch_fc_rank_keys(const int32_t *cons_len, uint32_t P, uint32_t *keys, hipStream_t s) {
    if (P) hipLaunchKernelGGL(k_fc_rank_keys, dim3((P + FC_BLOCK - 1) / FC_BLOCK), dim3(FC_BLOCK), 0, s, cons_len, P, keys);
}

void launch_fc_init(const FcCfg &c, uint32_t *list, unsigned long long *counters, hipStream_t s) {
    if (c.P) hipLaunchKernelGGL(k_fc_init, dim3((c.P + FC_BLOCK - 1) / FC_BLOCK), dim3(FC_BLOCK), 0, s, c, list, counters);
}

void launch_fc_round(const FcCfg &c, const uint32_t *list_in, uint32_t n_in, uint32_t round, uint32_t *list_out, unsigned long long *n_out, hipStream_t s) {
    if (!n_in) return;
    const dim3 grid((n_in + FC_BLOCK - 1) / FC_BLOCK);
    hipLaunchKernelGGL(k_fc_round_min, grid, dim3(FC_BLOCK), 0, s, c, list_in, n_in, round);
    hipLaunchKernelGGL(k_fc_round_decide, grid, dim3(FC_BLOCK), 0, s, c, list_in, n_in, round, list_out, n_out);
}

void launch_fc_accept_flags(const FcCfg &c, uint32_t *flags, hipStream_t s) {
    hipLaunchKernelGGL(k_fc_accept_flags, dim3((c.P + 1 + FC_BLOCK - 1) / FC_BLOCK), dim3(FC_BLOCK), 0, s, c, flags);
}

void launch_fc_number(const FcCfg &c, const uint32_t *ids, unsigned long long *wbegin, int32_t *wlen, unsigned long long *counters, hipStream_t s) {
    if (c.P) hipLaunchKernelGGL(k_fc_number, dim3((c.P + FC_BLOCK - 1) / FC_BLOCK), dim3(FC_BLOCK), 0, s, c, ids, wbegin, wlen, counters);
}

void launch_fc_apply_trim(const FcCfg &c, const int32_t *trim_by_id, uint32_t n_accepted, unsigned long long *counters, hipStream_t s) {
    if (n_accepted) hipLaunchKernelGGL(k_fc_apply_trim, dim3((n_accepted + FC_BLOCK - 1) / FC_BLOCK), dim3(FC_BLOCK), 0, s, c, trim_by_id, n_accepted, counters);
}

void launch_fc_fasta_sizes(const FcFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_fc_fasta_sizes, dim3(text_sizes_blocks(f.n, FC_BLOCK)), dim3(FC_BLOCK), 0, s, f, sizes, counters);
}

void launch_fc_fasta_write(const FcFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_fc_fasta_write, dim3(text_write_blocks(i0, i1, FC_BLOCK / 64)), dim3(FC_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
