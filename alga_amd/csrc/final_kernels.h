// alga_amd/csrc/final_kernels.h -- launchers of final_kernels.hip: the final contig set (include/alga_amd.h: alga_contig_trim_device,
// alga_final_contigs_device, alga_write_final_fasta_device)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alga {

// overlap lengths stop at 501: a sequence longer than 2 * 501 nt enters the trim build as its first 501 nt followed by its last 501 nt
constexpr int32_t FC_CAP_HALF = 501, FC_CAP = 2 * FC_CAP_HALF;

// counters[] (unsigned long long) the kernels fill
enum { FC_FLAGS = 0, FC_MAX_LEN, FC_SHORT, FC_REJECTED, FC_ACCEPTED, FC_TRIMMED_AWAY, FC_UNDECIDED, FC_RECORDS, FC_MAX_LINE, FC_COUNTERS };
// bits of counters[FC_FLAGS]
enum { FC_BAD_LEN = 1 };
// d_verdict (the values of include/alga_amd.h: ALGA_FINAL_*); FC_V_UNDECIDED lives between the rounds only
enum { FC_V_SHORT = 0, FC_V_REJECTED = 1, FC_V_ACCEPTED = 2, FC_V_TRIMMED_AWAY = 3, FC_V_UNDECIDED = 255 };

// what the filter kernels read and write: the unitig / contig result, the windows of its consensus, the per-pair arrays of the result
struct FcCfg {
    const int32_t *path_node;
    const unsigned long long *path_off, *word_off;
    const int32_t *cons_len, *cons_trim;
    uint32_t P;
    int32_t min_length, percent;
    const uint32_t *by_rank;          // pair of every rank (the sort's values)
    uint8_t *verdict;
    int32_t *rank, *id, *new_reads, *trim_left, *begin, *len, *order;
    uint32_t *first_acc;              // per read index: the smallest rank of an accepted pair that has it as an end entry (0xFFFFFFFF: none)
    unsigned long long *min_und;      // per read index: (round << 32) | ~(smallest rank of an undecided pair that has it as an end entry)
    const unsigned long long *seam_off;   // an extended result: the end entries of pair k are its seam list seam_entry[seam_off[k] .. seam_off[k+1])
    const int32_t *seam_entry;            // (indices into the pair's path entries); nullptr: the first and the last path entry
};

// lengths >= 0 (FC_BAD_LEN), the longest capped length into counters[FC_MAX_LEN]
void launch_fc_len_check(const int32_t *len, uint64_t n, unsigned long long *counters, hipStream_t s);
// rows[i] = sequence i in its cap form at `stride` words a row, tail bits zero; rlen[i] = its capped length
void launch_fc_gather(const uint32_t *words, const unsigned long long *begin, const int32_t *len, uint64_t n, int32_t stride, uint32_t *rows, int32_t *rlen,
                      hipStream_t s);
// keys[k] = 2^31 - 1 - cons_len[k]: ascending keys, stable over k, are the rank order
void launch_fc_rank_keys(const int32_t *cons_len, uint32_t P, uint32_t *keys, hipStream_t s);
// rank[], the verdicts that need no round (short; accepted whatever came before), the undecided pairs into list (their number: counters[FC_UNDECIDED])
void launch_fc_init(const FcCfg &c, uint32_t *list, unsigned long long *counters, hipStream_t s);
// one round: the undecided pairs of list_in register at their end reads, then every decidable one is decided; the rest goes to list_out (*n_out)
void launch_fc_round(const FcCfg &c, const uint32_t *list_in, uint32_t n_in, uint32_t round, uint32_t *list_out, unsigned long long *n_out, hipStream_t s);
// flags[r] = the pair of rank r is accepted (flags[P] = 0: an exclusive scan over P + 1 entries ends in the number of accepted pairs)
void launch_fc_accept_flags(const FcCfg &c, uint32_t *flags, hipStream_t s);
// id / order / new_reads / begin / len / trim_left of every pair, the windows of the accepted pairs in id order, the counts per verdict,
// counters[FC_MAX_LEN]
void launch_fc_number(const FcCfg &c, const uint32_t *ids, unsigned long long *wbegin, int32_t *wlen, unsigned long long *counters, hipStream_t s);
// the trim of every accepted pair (by id) applied: begin / len / trim_left, or TRIMMED_AWAY
void launch_fc_apply_trim(const FcCfg &c, const int32_t *trim_by_id, uint32_t n_accepted, unsigned long long *counters, hipStream_t s);

// the FASTA of the result: record j is the accepted pair of id j
struct FcFasta {
    const uint32_t *words;            // the untrimmed consensus, laid out by word_off
    const unsigned long long *word_off;
    const uint8_t *verdict;
    const int32_t *order, *begin, *len;
    uint64_t n;                       // ids: n_accepted
};
void launch_fc_fasta_sizes(const FcFasta &f, uint32_t *sizes, unsigned long long *counters /* GFA_SEGMENTS / GFA_MAX_LINE of gfa_kernels.h */, hipStream_t s);
void launch_fc_fasta_write(const FcFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s);

}  // namespace alga
