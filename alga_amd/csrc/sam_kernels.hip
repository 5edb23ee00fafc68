// alga_amd/csrc/sam_kernels.hip -- the pairs judged over both placement passes and every read as a SAM record (include/alga_amd.h:
// alga_judge_pairs_device, alga_write_sam_device; the definition is the comment there, host side in engine_sam.hip).
//
// Both kernels start from the COMBINED VIEW of a read (sam_view): the Hamming placement where it placed the read, else the gapped one.
//   k_sam_pair_check   the pair_off rules of the placement, once more on the device (this stage may be given another pair_off than the placement)
//   k_sam_judge        one thread per read in a grid-stride loop: its own view and its mate's, FLAG and TLEN of its record; the mate with the
//                      smaller index counts the pair and adds to the histogram (64-bit integer atomics).  The counters are summed per wave,
//                      one atomic per wave and counter, as k_pl_pairs does
//   k_sam_sizes / k_sam_write   the records through text_record.h: SamRecord is `head, RNAME, POS and MAPQ, CIGAR, RNEXT, PNEXT and TLEN, SEQ,
//                      QUAL and tags`.  The names come from FastaRecord's header builders, so the SAM and the FASTA cannot drift apart.  The
//                      sizes pass also leaves the writer's refusals in counters[GFA_FLAGS]
// Block sizes are picked, not tuned: four waves a block as in the other writers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sam_kernels.h"
#include "packed_device.h"
#include "text_record.h"

namespace alga {

namespace {

constexpr int SAM_BLOCK = 256, SAM_WAVES = SAM_BLOCK / 64;
constexpr uint8_t SAM_ST_PLACED = 1, SAM_ST_UNIQUE = 2, SAM_ST_MINUS = 4;   // ALGA_PLACE_* and ALGA_GAPPED_* of include/alga_amd.h: the same three bits
constexpr uint32_t SAM_OP_I = 1, SAM_OP_D = 2;                             // ALGA_CIGAR_*
constexpr uint32_t SAM_F_PAIRED = 0x1, SAM_F_PROPER = 0x2, SAM_F_UNPLACED = 0x4, SAM_F_MATE_UNPLACED = 0x8, SAM_F_MINUS = 0x10, SAM_F_MATE_MINUS = 0x20,
                   SAM_F_FIRST = 0x40, SAM_F_LAST = 0x80;

// rule 1: the combined view of a read
struct SamView {
    int32_t L, target, pos, end, nm;
    bool live, placed, gapped, minus, unique;
};

__device__ __forceinline__ SamView sam_view(const SamReads &v, uint64_t r) {
    SamView o;
    o.L = v.len[2 * r + 1];
    o.live = o.L >= 1;
    o.target = -1; o.pos = -1; o.end = -1; o.nm = 0;
    o.placed = o.gapped = o.minus = o.unique = false;
    if (!o.live) return o;
    const uint8_t hs = v.h_state[r];
    if (hs & SAM_ST_PLACED) {
        o.placed = true; o.target = v.h_target[r]; o.pos = v.h_pos[r]; o.end = o.pos + o.L; o.nm = v.h_mm[r];
        o.minus = hs & SAM_ST_MINUS; o.unique = hs & SAM_ST_UNIQUE;
    } else if (v.g_state) {
        const uint8_t gs = v.g_state[r];
        if (gs & SAM_ST_PLACED) {
            o.placed = o.gapped = true; o.target = v.g_target[r]; o.pos = v.g_pos[r]; o.end = v.g_end[r]; o.nm = v.g_edits[r];
            o.minus = gs & SAM_ST_MINUS; o.unique = gs & SAM_ST_UNIQUE;
        }
    }
    return o;
}

__global__ void __launch_bounds__(SAM_BLOCK) k_sam_pair_check(const uint8_t *__restrict__ pair_off, uint64_t n, unsigned long long *__restrict__ counters) {
    bool bad = false;
    for (uint64_t v = (uint64_t) blockIdx.x * SAM_BLOCK + threadIdx.x; v < n; v += (uint64_t) gridDim.x * SAM_BLOCK) {
        const uint8_t po = pair_off[v];
        if (po > 2 || po != pair_off[v ^ 1]) bad = true;
        else if (po == 1 && (v + 2 >= n || pair_off[v + 2] != 2)) bad = true;
        else if (po == 2 && (v < 2 || pair_off[v - 2] != 1)) bad = true;
    }
    if (bad) counters[SAM_BAD_PAIR] = 1ull;
}

__global__ void __launch_bounds__(SAM_BLOCK) k_sam_judge(SamReads v, int32_t max_insert, uint16_t *__restrict__ flag, int32_t *__restrict__ tlen,
                                                         unsigned long long *__restrict__ hist, unsigned long long *__restrict__ counters) {
    unsigned long long n_live = 0, n_h = 0, n_g = 0, n_un = 0, n_pairs = 0, n_proper = 0, n_improper = 0, n_split = 0, n_nu = 0, n_wg = 0, n_pg = 0, sum = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * SAM_BLOCK + threadIdx.x; r < v.R; r += (uint64_t) gridDim.x * SAM_BLOCK) {
        const SamView me = sam_view(v, r);
        uint32_t fl = 0;
        int32_t tl = 0;
        if (me.live) {
            n_live++;
            if (!me.placed) { n_un++; fl |= SAM_F_UNPLACED; }
            else { if (me.gapped) n_g++; else n_h++; if (me.minus) fl |= SAM_F_MINUS; }
            const uint8_t po = v.pair_off ? v.pair_off[2 * r + 1] : (uint8_t) 0;
            if (po == 1 || po == 2) {                                          // (checked: the mate is in range)
                const SamView mt = sam_view(v, po == 1 ? r + 1 : r - 1);
                if (mt.live) {
                    fl |= SAM_F_PAIRED | (po == 1 ? SAM_F_FIRST : SAM_F_LAST);
                    if (!mt.placed) fl |= SAM_F_MATE_UNPLACED;
                    else if (mt.minus) fl |= SAM_F_MATE_MINUS;
                    // rule 2; both mates come to the same verdict, the smaller index counts it
                    int verdict = 0;                                           // 0 not unique, 1 split, 2 improper, 3 proper
                    long long ins = 0;
                    if (me.unique && mt.unique) {
                        if (me.target != mt.target) verdict = 1;
                        else if (me.minus == mt.minus) verdict = 2;
                        else {
                            const SamView &p = me.minus ? mt : me, &m = me.minus ? me : mt;
                            ins = (long long) m.end - p.pos;
                            verdict = (p.pos <= m.pos && p.end <= m.end && ins >= 0 && ins <= (long long) max_insert) ? 3 : 2;
                        }
                    }
                    if (verdict == 3) fl |= SAM_F_PROPER;
                    if (me.placed && mt.placed && me.target == mt.target) {
                        const int32_t span = max(me.end, mt.end) - min(me.pos, mt.pos);
                        tl = (me.pos < mt.pos || (me.pos == mt.pos && po == 1)) ? span : -span;
                    }
                    if (po == 1) {
                        const bool wg = me.gapped || mt.gapped;
                        n_pairs++;
                        if (wg) n_wg++;
                        if (verdict == 0) n_nu++;
                        else if (verdict == 1) n_split++;
                        else if (verdict == 2) n_improper++;
                        else { n_proper++; if (wg) n_pg++; sum += (unsigned long long) ins; atomicAdd(&hist[ins], 1ull); }
                    }
                }
            }
        }
        flag[r] = (uint16_t) fl;
        tlen[r] = tl;
    }
    n_live = wave_sum(n_live); n_h = wave_sum(n_h); n_g = wave_sum(n_g); n_un = wave_sum(n_un); n_pairs = wave_sum(n_pairs); n_proper = wave_sum(n_proper);
    n_improper = wave_sum(n_improper); n_split = wave_sum(n_split); n_nu = wave_sum(n_nu); n_wg = wave_sum(n_wg); n_pg = wave_sum(n_pg); sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && n_live) {
        atomicAdd(&counters[SAM_LIVE], n_live);
        if (n_h) atomicAdd(&counters[SAM_PLACED_H], n_h);
        if (n_g) atomicAdd(&counters[SAM_PLACED_G], n_g);
        if (n_un) atomicAdd(&counters[SAM_UNPLACED], n_un);
        if (n_pairs) atomicAdd(&counters[SAM_PAIRS], n_pairs);
        if (n_proper) { atomicAdd(&counters[SAM_PROPER], n_proper); atomicAdd(&counters[SAM_INSERT_SUM], sum); }
        if (n_improper) atomicAdd(&counters[SAM_IMPROPER], n_improper);
        if (n_split) atomicAdd(&counters[SAM_SPLIT], n_split);
        if (n_nu) atomicAdd(&counters[SAM_NOT_UNIQUE], n_nu);
        if (n_wg) atomicAdd(&counters[SAM_WITH_GAPPED], n_wg);
        if (n_pg) atomicAdd(&counters[SAM_PROPER_GAPPED], n_pg);
    }
}

// ---- the SAM records ---------------------------------------------------------------------------------------------------------------------
// name(t): `contig_id=<t>_length=<len>`, in the depth form `_reads=<n>_depth=<q>.<dd>` behind it: FastaRecord's builders without the `>`
struct SamName {
    TextHeader<5> h;
    uint32_t n;                                                       // its bytes
    __device__ __forceinline__ void set(const SamText &f, uint32_t t) {
        FastaRecord<PackedSeq> b;
        b.head("contig_id=", (uint64_t) t, f.col_off[t + 1] - f.col_off[t]);
        if (f.names_depth) b.depth(f.t_reads[t], f.t_bases[t]);
        b.seal();
        h = b.h; n = b.hp - 1u;
    }
};

// `r<q>\t<flag>\t<rname>\t<pos>\t<mapq>\t<cigar>\t<rnext>\t<pnext>\t<tlen>\t<seq>\t*[\tNM:i:<nm>\tXP:A:<H|G>]\n`
struct SamRecord {
    static constexpr bool kPacked = true, kAligned = false;
    TextHeader<3> h0, h1, h2, tail;                                   // QNAME and FLAG; POS and MAPQ; PNEXT and TLEN (its sign in the literal); QUAL and the tags
    SamName name, next;
    uint32_t kind, nkind;                                             // RNAME: 0 `*`, 1 the name; RNEXT: 0 `*`, 1 `=`, 2 the name
    uint32_t e0, e1, e2, e3, e4, hp, L;                               // where the parts end; hp: where SEQ begins, L its length
    const uint32_t *rn;                                               // the runs of a G read (nr of them), else nr == 0 and cl == the read's length or 0 (`*`)
    uint32_t nr, cl;
    PackedSeq seq;
    __device__ __forceinline__ bool set(const SamText &f, uint64_t r) {
        const SamView me = sam_view(f.v, r);
        if (!me.live || (f.skip_unplaced && !me.placed)) return false;
        const uint32_t fl = f.flag[r];
        const bool paired = fl & SAM_F_PAIRED;
        const uint64_t m = (fl & SAM_F_FIRST) ? r + 1 : r - 1;
        SamView mt = me;
        if (paired) mt = sam_view(f.v, m);
        // RNAME / POS of this record and of the mate's: an unplaced read of a live pair borrows its placed mate's
        int32_t t1 = -1, p1 = -1, t2 = -1, p2 = -1;
        if (me.placed) { t1 = me.target; p1 = me.pos; }
        else if (paired && mt.placed) { t1 = mt.target; p1 = mt.pos; }
        if (paired) {
            if (mt.placed) { t2 = mt.target; p2 = mt.pos; }
            else if (me.placed) { t2 = me.target; p2 = me.pos; }
        }
        h0.f[0] = text_field("r", paired && m < r ? m : r); h0.f[1] = text_field("\t", (uint64_t) fl); h0.f[2] = text_lit("\t");
        e0 = h0.bytes() - 1u;
        kind = t1 >= 0 ? 1u : 0u;
        if (kind) name.set(f, (uint32_t) t1);
        e1 = e0 + (kind ? name.n : 1u);
        h1.f[0] = text_field("\t", (uint64_t) (p1 + 1)); h1.f[1] = text_field("\t", (me.placed && me.unique) ? 60ull : 0ull); h1.f[2] = text_lit("\t");
        e2 = e1 + h1.bytes() - 1u;
        // CIGAR; the clipped bases leave NM
        uint32_t cb = 1u, clip = 0;
        nr = 0; cl = 0; rn = nullptr;
        if (me.placed && !me.gapped) { cl = (uint32_t) me.L; cb = (uint32_t) dec_width(cl) + 1u; }
        else if (me.placed) {
            rn = f.v.g_cigar + f.v.g_cigar_off[r]; nr = f.v.g_cigar_off[r + 1] - f.v.g_cigar_off[r];
            cb = 0;
            for (uint32_t u = 0; u < nr; u++) {
                cb += (uint32_t) dec_width(rn[u] >> 2) + 1u;
                if ((u == 0 || u + 1 == nr) && (rn[u] & 3u) == SAM_OP_I) clip += rn[u] >> 2;
            }
        }
        e3 = e2 + cb;
        nkind = t2 < 0 ? 0u : (t2 == t1 ? 1u : 2u);
        if (nkind == 2) next.set(f, (uint32_t) t2);
        e4 = e3 + 1u + (nkind == 2 ? next.n : 1u);
        const int32_t tl = f.tlen[r];
        h2.f[0] = text_field("\t", (uint64_t) (p2 + 1));
        if (tl < 0) h2.f[1] = text_field("\t-", (uint64_t) (-(long long) tl)); else h2.f[1] = text_field("\t", (uint64_t) tl);
        h2.f[2] = text_lit("\t");
        hp = e4 + h2.bytes() - 1u;
        L = (uint32_t) me.L;
        seq.row = f.words + (size_t) (2 * r + ((me.placed && me.minus) ? 0 : 1)) * (size_t) f.stride; seq.q0 = 0;
        tail.f[0] = text_lit("\t*");
        if (me.placed) {
            const uint32_t nm = (uint32_t) me.nm > clip ? (uint32_t) me.nm - clip : 0u;
            tail.f[1] = text_field("\tNM:i:", (uint64_t) nm);
            if (me.gapped) tail.f[2] = text_lit("\tXP:A:G"); else tail.f[2] = text_lit("\tXP:A:H");
        }
        return true;
    }
    __device__ __forceinline__ uint32_t bytes() const { return hp + L + tail.bytes(); }
    __device__ __forceinline__ char cigar_at(uint32_t p) const {
        if (!nr) {
            if (!cl) return '*';
            const uint32_t w = (uint32_t) dec_width(cl);
            return p < w ? dec_digit(cl, w, p) : 'M';
        }
        for (uint32_t u = 0; u < nr; u++) {                               // as GpRecord::at renders them, an I run at either end as S
            const uint32_t ln = rn[u] >> 2, op = rn[u] & 3u, w = (uint32_t) dec_width(ln);
            if (p < w) return dec_digit(ln, w, p);
            if (p == w) return ((u == 0 || u + 1 == nr) && op == SAM_OP_I) ? 'S' : (char) ((0x44494Du >> (8 * op)) & 0xFF);   // "MID"
            p -= w + 1u;
        }
        return '*';
    }
    __device__ __forceinline__ char at(uint32_t p) const {
        if (p < e0) return h0.at(p);
        if (p < e1) return kind ? name.h.at(p - e0) : '*';
        if (p < e2) return h1.at(p - e1);
        if (p < e3) return cigar_at(p - e2);
        if (p < e4) return p == e3 ? '\t' : (nkind == 2 ? next.h.at(p - e3 - 1u) : (nkind ? '=' : '*'));
        if (p < hp) return h2.at(p - e4);
        if (p - hp < L) return seq.base(p - hp);
        return tail.at(p - hp - L);
    }
    __device__ __forceinline__ uint32_t packed() const { return L; }
    __device__ __forceinline__ uint4 bases16(uint32_t q) const { return seq.bases16(q); }
};

__global__ void __launch_bounds__(SAM_BLOCK) k_sam_sizes(SamText f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    // the writer's refusals: a live read longer than its row; a G read whose script has no run or not the read's length
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r < f.n) {
        const SamView me = sam_view(f.v, r);
        unsigned long long bad = 0;
        if (me.live && (long long) me.L > 16ll * f.stride) bad |= SAM_BAD_LEN;
        if (me.gapped) {
            const uint32_t a = f.v.g_cigar_off[r], b = f.v.g_cigar_off[r + 1];
            long long q = 0;
            for (uint32_t u = a; u < b; u++) if ((f.v.g_cigar[u] & 3u) != SAM_OP_D) q += f.v.g_cigar[u] >> 2;
            if (a >= b || q != (long long) me.L) bad |= SAM_BAD_SCRIPT;
        }
        if (bad) atomicOr(&counters[GFA_FLAGS], bad);
    }
    text_sizes_body<SamRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(SAM_BLOCK) k_sam_write(SamText f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<SamRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_sam_pair_check(const uint8_t *pair_off, uint64_t n, unsigned long long *counters, int max_blocks, hipStream_t s) {
    if (n && pair_off) hipLaunchKernelGGL(k_sam_pair_check, dim3(stage_grid(n, SAM_BLOCK, max_blocks > 0 ? std::min(max_blocks, 4096) : 4096)), dim3(SAM_BLOCK), 0, s, pair_off, n, counters);
}

void launch_sam_judge(const SamReads &v, int32_t max_insert, uint16_t *flag, int32_t *tlen, unsigned long long *hist, unsigned long long *counters, int max_blocks,
                      hipStream_t s) {
    if (v.R) hipLaunchKernelGGL(k_sam_judge, dim3(stage_grid(v.R, SAM_BLOCK, max_blocks > 0 ? std::min(max_blocks, 8192) : 8192)), dim3(SAM_BLOCK), 0, s, v, max_insert, flag, tlen, hist,
                                counters);
}

void launch_sam_sizes(const SamText &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_sam_sizes, dim3(text_sizes_blocks(f.n, SAM_BLOCK)), dim3(SAM_BLOCK), 0, s, f, sizes, counters);
}

void launch_sam_write(const SamText &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_sam_write, dim3(text_write_blocks(i0, i1, SAM_WAVES, f.max_blocks > 0 ? (uint64_t) f.max_blocks : 16384)), dim3(SAM_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
