// alga_amd/csrc/ipolish_kernels.hip -- the placed targets voted by the Hamming-placed and the gapped reads together: a column keeps its base, gets
// another or leaves, a string enters between two columns (include/alga_amd.h: alga_polish_indels_device; the definition is the comment there,
// host side in engine_ipolish.hip).
//
// Everything is in the placement's COLUMN space, as in polish_kernels.hip.  The H voters (one M run each, nearly all voters) are counted by that
// file's gather (launch_po_keys, the sort, launch_po_vote / _wide with its counts switched on: one 32-bit count per base and column, exact to
// 2^32 - 1, no atomics).  Only the G voters are walked here: they are the reads the Hamming pass could not place, a few per cent at most, and
// their cells are ADDED onto those counts by 32-bit integer atomics, which commute -- so the counts depend on no order.  One 32-bit path for
// them, no bit-sliced planes: a plane counter pays where a lane sees hundreds of voters per word, and here a word sees a handful.
//   k_ip_check        one thread per G voter: rule 8 on its script, then the walk of rule 2 (ip_walk) that only counts what it will vote
//   k_ip_vote_gapped  one thread per G voter: the same walk; M cells into counts4, D cells into del, an inner I run as a key (n << 26 | string)
//                     with its slot at a place an atomic cursor gives (their order is free: they are sorted), a long one into ins_all[slot]
//   k_ip_span         one thread per read: +1 / -1 of a voter's slots into the difference array (k_gp_depth_add's form); one scan follows
//   k_ip_ins_pick     over the votes sorted by (slot, key): the head of a slot's stretch walks it, run by run, and keeps (count desc, key asc)
//   k_ip_decide       one thread per old column: rules 4 and 5, the width of the column with its slot, its events, the per-target sums
//   k_ip_words        one lane per word of the NEW column array: a bisection in new_col for its first column, then a walk forward
//   k_ip_events       one thread per old column with an event: the insertion, then the column's own, at the place the scan of evn gives
//   k_ip_targets      one thread per target: new col_off / len / begin from new_col
//   k_ip_fasta_* / k_ip_tsv_*   the two text outputs through text_record.h
// ip_walk keeps no run array: the shift of a gap is found when the M run in front of it is walked (from the ORIGINAL runs: the walk is back at
// the original column and read offset after every gap), so a script costs a few registers and the kernels have no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ipolish_kernels.h"
#include "seed_device.h"
#include "text_record.h"

namespace alga {

namespace {

constexpr int IP_BLOCK = 256, IP_WAVES = IP_BLOCK / 64;
constexpr uint32_t IP_OP_M = 0, IP_OP_I = 1, IP_OP_D = 2;
constexpr uint8_t IP_ST_UNIQUE = 2, IP_ST_MINUS = 4;                    // ALGA_PLACE_ / ALGA_GAPPED_ UNIQUE and MINUS: the same bits

__device__ __forceinline__ uint32_t ip_wave_sum32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t) __shfl_xor((int) v, o);
    return v;
}
__device__ __forceinline__ uint32_t ip_wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t) __shfl_xor((int) v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t ip_wave_or32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t) __shfl_xor((int) v, o);
    return v;
}

// A G voter's script after rule 2, piece by piece, in order: em.m(first column, read offset, cells), em.d(first column, cells),
// em.ins(slot, read offset, bases, edge), em.shift(s) for a gap that moved.  c / a: the column and the read base the next run starts at.
template <class Emit>
__device__ __forceinline__ void ip_walk(const uint32_t *__restrict__ script, uint32_t nr, const uint32_t *__restrict__ row, const uint32_t *__restrict__ cols, uint32_t g0,
                                        Emit &em) {
    uint32_t c = g0, a = 0, pend = 0;                                  // pend: the shift of the gap behind the M run just walked
    for (uint32_t i = 0; i < nr; i++) {
        const uint32_t w = script[i], op = w & 3u, n = w >> 2;
        if (op == IP_OP_M) {
            uint32_t s = 0;
            if (i + 2 < nr) {                                          // the next run is neither the first nor the last
                const uint32_t wn = script[i + 1], opn = wn & 3u, nn = wn >> 2;
                if (opn == IP_OP_D) {
                    const uint64_t cc = (uint64_t) c + n;
                    while (s < n && base_at(cols, cc - 1 - s) == base_at(cols, cc + nn - 1 - s)) s++;
                } else if (opn == IP_OP_I) {
                    const uint64_t aa = (uint64_t) a + n;
                    while (s < n && base_at(row, aa - 1 - s) == base_at(row, aa + nn - 1 - s)) s++;
                }
            }
            if (n - s) em.m(c, a, n - s);
            c += n - s; a += n - s; pend = s;
        } else {
            const bool edge = i == 0 || i + 1 == nr;
            if (op == IP_OP_D) { em.d(c, n); c += n; }
            else { em.ins(c, a, n, edge); a += n; }
            if (pend) { em.shift(pend); em.m(c, a, pend); c += pend; a += pend; }      // the cells the gap passed over: M behind it
            pend = 0;
        }
    }
}

struct IpTally {
    int32_t max_ins;
    unsigned long long m_cells = 0, d_cells = 0;
    uint32_t ins_short = 0, ins_long = 0, ins_edge = 0, sh_runs = 0, sh_bases = 0;
    __device__ __forceinline__ void m(uint32_t, uint32_t, uint32_t n) { m_cells += n; }
    __device__ __forceinline__ void d(uint32_t, uint32_t n) { d_cells += n; }
    __device__ __forceinline__ void ins(uint32_t, uint32_t, uint32_t n, bool edge) { if (edge) ins_edge++; else if (n <= (uint32_t) max_ins) ins_short++; else ins_long++; }
    __device__ __forceinline__ void shift(uint32_t s) { sh_runs++; sh_bases += s; }
};

__global__ void __launch_bounds__(IP_BLOCK) k_ip_check(IpReads r, IpTargets t, int32_t max_ins, unsigned long long *__restrict__ counters) {
    IpTally ty{max_ins};
    unsigned long long voters = 0;
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * IP_BLOCK) {
        const uint8_t st = r.state[i];
        if (!(st & IP_ST_UNIQUE)) continue;
        const uint32_t v = (uint32_t) (2 * i) + ((st & IP_ST_MINUS) ? 0u : 1u);
        const int32_t L = r.len[v], tt = r.target[i], p = r.pos[i], e = r.end[i];
        const uint32_t o0 = r.cigar_off[i], o1 = r.cigar_off[i + 1];
        if (o1 < o0 || o1 - o0 > (uint32_t) IP_MAX_RUNS || o1 == o0 || (uint64_t) o1 > r.n_cigar) { bad |= IP_BAD_RUNS; continue; }
        if (tt < 0 || (uint32_t) tt >= t.T || p < 0 || e <= p || (int64_t) e > (int64_t) t.col_off[tt + 1] - (int64_t) t.col_off[tt]) { bad |= IP_BAD_PLACE; continue; }
        unsigned long long rl = 0, cl = 0;
        bool ops = true;
        for (uint32_t u = o0; u < o1; u++) {
            const uint32_t w = r.cigar[u], op = w & 3u;
            if (op == 3u) ops = false;
            if (op != IP_OP_D) rl += w >> 2;
            if (op != IP_OP_I) cl += w >> 2;
        }
        if (!ops) { bad |= IP_BAD_RUNS; continue; }
        if (L < 1 || (int64_t) L > 16ll * r.stride || rl != (unsigned long long) L) { bad |= IP_BAD_READ_LEN; continue; }
        if (cl != (unsigned long long) (e - p)) { bad |= IP_BAD_COL_LEN; continue; }
        voters++;
        ip_walk(r.cigar + o0, o1 - o0, r.rows + (uint64_t) v * (uint64_t) r.stride, t.cols, t.col_off[tt] + (uint32_t) p, ty);
    }
    voters = wave_sum(voters);
    const unsigned long long m = wave_sum(ty.m_cells), d = wave_sum(ty.d_cells);
    const uint32_t ins = ip_wave_sum32(ty.ins_short), il = ip_wave_sum32(ty.ins_long), ie = ip_wave_sum32(ty.ins_edge), sr = ip_wave_sum32(ty.sh_runs), sb = ip_wave_sum32(ty.sh_bases);
    bad = ip_wave_or32(bad);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&counters[IP_BAD], (unsigned long long) bad);
        if (voters) {
            atomicAdd(&counters[IP_VOTERS_G], voters); atomicAdd(&counters[IP_VOTES_G], m);
            if (d) atomicAdd(&counters[IP_DEL_VOTES], d);
            if (ins) atomicAdd(&counters[IP_INS_VOTES], (unsigned long long) ins);
            if (il) atomicAdd(&counters[IP_INS_LONG], (unsigned long long) il);
            if (ie) atomicAdd(&counters[IP_INS_EDGE], (unsigned long long) ie);
            if (sr) { atomicAdd(&counters[IP_SHIFTED_RUNS], (unsigned long long) sr); atomicAdd(&counters[IP_SHIFTED_BASES], (unsigned long long) sb); }
        }
    }
}

// (after the check: every G voter's script, target and position are in range; the key arrays hold counters[IP_INS_VOTES] entries)
struct IpCast {
    const uint32_t *row;
    int32_t max_ins;
    uint32_t *counts4, *del, *ins_all;
    unsigned long long *ins_key, *ins_slot, *cursor;
    __device__ __forceinline__ void m(uint32_t c, uint32_t a, uint32_t n) {
        for (uint32_t j = 0; j < n; j++) atomicAdd(&counts4[4ull * ((uint64_t) c + j) + base_at(row, (uint64_t) a + j)], 1u);
    }
    __device__ __forceinline__ void d(uint32_t c, uint32_t n) {
        for (uint32_t j = 0; j < n; j++) atomicAdd(&del[(uint64_t) c + j], 1u);
    }
    __device__ __forceinline__ void ins(uint32_t c, uint32_t a, uint32_t n, bool edge) {
        if (edge) return;
        if (n > (uint32_t) max_ins) { atomicAdd(&ins_all[c], 1u); return; }
        uint32_t str = 0;
        for (uint32_t j = 0; j < n; j++) str = (str << 2) | base_at(row, (uint64_t) a + j);
        const unsigned long long at = atomicAdd(cursor, 1ull);
        ins_key[at] = (unsigned long long) ((n << 26) | str);
        ins_slot[at] = (unsigned long long) c;
    }
    __device__ __forceinline__ void shift(uint32_t) {}
};

__global__ void __launch_bounds__(IP_BLOCK) k_ip_vote_gapped(IpReads r, IpTargets t, int32_t max_ins, uint32_t *__restrict__ counts4, uint32_t *__restrict__ del,
                                                             unsigned long long *__restrict__ ins_key, unsigned long long *__restrict__ ins_slot, uint32_t *__restrict__ ins_all,
                                                             unsigned long long *__restrict__ counters) {
    for (uint64_t i = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * IP_BLOCK) {
        const uint8_t st = r.state[i];
        if (!(st & IP_ST_UNIQUE)) continue;
        const uint32_t v = (uint32_t) (2 * i) + ((st & IP_ST_MINUS) ? 0u : 1u);
        const uint32_t o0 = r.cigar_off[i], o1 = r.cigar_off[i + 1];
        const uint32_t *row = r.rows + (uint64_t) v * (uint64_t) r.stride;
        IpCast cast{row, max_ins, counts4, del, ins_all, ins_key, ins_slot, &counters[IP_INS_CURSOR]};
        ip_walk(r.cigar + o0, o1 - o0, row, t.cols, t.col_off[r.target[i]] + (uint32_t) r.pos[i], cast);
    }
}

__global__ void __launch_bounds__(IP_BLOCK) k_ip_span(IpReads r, IpTargets t, const int32_t *__restrict__ pl_target, const int32_t *__restrict__ pl_pos,
                                                      const uint8_t *__restrict__ pl_state, uint32_t *__restrict__ diff) {
    for (uint64_t i = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * IP_BLOCK) {
        const uint8_t sh = pl_state[i], sg = r.state[i];
        uint32_t p, e;
        if (sh & IP_ST_UNIQUE) {
            p = t.col_off[pl_target[i]] + (uint32_t) pl_pos[i];
            e = p + (uint32_t) r.len[2 * i + ((sh & IP_ST_MINUS) ? 0u : 1u)];
        } else if (sg & IP_ST_UNIQUE) {
            const uint32_t o = t.col_off[r.target[i]];
            p = o + (uint32_t) r.pos[i]; e = o + (uint32_t) r.end[i];
        } else continue;
        atomicAdd(&diff[p + 1], 1u);                                   // e > p: p + 1 <= e <= columns, the array has columns + 1 entries
        atomicAdd(&diff[e], 0xFFFFFFFFu);
    }
}

__global__ void __launch_bounds__(IP_BLOCK) k_ip_ins_pick(const unsigned long long *__restrict__ slot, const unsigned long long *__restrict__ key, uint64_t n,
                                                          uint32_t *__restrict__ win_key, uint32_t *__restrict__ win_votes, uint32_t *__restrict__ ins_all) {
    for (uint64_t i = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; i < n; i += (uint64_t) gridDim.x * IP_BLOCK) {
        const unsigned long long c = slot[i];
        if (i && slot[i - 1] == c) continue;                           // not the head of its slot
        unsigned long long best_key = 0, run_key = key[i];
        uint32_t best = 0, run = 0, total = 0;
        for (uint64_t j = i; j < n && slot[j] == c; j++) {
            const unsigned long long k = key[j];
            if (k != run_key) { if (run > best) { best = run; best_key = run_key; } run_key = k; run = 0; }
            run++; total++;
        }
        if (run > best) { best = run; best_key = run_key; }           // keys ascend: the first of equal counts stays
        win_key[c] = (uint32_t) best_key; win_votes[c] = best;
        ins_all[c] += total;                                          // one thread per slot; the long ones were added before this kernel
    }
}

__global__ void __launch_bounds__(IP_BLOCK) k_ip_decide(IpTargets t, IpDecide d, unsigned long long *__restrict__ counters) {
    uint32_t n_voted = 0, n_sub = 0, n_del = 0, n_slots = 0, n_bases = 0, n_ac = 0, n_as = 0, mx = 0;
    for (uint64_t g = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; g <= t.columns; g += (uint64_t) gridDim.x * IP_BLOCK) {
        if (g == t.columns) { d.width[g] = 0; d.evn[g] = 0; continue; }
        const uint4 n4 = *reinterpret_cast<const uint4 *>(d.counts4 + 4 * g);
        const uint32_t v[5] = {n4.x, n4.y, n4.z, n4.w, d.del[g]};
        const uint32_t cur = base_at(t.cols, g), cover = v[0] + v[1] + v[2] + v[3] + v[4];
        uint32_t best = v[0], w = 0;
#pragma unroll
        for (uint32_t b = 1; b < 5; b++) if (v[b] > best) { best = v[b]; w = b; }
        const uint32_t ncur = cur == 0 ? v[0] : cur == 1 ? v[1] : cur == 2 ? v[2] : v[3];
        if (ncur == best) w = cur;                                    // a tie goes to cur, else to the smallest of A < C < G < T < -
        const bool differs = w != cur && cover >= (uint32_t) d.min_cover;
        const bool enough = 100ull * (unsigned long long) best >= (unsigned long long) d.min_percent * (unsigned long long) cover;
        const bool changed = differs && enough, amb_col = differs && !enough;
        const bool deleted = changed && w == 4u, subst = changed && w != 4u;
        const uint32_t span = d.span_scan[g + 1], key = d.win_key[g], wv = d.win_votes[g], all = d.ins_all[g];
        const bool spanned = span >= (uint32_t) d.min_cover;
        const bool ins = key && spanned && 100ull * (unsigned long long) wv >= (unsigned long long) d.min_percent * (unsigned long long) span;
        const bool amb_slot = spanned && !ins && 100ull * (unsigned long long) all >= (unsigned long long) d.min_percent * (unsigned long long) span;
        const uint32_t nins = ins ? key >> 26 : 0u;
        d.width[g] = nins + (deleted ? 0u : 1u);
        d.evn[g] = (uint32_t) ins + (uint32_t) changed;
        d.code[g] = (uint8_t) ((subst ? w : cur) | (deleted ? IP_C_DELETED : 0u) | (subst ? IP_C_SUBST : 0u) | (ins ? IP_C_INSERTED : 0u) | (amb_col ? IP_C_AMB_COL : 0u) |
                               (amb_slot ? IP_C_AMB_SLOT : 0u));
        if (d.counts5) {
#pragma unroll
            for (int b = 0; b < 5; b++) d.counts5[5 * g + b] = v[b];
            d.span[g] = span;
        }
        n_voted += cover >= (uint32_t) d.min_cover; n_sub += subst; n_del += deleted; n_slots += ins; n_bases += nins; n_ac += amb_col; n_as += amb_slot;
        mx = cover > mx ? cover : mx;
        if (changed | ins | amb_col | amb_slot) {                     // rare: one atomic per marked column
            const uint32_t tt = item_of(t.col_off, t.T, (uint32_t) g);
            if (subst) atomicAdd(&d.t_subs[tt], 1ull);
            if (deleted) atomicAdd(&d.t_dels[tt], 1ull);
            if (ins) atomicAdd(&d.t_ins[tt], (unsigned long long) nins);
            if (amb_col | amb_slot) atomicAdd(&d.t_amb[tt], (unsigned long long) ((uint32_t) amb_col + (uint32_t) amb_slot));
        }
    }
    n_voted = ip_wave_sum32(n_voted); n_sub = ip_wave_sum32(n_sub); n_del = ip_wave_sum32(n_del); n_slots = ip_wave_sum32(n_slots); n_bases = ip_wave_sum32(n_bases);
    n_ac = ip_wave_sum32(n_ac); n_as = ip_wave_sum32(n_as); mx = ip_wave_max32(mx);
    if ((threadIdx.x & 63) == 0) {
        if (n_voted) atomicAdd(&counters[IP_VOTED], (unsigned long long) n_voted);
        if (n_sub) atomicAdd(&counters[IP_SUBST], (unsigned long long) n_sub);
        if (n_del) atomicAdd(&counters[IP_DELETED], (unsigned long long) n_del);
        if (n_slots) { atomicAdd(&counters[IP_INS_SLOTS], (unsigned long long) n_slots); atomicAdd(&counters[IP_INS_BASES], (unsigned long long) n_bases); }
        if (n_ac) atomicAdd(&counters[IP_AMB_COLS], (unsigned long long) n_ac);
        if (n_as) atomicAdd(&counters[IP_AMB_SLOTS], (unsigned long long) n_as);
        if (mx) atomicMax(&counters[IP_MAX_COVER], (unsigned long long) mx);
    }
}

__global__ void __launch_bounds__(IP_BLOCK) k_ip_words(IpTargets t, IpBuild b, uint32_t *__restrict__ words) {
    // the items are the old columns, item g as wide as the new columns it becomes (new_col is the scan of the widths over columns + 1 entries, the
    // last width 0: new_col[columns] == new_columns); a deleted column is an empty item
    packed_words_body<IP_BLOCK>(b.new_col, (uint32_t) t.columns, b.new_columns, ((b.new_columns + 15) >> 4) + 2, words, [&](uint32_t g, uint32_t off) {
        const uint32_t cd = b.code[g];
        const uint32_t key = (cd & IP_C_INSERTED) ? b.win_key[g] : 0u, nins = key >> 26;
        return off < nins ? (key >> (2 * (nins - 1 - off))) & 3u : cd & IP_C_BASE;
    });
}

__global__ void __launch_bounds__(IP_BLOCK) k_ip_events(IpTargets t, IpBuild b, IpEvents ev) {
    for (uint64_t g = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; g < t.columns; g += (uint64_t) gridDim.x * IP_BLOCK) {
        uint32_t o = b.ev_off[g];
        if (b.ev_off[g + 1] == o) continue;
        const uint32_t cd = b.code[g], cur = base_at(t.cols, g);
        const uint4 n4 = *reinterpret_cast<const uint4 *>(b.counts4 + 4 * g);
        const uint32_t dl = b.del[g], cover = n4.x + n4.y + n4.z + n4.w + dl;
        if (cd & IP_C_INSERTED) {
            const uint32_t key = b.win_key[g];
            ev.col[o] = (uint32_t) g; ev.kind[o] = 1; ev.len[o] = (uint8_t) (key >> 26); ev.bases[o] = key & ((1u << 26) - 1u);
            ev.votes[o] = b.win_votes[g]; ev.cover[o] = b.span_scan[g + 1];
            o++;
        }
        if (cd & IP_C_SUBST) {
            const uint32_t nw = cd & IP_C_BASE;
            ev.col[o] = (uint32_t) g; ev.kind[o] = 0; ev.len[o] = 1; ev.bases[o] = cur | (nw << 2);
            ev.votes[o] = nw == 0 ? n4.x : nw == 1 ? n4.y : nw == 2 ? n4.z : n4.w; ev.cover[o] = cover;
        } else if (cd & IP_C_DELETED) {
            ev.col[o] = (uint32_t) g; ev.kind[o] = 2; ev.len[o] = 1; ev.bases[o] = cur; ev.votes[o] = dl; ev.cover[o] = cover;
        }
    }
}

__global__ void __launch_bounds__(IP_BLOCK) k_ip_targets(IpTargets t, const uint32_t *__restrict__ new_col, uint32_t *__restrict__ col_off, int32_t *__restrict__ len,
                                                         unsigned long long *__restrict__ begin, unsigned long long *__restrict__ counters) {
    uint32_t mx = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * IP_BLOCK + threadIdx.x; i <= t.T; i += (uint64_t) gridDim.x * IP_BLOCK) {
        const uint32_t c0 = new_col[t.col_off[i]];
        col_off[i] = c0;
        if (i < t.T) {
            const uint32_t l = new_col[t.col_off[i + 1]] - c0;
            len[i] = (int32_t) l; begin[i] = c0;
            mx = l > mx ? l : mx;
        }
    }
    mx = ip_wave_max32(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&counters[IP_LONGEST], (unsigned long long) mx);
}

// ---- the two text outputs ----------------------------------------------------------------------------------------------------------------
// `>contig_id=<t>_length=<len>_subs=<s>_ins=<i>_dels=<d>\n<columns col_off[t] .. col_off[t + 1])>\n`
struct IpRecord : FastaRecord<PackedSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const IpFasta &f, uint64_t j) {
        const int32_t len = f.len[j];
        if (len <= 0) return false;
        contig_head(j, (uint32_t) len);
        h.f[2] = text_field("_subs=", f.t_subs[j]); h.f[3] = text_field("_ins=", f.t_ins[j]); h.f[4] = text_field("_dels=", f.t_dels[j]); seal();
        seq.row = f.words; seq.q0 = f.col_off[j];
        return true;
    }
};

__global__ void __launch_bounds__(IP_BLOCK) k_ip_fasta_sizes(IpFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<IpRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(IP_BLOCK) k_ip_fasta_write(IpFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<IpRecord>(f, off, i0, i1, buf);
}

// `<contig>\t<pos>\t<kind>\t<len>\t<old>\t<new>\t<votes>\t<cover>\n`
struct IpLine {
    static constexpr bool kPacked = false, kAligned = false;
    TextHeader<3> h;
    TextHeader<2> tail;
    uint32_t hb, kind, n, bases;
    __device__ __forceinline__ bool set(const IpTsv &f, uint64_t i) {
        const uint32_t g = f.col[i], tt = item_of(f.old_col_off, f.T, g);
        kind = f.kind[i]; n = f.len[i]; bases = f.bases[i];
        h.f[0] = text_field("", (uint64_t) tt); h.f[1] = text_field("\t", (uint64_t) (g - f.old_col_off[tt]));
        if (kind == 0) h.f[2] = text_field("\tS\t", (uint64_t) n); else if (kind == 1) h.f[2] = text_field("\tI\t", (uint64_t) n); else h.f[2] = text_field("\tD\t", (uint64_t) n);
        hb = h.bytes() - 1u;
        tail.f[0] = text_field("\t", (uint64_t) f.votes[i]); tail.f[1] = text_field("\t", (uint64_t) f.cover[i]);
        return true;
    }
    __device__ __forceinline__ uint32_t n_new() const { return kind == 1 ? n : 1u; }
    __device__ __forceinline__ uint32_t bytes() const { return hb + 3u + n_new() + tail.bytes(); }
    __device__ __forceinline__ char letter(uint32_t b) const { return (char) ((0x54474341u >> (8 * (b & 3u))) & 0xFF); }
    __device__ __forceinline__ char at(uint32_t p) const {
        if (p < hb) return h.at(p);
        p -= hb;
        if (p == 0 || p == 2) return '\t';
        if (p == 1) return kind == 1 ? '-' : letter(bases);
        const uint32_t nn = n_new();
        if (p < 3u + nn) {
            if (kind == 0) return letter(bases >> 2);
            if (kind == 2) return '-';
            return letter(bases >> (2 * (n - 1u - (p - 3u))));
        }
        return tail.at(p - 3u - nn);
    }
};

__global__ void __launch_bounds__(IP_BLOCK) k_ip_tsv_sizes(IpTsv f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<IpLine>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(IP_BLOCK) k_ip_tsv_write(IpTsv f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<IpLine>(f, off, i0, i1, buf);
}

}  // namespace

void launch_ip_check(const IpReads &r, const IpTargets &t, int32_t max_ins, unsigned long long *counters, hipStream_t s) {
    if (r.R) hipLaunchKernelGGL(k_ip_check, dim3(stage_grid(r.R, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, r, t, max_ins, counters);
}

void launch_ip_vote_gapped(const IpReads &r, const IpTargets &t, int32_t max_ins, uint32_t *counts4, uint32_t *del, unsigned long long *ins_key, unsigned long long *ins_slot,
                           uint32_t *ins_all, unsigned long long *counters, hipStream_t s) {
    if (r.R) hipLaunchKernelGGL(k_ip_vote_gapped, dim3(stage_grid(r.R, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, r, t, max_ins, counts4, del, ins_key, ins_slot, ins_all, counters);
}

void launch_ip_span(const IpReads &r, const IpTargets &t, const int32_t *pl_target, const int32_t *pl_pos, const uint8_t *pl_state, uint32_t *diff, hipStream_t s) {
    if (r.R) hipLaunchKernelGGL(k_ip_span, dim3(stage_grid(r.R, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, r, t, pl_target, pl_pos, pl_state, diff);
}

void launch_ip_ins_pick(const unsigned long long *slot, const unsigned long long *key, uint64_t n, uint32_t *win_key, uint32_t *win_votes, uint32_t *ins_all, uint32_t max_blocks,
                        hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_ip_ins_pick, dim3(stage_grid(n, IP_BLOCK, max_blocks)), dim3(IP_BLOCK), 0, s, slot, key, n, win_key, win_votes, ins_all);
}

void launch_ip_decide(const IpTargets &t, const IpDecide &d, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_ip_decide, dim3(stage_grid(t.columns + 1, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, t, d, counters);
}

void launch_ip_words(const IpTargets &t, const IpBuild &b, uint32_t *words, hipStream_t s) {
    hipLaunchKernelGGL(k_ip_words, dim3(stage_grid(((b.new_columns + 15) >> 4) + 2, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, t, b, words);
}

void launch_ip_events(const IpTargets &t, const IpBuild &b, const IpEvents &ev, hipStream_t s) {
    if (t.columns) hipLaunchKernelGGL(k_ip_events, dim3(stage_grid(t.columns, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, t, b, ev);
}

void launch_ip_targets(const IpTargets &t, const uint32_t *new_col, uint32_t *col_off, int32_t *len, unsigned long long *begin, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_ip_targets, dim3(stage_grid((uint64_t) t.T + 1, IP_BLOCK, t.max_blocks)), dim3(IP_BLOCK), 0, s, t, new_col, col_off, len, begin, counters);
}

void launch_ip_fasta_sizes(const IpFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_ip_fasta_sizes, dim3(text_sizes_blocks(f.n, IP_BLOCK)), dim3(IP_BLOCK), 0, s, f, sizes, counters);
}

void launch_ip_fasta_write(const IpFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_ip_fasta_write, dim3(text_write_blocks(i0, i1, IP_WAVES)), dim3(IP_BLOCK), 0, s, f, off, i0, i1, buf);
}

void launch_ip_tsv_sizes(const IpTsv &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_ip_tsv_sizes, dim3(text_sizes_blocks(f.n, IP_BLOCK)), dim3(IP_BLOCK), 0, s, f, sizes, counters);
}

void launch_ip_tsv_write(const IpTsv &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_ip_tsv_write, dim3(text_write_blocks(i0, i1, IP_WAVES)), dim3(IP_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
