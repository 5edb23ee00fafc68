// alga_amd/csrc/scaffold_kernels.hip -- scaffolds from the pairs the placement split over two targets (include/alga_amd.h:
// alga_scaffold_placed_device; the definition is the comment there, host side in engine_scaffold.hip).
//
// Integer work only, wave-64, nothing depends on thread order or on the sort's order among equal keys: counts and sums are integer adds, the
// best and second-best bundle of an end are 64-bit atomicMax on links << 32 | ~partner (distinct per end: the partners differ).
//   k_sc_check        pair_off as the placement checks it, every UNIQUE read as the polish checks a voter -> the refusal flags
//   k_sc_links        one thread per read: the judge of a split pair writes (a << 32 | b, span), every other read a sentinel above every key
//   k_sc_heads        first link of every key among the sorted links; their count
//   k_sc_bundle_fill  the first link of every bundle at the place the scan of the heads gives, the spans added (one atomic per wave where
//                     the wave's links are of one bundle: a bundle over several blocks is a few adds)
//   k_sc_bundles      a, b, links, gap, SUPPORTED; best[end]       k_sc_second   second[end]
//   k_sc_choice       AMBIGUOUS and choice per end                 k_sc_joins    JOIN where both ends chose each other; partner[end]
//   k_sc_cycle_drop / k_sc_rank_init / k_sc_place / k_sc_layout   the joins turned into ordered, oriented paths by the chain core (chain_kernels.h;
//                     these four instantiate chain_device.h): a dropped join is DROPPED on its bundle, a state weighs its contig's length and the
//                     gap behind it; start, gap_after, join_links, JOINED per contig in the direction item 7 chooses; the 64-bit scaffold lengths
//   k_sc_fasta_sizes / k_sc_fasta_write   one record per scaffold, one wave per record; a byte finds its contig by bisection over the starts
// Block 256 and the grid caps are picked, not tuned; the launches' max_blocks lowers the cap of every grid that goes through stage_grid and of the
// FASTA write grid (option "scaffold_max_blocks": a knob of the tests, which make every grid-stride loop here take further passes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "scaffold_kernels.h"
#include "packed_device.h"
#include "text_record.h"
#include "chain_device.h"

namespace alga {

namespace {

constexpr int SC_BLOCK = 256, SC_WAVES = SC_BLOCK / 64;
static_assert(SC_BLOCK == CHAIN_BLOCK, "the bodies of chain_device.h stride by CHAIN_BLOCK");
constexpr uint8_t SC_ST_UNIQUE = 2, SC_ST_MINUS = 4;                    // ALGA_PLACE_UNIQUE, ALGA_PLACE_MINUS

__device__ __forceinline__ uint32_t sc_wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t) __shfl_xor((int) v, o);
    return v;
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_check(ScReads r, ScTargets t, unsigned long long *__restrict__ counters) {
    uint32_t bad = 0;
    const uint64_t n = 2 * r.R, step = (uint64_t) gridDim.x * SC_BLOCK;
    if (r.pair_off)
        for (uint64_t v = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; v < n; v += step) {
            const uint8_t po = r.pair_off[v];
            if (po > 2 || po != r.pair_off[v ^ 1]) bad |= SC_BAD_PAIR;
            else if (po == 1 && (v + 2 >= n || r.pair_off[v + 2] != 2)) bad |= SC_BAD_PAIR;
            else if (po == 2 && (v < 2 || r.pair_off[v - 2] != 1)) bad |= SC_BAD_PAIR;
        }
    for (uint64_t i = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; i < r.R; i += step) {
        if (!(r.state[i] & SC_ST_UNIQUE)) continue;
        const int32_t L = r.len[2 * i + 1];
        if (L < 1 || (int64_t) L > 16ll * r.stride) { bad |= SC_BAD_LEN; continue; }
        const int32_t tt = r.target[i], p = r.pos[i];
        if (tt < 0 || (uint32_t) tt >= t.T || p < 0 || (int64_t) p + L > (int64_t) t.col_off[tt + 1] - (int64_t) t.col_off[tt]) bad |= SC_BAD_PLACE;
    }
    bad = sc_wave_or(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(&counters[SC_BAD], (unsigned long long) bad);
}

// (after the check: every UNIQUE read lies inside its target, a judge's mate is read r + 1 < R)
__global__ void __launch_bounds__(SC_BLOCK) k_sc_links(ScReads r, ScTargets t, int32_t max_insert, unsigned long long sentinel, unsigned long long *__restrict__ keys,
                                                       uint32_t *__restrict__ vals, uint32_t *__restrict__ span, unsigned long long *__restrict__ counters) {
    unsigned long long n_split = 0, n_links = 0, n_far = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; i < r.R; i += (uint64_t) gridDim.x * SC_BLOCK) {
        unsigned long long key = sentinel;
        uint32_t sp = 0;
        if (r.pair_off[2 * i + 1] == 1) {
            const uint64_t j = i + 1;
            const uint8_t s1 = r.state[i], s2 = r.state[j];
            const int32_t t1 = r.target[i], t2 = r.target[j];
            if ((s1 & SC_ST_UNIQUE) && (s2 & SC_ST_UNIQUE) && t1 != t2) {
                n_split++;
                const long long l1 = (long long) t.col_off[t1 + 1] - (long long) t.col_off[t1], l2 = (long long) t.col_off[t2 + 1] - (long long) t.col_off[t2];
                const long long d1 = (s1 & SC_ST_MINUS) ? (long long) r.pos[i] + r.len[2 * i + 1] : l1 - r.pos[i];
                const long long d2 = (s2 & SC_ST_MINUS) ? (long long) r.pos[j] + r.len[2 * j + 1] : l2 - r.pos[j];
                if (d1 + d2 <= (long long) max_insert) {
                    const uint32_t x1 = 2u * (uint32_t) t1 + ((s1 & SC_ST_MINUS) ? 0u : 1u), x2 = 2u * (uint32_t) t2 + ((s2 & SC_ST_MINUS) ? 0u : 1u);
                    const uint32_t a = x1 < x2 ? x1 : x2, b = x1 < x2 ? x2 : x1;
                    key = ((unsigned long long) a << 32) | b;
                    sp = (uint32_t) (d1 + d2);
                    n_links++;
                } else n_far++;
            }
        }
        keys[i] = key; vals[i] = (uint32_t) i; span[i] = sp;
    }
    n_split = wave_sum(n_split); n_links = wave_sum(n_links); n_far = wave_sum(n_far);
    if ((threadIdx.x & 63) == 0 && n_split) {
        atomicAdd(&counters[SC_SPLIT], n_split);
        if (n_links) atomicAdd(&counters[SC_LINKS], n_links);
        if (n_far) atomicAdd(&counters[SC_TOO_FAR], n_far);
    }
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_heads(const unsigned long long *__restrict__ keys, uint64_t n_links, uint32_t *__restrict__ heads,
                                                       unsigned long long *__restrict__ counters) {
    unsigned long long n = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; i < n_links; i += (uint64_t) gridDim.x * SC_BLOCK) {
        const uint32_t h = i == 0 || keys[i] != keys[i - 1];
        heads[i] = h; n += h;
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&counters[SC_BUNDLES], n);
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_bundle_fill(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ span, const uint32_t *__restrict__ heads,
                                                             const uint32_t *__restrict__ pos, uint64_t n_links, uint64_t n_bundles, uint32_t *__restrict__ b_start,
                                                             unsigned long long *__restrict__ b_span) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) b_start[n_bundles] = (uint32_t) n_links;
    // whole waves stride: lane l of a pass holds link base + l
    for (uint64_t base = (uint64_t) blockIdx.x * SC_BLOCK + (threadIdx.x & ~63); base < n_links; base += (uint64_t) gridDim.x * SC_BLOCK) {
        const uint64_t i = base + (uint64_t) lane;
        const bool active = i < n_links;
        uint32_t bid = 0;
        unsigned long long sp = 0;
        if (active) {
            const uint32_t h = heads[i];
            bid = pos[i] + h - 1u;
            if (h) b_start[bid] = (uint32_t) i;
            sp = span[vals[i]];
        }
        const uint32_t bid0 = (uint32_t) __shfl((int) bid, 0);            // lane 0 is active wherever a lane of the pass is
        if (__all(!active || bid == bid0)) {
            sp = wave_sum(sp);
            if (lane == 0) atomicAdd(&b_span[bid0], sp);
        } else if (active) atomicAdd(&b_span[bid], sp);
    }
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_bundles(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ b_start, ScBundles b, ScParams p,
                                                         unsigned long long *__restrict__ best, unsigned long long *__restrict__ counters) {
    unsigned long long n_sup = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; i < b.n; i += (uint64_t) gridDim.x * SC_BLOCK) {
        const uint32_t i0 = b_start[i], n = b_start[i + 1] - i0;
        const unsigned long long key = keys[i0];
        const uint32_t ea = (uint32_t) (key >> 32), eb = (uint32_t) key;
        const bool sup = (unsigned long long) n >= (unsigned long long) p.min_links;
        b.a[i] = ea; b.b[i] = eb; b.links[i] = n;
        b.gap[i] = (int32_t) ((long long) p.insert - (long long) (b.span[i] / (unsigned long long) n));
        b.state[i] = sup ? SC_B_SUPPORTED : (uint8_t) 0;
        if (sup) {
            n_sup++;
            atomicMax(&best[ea], ((unsigned long long) n << 32) | (uint32_t) ~eb);
            atomicMax(&best[eb], ((unsigned long long) n << 32) | (uint32_t) ~ea);
        }
    }
    n_sup = wave_sum(n_sup);
    if ((threadIdx.x & 63) == 0 && n_sup) atomicAdd(&counters[SC_SUPPORTED], n_sup);
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_second(ScBundles b, const unsigned long long *__restrict__ best, unsigned long long *__restrict__ second) {
    for (uint64_t i = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; i < b.n; i += (uint64_t) gridDim.x * SC_BLOCK) {
        if (!(b.state[i] & SC_B_SUPPORTED)) continue;
        const uint32_t ea = b.a[i], eb = b.b[i];
        const unsigned long long n = b.links[i], pa = (n << 32) | (uint32_t) ~eb, pb = (n << 32) | (uint32_t) ~ea;
        if (pa != best[ea]) atomicMax(&second[ea], pa);
        if (pb != best[eb]) atomicMax(&second[eb], pb);
    }
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_choice(const unsigned long long *__restrict__ best, const unsigned long long *__restrict__ second, uint64_t n_ends,
                                                        int32_t max_second_percent, uint32_t *__restrict__ choice, uint8_t *__restrict__ end_state,
                                                        unsigned long long *__restrict__ counters) {
    unsigned long long n_amb = 0;
    for (uint64_t x = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; x < n_ends; x += (uint64_t) gridDim.x * SC_BLOCK) {
        const unsigned long long b1 = best[x], b2 = second[x];
        uint8_t st = 0;
        uint32_t ch = SC_NONE;
        if (b1) {
            st = SC_E_SUPPORTED;
            const bool amb = b2 && 100ull * (b2 >> 32) >= (unsigned long long) max_second_percent * (b1 >> 32);
            if (amb) { st |= SC_E_AMBIGUOUS; n_amb++; }
            else ch = ~(uint32_t) b1;
        }
        choice[x] = ch; end_state[x] = st;
    }
    n_amb = wave_sum(n_amb);
    if ((threadIdx.x & 63) == 0 && n_amb) atomicAdd(&counters[SC_AMBIGUOUS], n_amb);
}

// (an end is joined by at most one bundle: its choice is one end, and only the bundle of that key can name it)
__global__ void __launch_bounds__(SC_BLOCK) k_sc_joins(ScBundles b, const uint32_t *__restrict__ choice, uint32_t *__restrict__ partner, uint32_t *__restrict__ join_bundle) {
    for (uint64_t i = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; i < b.n; i += (uint64_t) gridDim.x * SC_BLOCK) {
        if (!(b.state[i] & SC_B_SUPPORTED)) continue;
        const uint32_t ea = b.a[i], eb = b.b[i];
        if (choice[ea] != eb || choice[eb] != ea) continue;
        b.state[i] = SC_B_SUPPORTED | SC_B_JOIN;
        partner[ea] = eb; partner[eb] = ea;
        join_bundle[ea] = (uint32_t) i; join_bundle[eb] = (uint32_t) i;
    }
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_cycle_drop(ChainLists l, uint32_t T, uint32_t *__restrict__ partner, const uint32_t *__restrict__ join_bundle,
                                                            uint8_t *__restrict__ b_state, unsigned long long *__restrict__ counters) {
    chain_cycle_drop_body(l, T, partner, [=](uint64_t x, uint32_t) { b_state[join_bundle[x]] = SC_B_SUPPORTED | SC_B_JOIN | SC_B_DROPPED; }, &counters[SC_DROPPED]);
}

// the gap behind a joined end (its bundle's, at least min_gap); as Weight, a contig's length and the gap behind the end it is left at
struct ScGap {
    const uint32_t *col_off, *join_bundle;
    const int32_t *b_gap;
    int32_t min_gap;
    __device__ __forceinline__ uint32_t behind(uint32_t end, bool joined) const {
        if (!joined) return 0u;
        const int32_t g = b_gap[join_bundle[end]];
        return (uint32_t) (g > min_gap ? g : min_gap);
    }
    __device__ __forceinline__ unsigned long long operator()(uint32_t x, bool joined) const {
        return (unsigned long long) (col_off[(x >> 1) + 1] - col_off[x >> 1]) + behind(x ^ 1u, joined);
    }
};

__global__ void __launch_bounds__(SC_BLOCK) k_sc_rank_init(ScTargets t, const uint32_t *__restrict__ partner, const uint32_t *__restrict__ join_bundle,
                                                           const int32_t *__restrict__ b_gap, int32_t min_gap, ChainLists l) {
    chain_rank_init_body(partner, 2ull * t.T, l, ScGap{t.col_off, join_bundle, b_gap, min_gap});
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_place(ScTargets t, ChainLists l, const uint32_t *__restrict__ partner, const uint32_t *__restrict__ join_bundle,
                                                       const int32_t *__restrict__ b_gap, const uint32_t *__restrict__ b_links, int32_t min_gap, ScLayout o,
                                                       uint32_t *__restrict__ head, uint32_t *__restrict__ first, uint32_t *__restrict__ members,
                                                       unsigned long long *__restrict__ counters) {
    unsigned long long n_joins = 0;
    for (uint64_t c = (uint64_t) blockIdx.x * SC_BLOCK + threadIdx.x; c <= t.T; c += (uint64_t) gridDim.x * SC_BLOCK) {
        if (c == t.T) { first[c] = 0; members[c] = 0; continue; }               // the place of the scans' totals
        const uint32_t len = t.col_off[c + 1] - t.col_off[c];
        o.end_state[2 * c] |= partner[2 * c] != CHAIN_NONE ? SC_E_JOINED : (uint8_t) 0;
        o.end_state[2 * c + 1] |= partner[2 * c + 1] != CHAIN_NONE ? SC_E_JOINED : (uint8_t) 0;
        if (len == 0) {                                                        // in no scaffold (nothing is placed on it: it has no join)
            o.scaffold[c] = -1; o.rank[c] = -1; o.orient[c] = 0; o.start[c] = 0; o.gap_after[c] = 0; o.join_links[c] = 0;
            head[c] = (uint32_t) c; first[c] = 0; members[c] = 0;
            continue;
        }
        const ChainPos p = chain_position(l, (uint32_t) c);
        const bool joined = partner[p.out] != CHAIN_NONE;
        o.rank[c] = (int32_t) p.rank; o.orient[c] = (uint8_t) p.e;
        o.start[c] = l.wsum[p.hx] - l.wsum[p.x];
        o.gap_after[c] = (int32_t) ScGap{t.col_off, join_bundle, b_gap, min_gap}.behind(p.out, joined);
        o.join_links[c] = joined ? b_links[join_bundle[p.out]] : 0u;
        n_joins += joined;
        head[c] = p.hx >> 1; first[c] = p.rank == 0; members[c] = p.rank == 0 ? p.m : 0u;
    }
    n_joins = wave_sum(n_joins);
    if ((threadIdx.x & 63) == 0 && n_joins) atomicAdd(&counters[SC_JOINS], n_joins);
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_layout(ScTargets t, ChainLists l, const uint32_t *__restrict__ head, const uint32_t *__restrict__ first_scan,
                                                        const uint32_t *__restrict__ members_scan, ScLayout o, unsigned long long *__restrict__ counters) {
    unsigned long long n_sc = 0, n_multi = 0, n_mem = 0, longest = 0;
    chain_layout_body(l, t.T, o.rank, o.orient, head, first_scan, members_scan, o.scaffold, o.s_off, o.s_members,
                      [&](uint32_t, uint32_t sid, uint32_t, unsigned long long bases, uint32_t members) {      // the 64-bit length
                          o.s_len[sid] = bases; n_sc++; n_multi += members > 1u; n_mem += members; longest = bases > longest ? bases : longest;
                      });
    n_sc = wave_sum(n_sc); n_multi = wave_sum(n_multi); n_mem = wave_sum(n_mem); longest = wave_max(longest);
    if ((threadIdx.x & 63) == 0 && n_sc) {
        atomicAdd(&counters[SC_SCAFFOLDS], n_sc); atomicAdd(&counters[SC_MEMBERS], n_mem); atomicMax(&counters[SC_LONGEST], longest);
        if (n_multi) atomicAdd(&counters[SC_MULTI], n_multi);
    }
}

// ---- FASTA of the scaffolds ------------------------------------------------------------------------------------------------------------
// the sequence of a scaffold: its contigs in their orientation, `N` between them
struct ScSeq {
    static constexpr bool kPacked = false;
    uint32_t m;
    const int32_t *mem;               // the scaffold's contigs
    const unsigned long long *start;
    const uint32_t *col_off, *words;
    const uint8_t *orient;
    __device__ char base(uint32_t q) const {
        uint32_t lo = 0, hi = m;                                            // the last member that starts at or before q
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (start[mem[mid]] <= q) lo = mid; else hi = mid;
        }
        const uint32_t c = (uint32_t) mem[lo], c0 = col_off[c], len = col_off[c + 1] - c0;
        const unsigned long long k = q - start[c];
        if (k >= len) return 'N';
        const bool minus = orient[c] != 0;
        const uint32_t g = minus ? c0 + len - 1u - (uint32_t) k : c0 + (uint32_t) k;
        const uint32_t code = (words[g >> 4] >> (2 * (g & 15))) & 3u;
        return (char) ((0x54474341u >> (8 * (minus ? 3u - code : code))) & 0xFF);
    }
};

// `>scaffold_id=<j>_length=<s_len>_contigs=<m>\n<sequence>\n`
struct ScRecord : FastaRecord<ScSeq> {
    static constexpr bool kAligned = false;
    __device__ __forceinline__ bool set(const ScFasta &f, uint64_t j) {
        seq.m = f.s_off[j + 1] - f.s_off[j]; seq.mem = f.s_members + f.s_off[j];
        seq.start = f.start; seq.col_off = f.col_off; seq.words = f.words; seq.orient = f.orient;
        head(">scaffold_id=", j, (uint32_t) f.s_len[j]); h.f[2] = text_field("_contigs=", seq.m); seal();
        return true;
    }
};

__global__ void __launch_bounds__(SC_BLOCK) k_sc_fasta_sizes(ScFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<ScRecord>(f, f.n, sizes, counters);
}
__global__ void __launch_bounds__(SC_BLOCK) k_sc_fasta_write(ScFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ buf) {
    text_write_body<ScRecord>(f, off, i0, i1, buf);
}

}  // namespace

void launch_sc_check(const ScReads &r, const ScTargets &t, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (r.R) hipLaunchKernelGGL(k_sc_check, dim3(stage_grid(2 * r.R, SC_BLOCK, std::min<uint64_t>(4096, max_blocks))), dim3(SC_BLOCK), 0, s, r, t, counters);
}

void launch_sc_links(const ScReads &r, const ScTargets &t, int32_t max_insert, unsigned long long sentinel, unsigned long long *keys, uint32_t *vals, uint32_t *span,
                     unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (r.R && r.pair_off) hipLaunchKernelGGL(k_sc_links, dim3(stage_grid(r.R, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, r, t, max_insert, sentinel, keys, vals, span, counters);
}

void launch_sc_heads(const unsigned long long *keys, uint64_t n_links, uint32_t *heads, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (n_links) hipLaunchKernelGGL(k_sc_heads, dim3(stage_grid(n_links, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, keys, n_links, heads, counters);
}

void launch_sc_bundle_fill(const uint32_t *vals, const uint32_t *span, const uint32_t *heads, const uint32_t *pos, uint64_t n_links, uint64_t n_bundles, uint32_t *b_start,
                           unsigned long long *b_span, uint32_t max_blocks, hipStream_t s) {
    if (n_links) hipLaunchKernelGGL(k_sc_bundle_fill, dim3(stage_grid(n_links, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, vals, span, heads, pos, n_links, n_bundles, b_start, b_span);
}

void launch_sc_bundles(const unsigned long long *keys, const uint32_t *b_start, const ScBundles &b, const ScParams &p, unsigned long long *best, unsigned long long *counters,
                       uint32_t max_blocks, hipStream_t s) {
    if (b.n) hipLaunchKernelGGL(k_sc_bundles, dim3(stage_grid(b.n, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, keys, b_start, b, p, best, counters);
}

void launch_sc_second(const ScBundles &b, const unsigned long long *best, unsigned long long *second, uint32_t max_blocks, hipStream_t s) {
    if (b.n) hipLaunchKernelGGL(k_sc_second, dim3(stage_grid(b.n, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, b, best, second);
}

void launch_sc_choice(const unsigned long long *best, const unsigned long long *second, uint64_t n_ends, int32_t max_second_percent, uint32_t *choice, uint8_t *end_state,
                      unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (n_ends) hipLaunchKernelGGL(k_sc_choice, dim3(stage_grid(n_ends, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, best, second, n_ends, max_second_percent, choice, end_state, counters);
}

void launch_sc_joins(const ScBundles &b, const uint32_t *choice, uint32_t *partner, uint32_t *join_bundle, uint32_t max_blocks, hipStream_t s) {
    if (b.n) hipLaunchKernelGGL(k_sc_joins, dim3(stage_grid(b.n, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, b, choice, partner, join_bundle);
}

void launch_sc_cycle_drop(const ChainLists &l, uint32_t T, uint32_t *partner, const uint32_t *join_bundle, uint8_t *b_state, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    if (T) hipLaunchKernelGGL(k_sc_cycle_drop, dim3(stage_grid(T, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, l, T, partner, join_bundle, b_state, counters);
}

void launch_sc_rank_init(const ScTargets &t, const uint32_t *partner, const uint32_t *join_bundle, const int32_t *b_gap, int32_t min_gap, const ChainLists &l, uint32_t max_blocks, hipStream_t s) {
    if (t.T) hipLaunchKernelGGL(k_sc_rank_init, dim3(stage_grid(2ull * t.T, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, t, partner, join_bundle, b_gap, min_gap, l);
}

void launch_sc_place(const ScTargets &t, const ChainLists &l, const uint32_t *partner, const uint32_t *join_bundle, const int32_t *b_gap, const uint32_t *b_links, int32_t min_gap,
                     const ScLayout &o, uint32_t *head, uint32_t *first, uint32_t *members, unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_sc_place, dim3(stage_grid((uint64_t) t.T + 1, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, t, l, partner, join_bundle, b_gap, b_links, min_gap, o, head, first, members, counters);
}

void launch_sc_layout(const ScTargets &t, const ChainLists &l, const uint32_t *head, const uint32_t *first_scan, const uint32_t *members_scan, const ScLayout &o,
                      unsigned long long *counters, uint32_t max_blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_sc_layout, dim3(stage_grid((uint64_t) t.T + 1, SC_BLOCK, max_blocks)), dim3(SC_BLOCK), 0, s, t, l, head, first_scan, members_scan, o, counters);
}

void launch_sc_fasta_sizes(const ScFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (f.n) hipLaunchKernelGGL(k_sc_fasta_sizes, dim3(text_sizes_blocks(f.n, SC_BLOCK)), dim3(SC_BLOCK), 0, s, f, sizes, counters);
}

void launch_sc_fasta_write(const ScFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    hipLaunchKernelGGL(k_sc_fasta_write, dim3(text_write_blocks(i0, i1, SC_WAVES, f.max_blocks)), dim3(SC_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
