// alga_amd/csrc/text_record.h -- device code of every text record the engine writes (GFA segment lines and all FASTA outputs): what a
// record is and how a wave writes it.  Included by the *_kernels.hip files only; everything here is internal to the including file (the
// build has no relocatable device code, so each file gets its own copy of the table).
//
// A record is `header, sequence, what follows the sequence`.  A record type R supplies
//   bool     set(const Src &, uint64_t j)   fills the record of item j; false: the item is not written (and nothing else may be asked of it)
//   uint32_t bytes()                        the record's length
//   char     at(uint32_t p)                 its byte p
//   R::kAligned                             true: written in 16-byte aligned blocks; false: byte by byte, a lane a byte
//   R::kPacked, and if it is true: hp, packed(), bases16(q): bytes [hp, hp + packed()) are bases q = 0 .. of a PackedSeq
// and the two bodies below do the rest: text_sizes_body (one thread per item) and text_write_body (one wave per record).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gfa_kernels.h"

namespace alga {

namespace {

__device__ __constant__ uint64_t kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
                                               1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull,
                                               100000000000000ull, 1000000000000000ull, 10000000000000000ull, 100000000000000000ull,
                                               1000000000000000000ull, 10000000000000000000ull};

// decimal width of a non-negative value
__device__ __forceinline__ int dec_width(uint64_t v) {
    int w = 1;
    while (w < 20 && v >= kPow10[w]) w++;
    return w;
}
// digit d (0 = the first) of v written in `width` digits; one 32-bit division where both operands fit
__device__ __forceinline__ char dec_digit(uint64_t v, uint32_t width, uint32_t d) {
    const uint64_t p = kPow10[width - 1 - d];
    if (((v | p) >> 32) == 0) return (char) ('0' + ((uint32_t) v / (uint32_t) p) % 10u);
    return (char) ('0' + (v / p) % 10ull);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// bases q0 .. of a row of 2-bit codes (A C G T = 0..3, 16 codes per word, low bits first) as ASCII
struct PackedSeq {
    static constexpr bool kPacked = true;
    const uint32_t *row; uint32_t q0;
    __device__ __forceinline__ char base(uint32_t q) const { q += q0; return (char) ((0x54474341u >> (8 * ((row[q >> 4] >> (2 * (q & 15))) & 3))) & 0xFF); }
    // 16 bases from sequence index q (all inside the sequence: row[w + 1] is read when q0 + q is no multiple of 16) as 4 little-endian words
    __device__ __forceinline__ uint4 bases16(uint32_t q) const {
        q += q0;
        const uint32_t w = q >> 4, sh = q & 15;
        uint32_t codes = row[w];
        if (sh) codes = (uint32_t) ((((uint64_t) row[w + 1] << 32) | codes) >> (2 * sh));
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) x |= ((0x54474341u >> (8 * ((codes >> (2 * (4 * k + b))) & 3))) & 0xFFu) << (8 * b);
            o[k] = x;
        }
        return make_uint4(o[0], o[1], o[2], o[3]);
    }
};

// one field of a header: a literal, then (w > 0) a value in w decimal digits
struct TextField {
    const char *lit = nullptr; uint32_t nlit = 0; uint32_t w = 0; uint64_t v = 0;
};
template <uint32_t N> __device__ __forceinline__ TextField text_lit(const char (&lit)[N]) { return TextField{lit, N - 1, 0, 0}; }
template <uint32_t N> __device__ __forceinline__ TextField text_field(const char (&lit)[N], uint64_t v) { return TextField{lit, N - 1, (uint32_t) dec_width(v), v}; }
// ... in exactly w digits, padded with zeros (v < 10^w)
template <uint32_t N> __device__ __forceinline__ TextField text_fixed(const char (&lit)[N], uint64_t v, uint32_t w) { return TextField{lit, N - 1, w, v}; }

// N fields and a newline.  The walks are unrolled: an index known at compile time keeps the fields in registers.
template <int N> struct TextHeader {
    TextField f[N];
    __device__ __forceinline__ uint32_t bytes() const {
        uint32_t b = 1;
#pragma unroll
        for (int i = 0; i < N; i++) b += f[i].nlit + f[i].w;
        return b;
    }
    __device__ __forceinline__ char at(uint32_t p) const {
        // p lies in at most one field: left of a field p - at0 wraps around and matches nothing.  A digit is taken after the walk, so
        // that the division is there once.
        uint64_t v = 0; uint32_t w = 0, d = 0, at0 = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (p - at0 < f[i].nlit) return f[i].lit[p - at0];
            at0 += f[i].nlit;
            if (p - at0 < f[i].w) { v = f[i].v; w = f[i].w; d = p - at0; }
            at0 += f[i].w;
        }
        return w ? dec_digit(v, w, d) : '\n';
    }
};

// `<header>\n<sequence>\n`; Seq: base(q) and kPacked, a packed one bases16(q) as well.  A set() ends with seal().
template <class Seq> struct FastaRecord {
    static constexpr bool kPacked = Seq::kPacked, kAligned = true;
    TextHeader<5> h;
    uint32_t hp, L;                                                   // bytes before the sequence, its length
    Seq seq;
    // `<prefix><id>_length=<len>`, what every header starts with
    template <uint32_t N> __device__ __forceinline__ void head(const char (&prefix)[N], uint64_t id, uint32_t len) {
        h.f[0] = text_field(prefix, id); h.f[1] = text_field("_length=", len); L = len;
    }
    __device__ __forceinline__ void contig_head(uint64_t id, uint32_t len) { head(">contig_id=", id, len); }
    // `_reads=<n>_depth=<q>.<dd>`: q.dd = floor(100 * bases / L) / 100, without a product above 2^64
    __device__ __forceinline__ void depth(uint64_t reads, uint64_t bases) {
        h.f[2] = text_field("_reads=", reads); h.f[3] = text_field("_depth=", bases / L); h.f[4] = text_fixed(".", ((bases % L) * 100ull) / L, 2);
    }
    __device__ __forceinline__ void seal() { hp = h.bytes(); }
    __device__ __forceinline__ uint32_t bytes() const { return hp + L + 1u; }
    __device__ __forceinline__ char at(uint32_t p) const { return p < hp ? h.at(p) : (p - hp < L ? seq.base(p - hp) : '\n'); }
    __device__ __forceinline__ uint32_t packed() const { return L; }
    __device__ __forceinline__ uint4 bases16(uint32_t q) const { return seq.bases16(q); }
};

// One thread per item j < n: sizes[j] = the bytes of its record (0: not written); the live records and the longest one into the counters.
template <class R, class Src> __device__ __forceinline__ void text_sizes_body(const Src &src, uint64_t n, uint32_t *__restrict__ sizes,
                                                                              unsigned long long *__restrict__ counters) {
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long live = 0, bytes = 0;
    if (j < n) {
        R r;
        if (r.set(src, j)) { bytes = r.bytes(); live = 1; }
        sizes[j] = (uint32_t) bytes;
    }
    live = wave_sum(live);
    bytes = wave_max(bytes);
    if ((threadIdx.x & 63) == 0 && live) {
        atomicAdd(&counters[GFA_SEGMENTS], live);
        atomicMax(&counters[GFA_MAX_LINE], bytes);
    }
}

// One wave per item in [i0, i1); buf + off[j] - off[i0] is the first byte of record j.  An aligned record type: 16-byte aligned stores, a block
// that lies inside a packed sequence comes from bases16, any other is put together from at(); byte stores for the partial blocks at the two
// ends of the record (they belong to the neighbouring records as well).
template <class R, class Src> __device__ __forceinline__ void text_write_body(const Src &src, const unsigned long long *__restrict__ off, uint64_t i0,
                                                                              uint64_t i1, char *__restrict__ buf) {
    const int lane = threadIdx.x & 63;
    const uint64_t base = off[i0];
    const uint64_t waves = (uint64_t) gridDim.x * (blockDim.x >> 6);
    // the wave's number is the same in all its lanes: said so, what depends on the record alone is kept in scalar registers
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    for (uint64_t j = i0 + (uint64_t) blockIdx.x * (blockDim.x >> 6) + wave; j < i1; j += waves) {
        const uint64_t l0 = off[j], l1 = off[j + 1];
        if (l0 == l1) continue;
        R s;
        s.set(src, j);
        char *g0 = buf + (l0 - base), *g1 = buf + (l1 - base);
        char *a0 = (char *) (((uintptr_t) g0 + 15) & ~(uintptr_t) 15), *a1 = (char *) ((uintptr_t) g1 & ~(uintptr_t) 15);
        if (!R::kAligned || a0 >= a1) {                               // ... or no whole aligned block inside the record
            for (char *p = g0 + lane; p < g1; p += 64) *p = s.at((uint32_t) (p - g0));
            continue;
        }
        if (g0 + lane < a0) g0[lane] = s.at((uint32_t) lane);         // < 16 bytes before the first aligned block, < 16 after the last
        if (a1 + lane < g1) a1[lane] = s.at((uint32_t) (a1 - g0) + lane);
        const uint64_t nblk = (uint64_t) (a1 - a0) >> 4;
        for (uint64_t q = lane; q < nblk; q += 64) {
            const uint32_t p = (uint32_t) (a0 - g0) + (uint32_t) (q << 4);
            uint4 v;
            bool done = false;
            if constexpr (R::kPacked) {
                if (p >= s.hp && p + 16 <= s.hp + s.packed()) { v = s.bases16(p - s.hp); done = true; }
            }
            if (!done) {
                uint32_t o[4];
                for (int k = 0; k < 4; k++) {
                    uint32_t x = 0;
                    for (int b = 0; b < 4; b++) x |= (uint32_t) (uint8_t) s.at(p + 4 * k + b) << (8 * b);
                    o[k] = x;
                }
                v = make_uint4(o[0], o[1], o[2], o[3]);
            }
            *reinterpret_cast<uint4 *>(a0 + (q << 4)) = v;
        }
    }
}

// ---- the grids of a *_sizes / *_write kernel pair (host)
// text_sizes_body has one thread per item and no loop: its grid is exact (n > 0)
inline unsigned text_sizes_blocks(uint64_t n, int block) { return (unsigned) ((n + (uint64_t) block - 1) / (uint64_t) block); }
// text_write_body strides by waves: a wave per record of [i0, i1) (i0 < i1), at most `cap` blocks
inline unsigned text_write_blocks(uint64_t i0, uint64_t i1, int waves_per_block, uint64_t cap = 16384) {
    const uint64_t g = (i1 - i0 + (uint64_t) waves_per_block - 1) / (uint64_t) waves_per_block;
    return (unsigned) (g < cap ? g : cap);
}

}  // namespace

}  // namespace alga
