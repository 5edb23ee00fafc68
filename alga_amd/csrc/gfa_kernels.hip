// alga_amd/csrc/gfa_kernels.hip -- the GFA 1.0 text of an overlap graph, formatted on the GPU (include/alga_amd.h: alga_write_gfa_device).
//
// Integer work and byte movement only.  The text is a sequence of ITEMS: n_seg segment lines (one per twin pair / node, empty when the
// node is gone), then one link line per edge (empty when its twin's line stands for it).  The pipeline:
//   k_gfa_check      ids in range, list sorted by (src, dst, offset), lengths >= 0 and equal within a twin pair -> one flag word
//   k_gfa_seg_sizes  one thread per segment: the byte length of its line
//   k_gfa_link_sizes one thread per edge: the twin found by binary search in the twin source's row, the keep decision, the line length
//   64-bit scan      byte offset of every item (the file of the north-star graph is ~9 GB: 32-bit offsets do not do)
//   k_gfa_bounds     chunk k starts at the first item whose offset is >= k * step (step = chunk size - longest line: a chunk never
//                    exceeds the device buffer, and it ends at a line boundary)
//   k_gfa_seg_write  one wave per segment line: 16-byte aligned stores of the ASCII bases (2-bit codes A C G T = 0..3, 16 codes per
//                    word, low bits first), byte stores for the partial 16-byte blocks at the two ends of the line (neighbouring lines)
//   k_gfa_link_write one thread per kept edge: its own integer-to-decimal conversion
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gfa_kernels.h"

namespace alga {

namespace {

constexpr int GFA_BLOCK = 256;
constexpr int SCAN_T = 256, SCAN_K = 8, SCAN_TILE64 = SCAN_T * SCAN_K;

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
// ... of a signed one (a minus sign counts)
__device__ __forceinline__ int sdec_width(int64_t v) { return v < 0 ? 1 + dec_width((uint64_t) (-v)) : dec_width((uint64_t) v); }

__device__ __forceinline__ char *put_sdec(char *p, int64_t v) {
    uint64_t u = (uint64_t) v;
    if (v < 0) { *p++ = '-'; u = (uint64_t) (-v); }
    const int w = dec_width(u);
    for (int k = w - 1; k >= 0; k--) { p[k] = (char) ('0' + u % 10); u /= 10; }
    return p + w;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

__device__ __forceinline__ bool edge_less(const alga_edge_dev &x, const alga_edge_dev &y) {
    return x.src < y.src || (x.src == y.src && (x.dst < y.dst || (x.dst == y.dst && x.offset < y.offset)));
}

__device__ __forceinline__ uint64_t seg_line_bytes(uint64_t name, int32_t L, int seqs) {
    // S \t name \t seq \t LN:i: len \n
    return L > 0 ? 2 + dec_width(name) + 1 + (seqs ? (uint64_t) L : 1) + 6 + dec_width((uint64_t) L) + 1 : 0;
}

// > unitig_ name _length= len \n seq \n  (prefix: 8 bytes, or the 11 of ">contig_id=")
__device__ __forceinline__ uint64_t fasta_record_bytes(uint64_t name, int32_t L, int32_t min_length, uint32_t prefix) {
    return L > 0 && L >= min_length ? prefix + dec_width(name) + 8 + dec_width((uint64_t) L) + 1 + (uint64_t) L + 1 : 0;
}

__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_check(GfaCfg c, unsigned long long *__restrict__ counters) {
    const uint64_t items = c.m > (uint64_t) c.n ? c.m : (uint64_t) c.n;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (uint64_t) gridDim.x * blockDim.x) {
        if (i < c.m) {
            const alga_edge_dev x = c.e[i];
            if (x.src < 0 || x.src >= c.n || x.dst < 0 || x.dst >= c.n) bad |= GFA_BAD_ID;
            if (i > 0 && edge_less(x, c.e[i - 1])) bad |= GFA_BAD_ORDER;
        }
        if (i < (uint64_t) c.n) {
            const int32_t L = c.len[i];
            if (L < 0) bad |= GFA_BAD_LEN;
            if (c.twins && (i & 1) && c.len[i - 1] != L) bad |= GFA_BAD_TWIN;
        }
    }
    if (bad) atomicOr(&counters[GFA_FLAGS], bad);
}

__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_seg_sizes(GfaCfg c, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long live = 0, bytes = 0;
    if (j < c.n_seg) {
        const int32_t L = c.len[c.twins ? 2 * j + 1 : j];
        bytes = c.fasta ? fasta_record_bytes(c.rec_rank ? c.rec_rank[j] : j, L, c.min_length, c.rec_rank ? 11u : 8u) : seg_line_bytes(j, L, c.seqs);
        live = bytes > 0;
        sizes[j] = (uint32_t) bytes;
    }
    live = wave_sum(live);
    bytes = wave_max(bytes);
    if ((threadIdx.x & 63) == 0 && live) {
        atomicAdd(&counters[GFA_SEGMENTS], live);
        atomicMax(&counters[GFA_MAX_LINE], bytes);
    }
}

__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_link_sizes(GfaCfg c, const uint32_t *__restrict__ rowptr, uint32_t *__restrict__ sizes,
                                                              unsigned long long *__restrict__ counters) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long kept = 0, merged = 0, bytes = 0;
    if (i < c.m) {
        const alga_edge_dev x = c.e[i];
        bool keep = true;
        if (c.twins) {
            const int32_t ts = x.dst ^ 1, td = x.src ^ 1;
            if (ts < x.src || (ts == x.src && td < x.dst)) {          // only a twin that sorts first can take the line
                const int32_t to = c.len[x.dst] - c.len[x.src] + x.offset;
                uint32_t lo = rowptr[ts], hi = rowptr[ts + 1];
                while (lo < hi) {                                     // the row is sorted by (dst, offset)
                    const uint32_t mid = (lo + hi) >> 1;
                    const alga_edge_dev y = c.e[mid];
                    if (y.dst < td || (y.dst == td && y.offset < to)) lo = mid + 1; else hi = mid;
                }
                keep = !(lo < rowptr[ts + 1] && c.e[lo].dst == td && c.e[lo].offset == to);
            }
        }
        if (keep) {
            const uint64_t na = c.twins ? (uint64_t) (x.src >> 1) : (uint64_t) x.src, nb = c.twins ? (uint64_t) (x.dst >> 1) : (uint64_t) x.dst;
            // L \t na \t o \t nb \t o \t overlap M \n
            bytes = 10 + dec_width(na) + dec_width(nb) + sdec_width((int64_t) c.len[x.src] - x.offset);
            kept = 1;
        } else merged = 1;
        sizes[c.n_seg + i] = (uint32_t) bytes;
    }
    kept = wave_sum(kept);
    merged = wave_sum(merged);
    bytes = wave_max(bytes);
    if ((threadIdx.x & 63) == 0 && (kept || merged)) {
        if (kept) atomicAdd(&counters[GFA_LINKS], kept);
        if (merged) atomicAdd(&counters[GFA_MERGED], merged);
        atomicMax(&counters[GFA_MAX_LINE], bytes);
    }
}

// ---- 64-bit exclusive scan: tile sums -> one-workgroup spine -> per-tile scan ----------------------------------------------------
__device__ __forceinline__ unsigned long long block_exscan64(unsigned long long v, unsigned long long *lds /* SCAN_T / 64 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned long long off = 0;
    for (int w = 0; w < wave; w++) off += lds[w];
    return off + inc - v;
}

__global__ void __launch_bounds__(SCAN_T) k_gfa_scan_tiles(const uint32_t *__restrict__ in, uint64_t n, unsigned long long *__restrict__ tiles) {
    __shared__ unsigned long long lds[SCAN_T / 64];
    const uint64_t base = (uint64_t) blockIdx.x * SCAN_TILE64;
    unsigned long long s = 0;
    for (int k = 0; k < SCAN_K; k++) { const uint64_t i = base + (uint64_t) k * SCAN_T + threadIdx.x; if (i < n) s += in[i]; }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long t = 0; for (int w = 0; w < SCAN_T / 64; w++) t += lds[w]; tiles[blockIdx.x] = t; }
}

__global__ void __launch_bounds__(1024) k_gfa_scan_spine(unsigned long long *tiles, uint64_t n_tiles) {
    __shared__ unsigned long long lds[1024 / 64];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t base = 0; base < n_tiles; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long v = i < n_tiles ? tiles[i] : 0;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        unsigned long long inc = v;
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane == 63) lds[wave] = inc;
        __syncthreads();
        unsigned long long off = carry;
        for (int w = 0; w < wave; w++) off += lds[w];
        if (i < n_tiles) tiles[i] = off + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = off + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) tiles[n_tiles] = carry;
}

// thread t of tile b scans the SCAN_K consecutive items base + t * SCAN_K ..
__global__ void __launch_bounds__(SCAN_T) k_gfa_scan_down(const uint32_t *__restrict__ in, uint64_t n, const unsigned long long *__restrict__ tiles,
                                                          unsigned long long *__restrict__ out) {
    __shared__ unsigned long long lds[SCAN_T / 64];
    const uint64_t base = (uint64_t) blockIdx.x * SCAN_TILE64 + (uint64_t) threadIdx.x * SCAN_K;
    uint32_t v[SCAN_K];
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_K; k++) { v[k] = base + k < n ? in[base + k] : 0; s += v[k]; }
    unsigned long long ex = block_exscan64(s, lds) + tiles[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_K; k++) { if (base + k < n) out[base + k] = ex; ex += v[k]; }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = tiles[gridDim.x];
}

__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_bounds(const unsigned long long *__restrict__ off, uint64_t n, uint64_t step, uint64_t K,
                                                          unsigned long long *__restrict__ bounds) {
    const uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k > K) return;
    uint64_t b;
    if (k == 0) b = 0;
    else if (k == K) b = n;
    else {
        const unsigned long long want = (unsigned long long) k * step;
        uint64_t lo = 0, hi = n;                                      // first i in [0, n] with off[i] >= want (off[n] = total >= want)
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] < want) lo = mid + 1; else hi = mid; }
        b = lo;
    }
    bounds[k] = b;
    bounds[K + 1 + k] = off[b];
}

// byte p of a segment line: "S\t" name "\t" seq "\tLN:i:" len "\n"; of a FASTA record: ">unitig_" name "_length=" len "\n" seq "\n"
// CONTIG: the FASTA of a contig result (">contig_id=" and the record's rank as its name); false: the code as it was before that form existed
template <bool CONTIG> struct SegLine {
    uint64_t name; int32_t L; int wn, wl; uint32_t hp, sl;           // hp = bytes before the sequence, sl = bytes of the sequence field
    const uint32_t *row; int seqs;
    int fasta; uint32_t q0;                                           // FASTA: the sequence starts at base q0 of the row
    __device__ __forceinline__ char digit(uint64_t v, int w, int d) const { return (char) ('0' + (v / kPow10[w - 1 - d]) % 10); }
    __device__ __forceinline__ char base(uint32_t q) const { q += q0; return (char) ((0x54474341u >> (8 * ((row[q >> 4] >> (2 * (q & 15))) & 3))) & 0xFF); }
    __device__ char at(uint32_t p) const {
        if (fasta) {
            constexpr uint32_t fp = CONTIG ? 11u : 8u;
            if (p < fp) return CONTIG ? ">contig_id="[p] : ">unitig_"[p];
            if (p < fp + wn) return digit(name, wn, (int) (p - fp));
            if (p < fp + 8u + wn) return "_length="[p - fp - wn];
            if (p + 1 < hp) return digit((uint64_t) L, wl, (int) (p - fp - 8 - wn));
            if (p < hp) return '\n';
            return p - hp < sl ? base(p - hp) : '\n';
        }
        if (p < hp) return p < 2 ? (p == 0 ? 'S' : '\t') : (p < 2u + wn ? digit(name, wn, (int) p - 2) : '\t');
        const uint32_t q = p - hp;
        if (q < sl) return seqs ? base(q) : '*';
        const uint32_t r = q - sl;
        if (r < 6) return "\tLN:i:"[r];
        return r < 6u + wl ? digit((uint64_t) L, wl, (int) r - 6) : '\n';
    }
    // 16 bases from sequence index q (all inside the sequence) as 4 little-endian words of ASCII
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

// one wave per segment item in [i0, i1) (items below n_seg); buf + off[j] - base is the line's first byte
template <bool CONTIG> __global__ void __launch_bounds__(GFA_BLOCK) k_gfa_seg_write(GfaCfg c, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1,
                                                             char *__restrict__ buf) {
    const int lane = threadIdx.x & 63;
    const uint64_t base = off[i0];
    const uint64_t waves = (uint64_t) gridDim.x * (blockDim.x >> 6);
    for (uint64_t j = i0 + (uint64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < i1; j += waves) {
        const uint64_t l0 = off[j], l1 = off[j + 1];
        if (l0 == l1) continue;
        const uint64_t node = c.twins ? 2 * j + 1 : j;
        SegLine<CONTIG> s;
        s.name = CONTIG ? c.rec_rank[j] : j; s.L = c.len[node]; s.wn = dec_width(s.name); s.wl = dec_width((uint64_t) s.L);
        s.hp = c.fasta ? (CONTIG ? 11 : 8) + s.wn + 8 + s.wl + 1 : 2 + s.wn + 1; s.sl = c.seqs ? (uint32_t) s.L : 1u;
        s.row = c.row(node); s.seqs = c.seqs;
        s.fasta = c.fasta; s.q0 = c.fasta ? (uint32_t) c.seq_off[j] : 0u;
        char *g0 = buf + (l0 - base), *g1 = buf + (l1 - base);
        char *a0 = (char *) (((uintptr_t) g0 + 15) & ~(uintptr_t) 15), *a1 = (char *) ((uintptr_t) g1 & ~(uintptr_t) 15);
        if (a0 >= a1) {                                               // no whole aligned block inside the line
            for (char *p = g0 + lane; p < g1; p += 64) *p = s.at((uint32_t) (p - g0));
            continue;
        }
        if (g0 + lane < a0) g0[lane] = s.at((uint32_t) lane);         // < 16 bytes before the first aligned block, < 16 after the last
        if (a1 + lane < g1) a1[lane] = s.at((uint32_t) (a1 - g0) + lane);
        const uint64_t nblk = (uint64_t) (a1 - a0) >> 4;
        for (uint64_t q = lane; q < nblk; q += 64) {
            const uint32_t p = (uint32_t) (a0 - g0) + (uint32_t) (q << 4);
            uint4 v;
            if (s.seqs && p >= s.hp && p + 16 <= s.hp + s.sl) v = s.bases16(p - s.hp);
            else {
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

// one thread per link item in [i0, i1) (items from n_seg on)
__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_link_write(GfaCfg c, const unsigned long long *__restrict__ off, uint64_t chunk_i0, uint64_t i0,
                                                              uint64_t i1, char *__restrict__ buf) {
    const uint64_t i = i0 + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= i1) return;
    const uint64_t base = off[chunk_i0], l0 = off[i];
    if (l0 == off[i + 1]) return;
    const alga_edge_dev x = c.e[i - c.n_seg];
    char *p = buf + (l0 - base);
    *p++ = 'L'; *p++ = '\t';
    p = put_sdec(p, c.twins ? (x.src >> 1) : x.src);
    *p++ = '\t'; *p++ = (!c.twins || (x.src & 1)) ? '+' : '-'; *p++ = '\t';
    p = put_sdec(p, c.twins ? (x.dst >> 1) : x.dst);
    *p++ = '\t'; *p++ = (!c.twins || (x.dst & 1)) ? '+' : '-'; *p++ = '\t';
    p = put_sdec(p, (int64_t) c.len[x.src] - x.offset);
    *p++ = 'M'; *p = '\n';
}

inline unsigned grid_of(uint64_t items, int per_block) { return (unsigned) ((items + per_block - 1) / per_block); }

}  // namespace

void launch_gfa_check(const GfaCfg &c, unsigned long long *counters, hipStream_t s) {
    const uint64_t items = c.m > (uint64_t) c.n ? c.m : (uint64_t) c.n;
    if (!items) return;
    const uint64_t g = (items + GFA_BLOCK - 1) / GFA_BLOCK;
    hipLaunchKernelGGL(k_gfa_check, dim3((unsigned) (g < 65536 ? g : 65536)), dim3(GFA_BLOCK), 0, s, c, counters);
}

void launch_gfa_sizes(const GfaCfg &c, const uint32_t *rowptr, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (c.n_seg) hipLaunchKernelGGL(k_gfa_seg_sizes, dim3(grid_of(c.n_seg, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, c, sizes, counters);
    if (c.m) hipLaunchKernelGGL(k_gfa_link_sizes, dim3(grid_of(c.m, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, c, rowptr, sizes, counters);
}

size_t gfa_scan_tiles(uint64_t n) { return (size_t) ((n + SCAN_TILE64 - 1) / SCAN_TILE64); }

void launch_gfa_scan64(const uint32_t *sizes, uint64_t n, unsigned long long *off, unsigned long long *tiles, hipStream_t s) {
    const uint64_t nt = gfa_scan_tiles(n);
    if (!nt) { (void) hipMemsetAsync(off, 0, sizeof(unsigned long long), s); return; }
    hipLaunchKernelGGL(k_gfa_scan_tiles, dim3((unsigned) nt), dim3(SCAN_T), 0, s, sizes, n, tiles);
    hipLaunchKernelGGL(k_gfa_scan_spine, dim3(1), dim3(1024), 0, s, tiles, nt);
    hipLaunchKernelGGL(k_gfa_scan_down, dim3((unsigned) nt), dim3(SCAN_T), 0, s, sizes, n, (const unsigned long long *) tiles, off);
}

void launch_gfa_bounds(const unsigned long long *off, uint64_t n, uint64_t step, uint64_t K, unsigned long long *bounds, hipStream_t s) {
    hipLaunchKernelGGL(k_gfa_bounds, dim3(grid_of(K + 1, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, off, n, step, K, bounds);
}

void launch_gfa_format(const GfaCfg &c, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    const uint64_t s1 = i1 < c.n_seg ? i1 : c.n_seg;
    if (i0 < s1) {
        const uint64_t g = grid_of(s1 - i0, GFA_BLOCK / 64);
        if (c.fasta && c.rec_rank) hipLaunchKernelGGL(k_gfa_seg_write<true>, dim3((unsigned) (g < 16384 ? g : 16384)), dim3(GFA_BLOCK), 0, s, c, off, i0, s1, buf);
        else hipLaunchKernelGGL(k_gfa_seg_write<false>, dim3((unsigned) (g < 16384 ? g : 16384)), dim3(GFA_BLOCK), 0, s, c, off, i0, s1, buf);
    }
    const uint64_t l0 = i0 > c.n_seg ? i0 : c.n_seg;
    if (l0 < i1) {
        // the chunk's bytes start at off[i0]: its link lines are placed relative to that
        hipLaunchKernelGGL(k_gfa_link_write, dim3(grid_of(i1 - l0, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, c, off, i0, l0, i1, buf);
    }
}

}  // namespace alga
