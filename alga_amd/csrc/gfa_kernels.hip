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
//   k_gfa_fasta_sizes / k_gfa_fasta_write   the consensus windows as FASTA records (GfaFasta), through the same scan and bounds
// A segment line and a FASTA record are record types of text_record.h: the sizes and write kernels are its two bodies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gfa_kernels.h"
#include "text_record.h"

namespace alga {

namespace {

constexpr int GFA_BLOCK = 256;
constexpr int SCAN_T = 256, SCAN_K = 8, SCAN_TILE64 = SCAN_T * SCAN_K;

// decimal width of a signed value (a minus sign counts)
__device__ __forceinline__ int sdec_width(int64_t v) { return v < 0 ? 1 + dec_width((uint64_t) (-v)) : dec_width((uint64_t) v); }

__device__ __forceinline__ char *put_sdec(char *p, int64_t v) {
    uint64_t u = (uint64_t) v;
    if (v < 0) { *p++ = '-'; u = (uint64_t) (-v); }
    const int w = dec_width(u);
    for (int k = w - 1; k >= 0; k--) { p[k] = (char) ('0' + u % 10); u /= 10; }
    return p + w;
}

__device__ __forceinline__ bool edge_less(const alga_edge_dev &x, const alga_edge_dev &y) {
    return x.src < y.src || (x.src == y.src && (x.dst < y.dst || (x.dst == y.dst && x.offset < y.offset)));
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

// "S\t" name "\t" seq "\tLN:i:" len "\n"; seq is `*` without ALGA_GFA_SEQUENCES
struct SegLine {
    static constexpr bool kPacked = true, kAligned = true;
    TextHeader<2> h; TextHeader<1> t;                                 // before and after the sequence (h's newline is never reached)
    uint32_t hp, sl; int seqs;                                        // hp = bytes before the sequence, sl = bytes of the sequence field
    PackedSeq seq;
    __device__ __forceinline__ bool set(const GfaCfg &c, uint64_t j) {
        const uint64_t node = c.twins ? 2 * j + 1 : j;
        const int32_t L = c.len[node];
        if (L <= 0) return false;
        h.f[0] = text_field("S\t", j); h.f[1] = text_lit("\t"); t.f[0] = text_field("\tLN:i:", (uint64_t) L);
        hp = h.bytes() - 1u; seqs = c.seqs; sl = seqs ? (uint32_t) L : 1u;
        seq.row = c.row(node); seq.q0 = 0;
        return true;
    }
    __device__ __forceinline__ uint32_t bytes() const { return hp + sl + t.bytes(); }
    __device__ __forceinline__ char at(uint32_t p) const {
        if (p < hp) return h.at(p);
        const uint32_t q = p - hp;
        if (q < sl) return seqs ? seq.base(q) : '*';
        return t.at(q - sl);
    }
    __device__ __forceinline__ uint32_t packed() const { return seqs ? sl : 0u; }
    __device__ __forceinline__ uint4 bases16(uint32_t q) const { return seq.bases16(q); }
};

// `>unitig_<j>_length=<len>` or, of a contig result, `>contig_id=<rank>_length=<len>`, then the window of row j
struct WindowRecord : FastaRecord<PackedSeq> {
    __device__ __forceinline__ bool window(const GfaFasta &f, uint64_t j) {
        const int32_t len = f.len[j];
        seq.row = f.words + f.row_off[j]; seq.q0 = (uint32_t) f.seq_off[j];
        L = (uint32_t) len;
        return len > 0 && len >= f.min_length;
    }
};
struct UnitigRecord : WindowRecord {
    __device__ __forceinline__ bool set(const GfaFasta &f, uint64_t j) {
        if (!window(f, j)) return false;
        head(">unitig_", j, L); seal();
        return true;
    }
};
struct ContigRecord : WindowRecord {
    __device__ __forceinline__ bool set(const GfaFasta &f, uint64_t j) {
        if (!window(f, j)) return false;
        contig_head(f.rec_rank[j], L); seal();
        return true;
    }
};

__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_seg_sizes(GfaCfg c, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<SegLine>(c, c.n_seg, sizes, counters);
}
// items in [i0, i1) (items below n_seg)
__global__ void __launch_bounds__(GFA_BLOCK) k_gfa_seg_write(GfaCfg c, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1,
                                                             char *__restrict__ buf) {
    text_write_body<SegLine>(c, off, i0, i1, buf);
}

template <class R> __global__ void __launch_bounds__(GFA_BLOCK) k_gfa_fasta_sizes(GfaFasta f, uint32_t *__restrict__ sizes, unsigned long long *__restrict__ counters) {
    text_sizes_body<R>(f, f.n, sizes, counters);
}
template <class R> __global__ void __launch_bounds__(GFA_BLOCK) k_gfa_fasta_write(GfaFasta f, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1,
                                                                                  char *__restrict__ buf) {
    text_write_body<R>(f, off, i0, i1, buf);
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
    if (c.n_seg) hipLaunchKernelGGL(k_gfa_seg_sizes, dim3(text_sizes_blocks(c.n_seg, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, c, sizes, counters);
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
    if (i0 < s1) hipLaunchKernelGGL(k_gfa_seg_write, dim3(text_write_blocks(i0, s1, GFA_BLOCK / 64)), dim3(GFA_BLOCK), 0, s, c, off, i0, s1, buf);
    const uint64_t l0 = i0 > c.n_seg ? i0 : c.n_seg;
    if (l0 < i1) {
        // the chunk's bytes start at off[i0]: its link lines are placed relative to that
        hipLaunchKernelGGL(k_gfa_link_write, dim3(grid_of(i1 - l0, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, c, off, i0, l0, i1, buf);
    }
}

void launch_gfa_fasta_sizes(const GfaFasta &f, uint32_t *sizes, unsigned long long *counters, hipStream_t s) {
    if (!f.n) return;
    if (f.rec_rank) hipLaunchKernelGGL(k_gfa_fasta_sizes<ContigRecord>, dim3(text_sizes_blocks(f.n, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, f, sizes, counters);
    else hipLaunchKernelGGL(k_gfa_fasta_sizes<UnitigRecord>, dim3(text_sizes_blocks(f.n, GFA_BLOCK)), dim3(GFA_BLOCK), 0, s, f, sizes, counters);
}

void launch_gfa_fasta_write(const GfaFasta &f, const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) {
    if (i0 >= i1) return;
    const dim3 grid(text_write_blocks(i0, i1, GFA_BLOCK / 64));
    if (f.rec_rank) hipLaunchKernelGGL(k_gfa_fasta_write<ContigRecord>, grid, dim3(GFA_BLOCK), 0, s, f, off, i0, i1, buf);
    else hipLaunchKernelGGL(k_gfa_fasta_write<UnitigRecord>, grid, dim3(GFA_BLOCK), 0, s, f, off, i0, i1, buf);
}

}  // namespace alga
