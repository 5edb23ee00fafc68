// alga_amd/csrc/engine_gfa.hip -- C ABI of the GFA 1.0 export (include/alga_amd.h: alga_write_gfa_device; kernels in gfa_kernels.hip).
//
// Host side: two small read-backs before any byte of text exists (the device's verdict on the input; then the line count, the
// longest line and the total size with the chunk bounds), then one loop over the chunks: the device formats chunk k into its buffer,
// the buffer goes down into pinned host buffer k % 2, and a host thread pwrite()s it at its file offset while the device formats
// chunk k + 1.  The only wait per chunk is the main thread's for the write of chunk k - 2 (whose pinned buffer chunk k reuses).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <cstring>
#include <future>
#include <vector>

#include "engine_internal.h"
#include "contig_kernels.h"
#include "gfa_kernels.h"
#include "simplify_kernels.h"

using namespace alga;

namespace {

const char kGfaHeader[] = "H\tVN:Z:1.0\n";

bool write_all(int fd, const char *p, size_t bytes, uint64_t at) {
    while (bytes) {
        const ssize_t w = pwrite(fd, p, bytes, (off_t) at);
        if (w <= 0) return false;
        p += w; bytes -= (size_t) w; at += (uint64_t) w;
    }
    return true;
}

int gfa_impl(alga_engine *e, const AlgaTextJob &job, const char *path, alga_gfa_info *info, int &fd) {
    hipStream_t s = e->own_stream;
    const uint64_t N = job.items;
    int rc;
    AlgaEvents<12> evs;
    // [0, 1] checks .. scan, [2, 3] the copies' ends (one per pinned slot), [4 + 2 * (k % 4), 5 + 2 * (k % 4)] the formatting of chunk k
    // (read back once the write of chunk k is done, two chunks later: four pairs are never overwritten before that)
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->counters, GFA_COUNTERS * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->gfa_sizes, (size_t) (N + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gfa_off, (size_t) (N + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->gfa_tiles, (gfa_scan_tiles(N) + 1) * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->counters.p, *off = (unsigned long long *) e->gfa_off.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, GFA_COUNTERS * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    if (job.prepare && (rc = job.prepare(cnt, s))) return rc;
    job.sizes((uint32_t *) e->gfa_sizes.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_gfa_sizes"))) return rc;
    launch_gfa_scan64((const uint32_t *) e->gfa_sizes.p, N, off, (unsigned long long *) e->gfa_tiles.p, s);
    if ((rc = alga_check_launch(e, "gfa scan"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, GFA_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + GFA_COUNTERS, off + N, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIP_TRY(e, hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1]));
    double ms_format = ms;
    if (job.verdict && (rc = job.verdict(e->h_counters))) return rc;
    const uint64_t total = e->h_counters[GFA_COUNTERS], max_line = e->h_counters[GFA_MAX_LINE], head = strlen(job.head);
    if (info) {
        info->segments = e->h_counters[GFA_SEGMENTS]; info->links = e->h_counters[GFA_LINKS]; info->links_merged = e->h_counters[GFA_MERGED];
        info->bytes = head + total;
    }
    // chunks: step = cap - longest line, so that no chunk exceeds cap and each ends at a line boundary
    uint64_t cap = (uint64_t) e->opt_gfa_chunk_mb << 20;
    if (cap < 2 * max_line) cap = (2 * max_line + 4095) & ~4095ull;
    const uint64_t step = cap - max_line, K = total ? (total + step - 1) / step : 0;
    std::vector<unsigned long long> bounds(2 * (size_t) (K + 1));
    if (K) {
        if ((rc = alga_ensure(e, e->gfa_bounds, bounds.size() * sizeof(unsigned long long)))) return rc;
        launch_gfa_bounds(off, N, step, K, (unsigned long long *) e->gfa_bounds.p, s);
        if ((rc = alga_check_launch(e, "k_gfa_bounds"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(bounds.data(), e->gfa_bounds.p, bounds.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        if ((rc = alga_ensure(e, e->gfa_buf, (size_t) cap))) return rc;
        if (e->gfa_pin_cap < cap) {
            for (void *&p : e->gfa_pin) { if (p) HIP_TRY(e, hipHostFree(p)); p = nullptr; }
            e->gfa_pin_cap = 0;
            for (void *&p : e->gfa_pin) HIP_TRY(e, hipHostMalloc(&p, (size_t) cap));
            e->gfa_pin_cap = cap;
        }
    }
    fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    auto io_fail = [&](const char *verb) { return alga_fail(e, ALGA_ERR_IO, (std::string("cannot ") + verb + " the " + job.kind + " file").c_str()); };
    if (fd < 0) return io_fail("create");
    if (head && !write_all(fd, job.head, head, 0)) return io_fail("write");
    std::future<bool> writer[2];
    int pending_fmt[2] = {-1, -1};                                 // event pair of the chunk the slot holds, -1 none
    bool io_ok = true;
    auto finish_slot = [&](int slot) -> int {                      // the write that last used pinned buffer `slot` is done; its format time counted
        if (writer[slot].valid()) io_ok = writer[slot].get() && io_ok;
        if (pending_fmt[slot] >= 0) {
            float t = 0.0f;
            HIP_TRY(e, hipEventElapsedTime(&t, evs.ev[(size_t) (4 + 2 * pending_fmt[slot])], evs.ev[(size_t) (5 + 2 * pending_fmt[slot])]));
            ms_format += t;
            pending_fmt[slot] = -1;
        }
        return ALGA_OK;
    };
    char *dbuf = (char *) e->gfa_buf.p;
    int slot = 0, pair = 0;
    for (uint64_t k = 0; k < K && rc == ALGA_OK && io_ok; k++) {
        const uint64_t i0 = bounds[(size_t) k], i1 = bounds[(size_t) k + 1];
        const uint64_t b0 = bounds[(size_t) (K + 1 + k)], bytes = bounds[(size_t) (K + 2 + k)] - b0;
        if (!bytes) continue;
        // the formatting of chunk k runs behind the copy of chunk k - 1 (same stream, one device buffer)
        HIP_TRY(e, hipEventRecord(evs.ev[(size_t) (4 + 2 * pair)], s));
        job.format(off, i0, i1, dbuf, s);
        if ((rc = alga_check_launch(e, "k_gfa_format"))) break;
        HIP_TRY(e, hipEventRecord(evs.ev[(size_t) (5 + 2 * pair)], s));
        // ... wait for the write of the chunk two before (it read this pinned buffer) while the device formats
        if ((rc = finish_slot(slot)) || !io_ok) break;
        pending_fmt[slot] = pair;
        pair = (pair + 1) & 3;
        HIP_TRY(e, hipMemcpyAsync(e->gfa_pin[slot], dbuf, (size_t) bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipEventRecord(evs.ev[(size_t) (2 + slot)], s));
        hipEvent_t copied = evs.ev[(size_t) (2 + slot)];
        const char *src = (const char *) e->gfa_pin[slot];
        const int f = fd;
        writer[slot] = std::async(std::launch::async, [copied, src, bytes, f, at = head + b0]() {
            return hipEventSynchronize(copied) == hipSuccess && write_all(f, src, (size_t) bytes, at);
        });
        slot ^= 1;
    }
    for (int k = 0; k < 2; k++) { const int r = finish_slot(k); if (rc == ALGA_OK) rc = r; }
    if (rc != ALGA_OK) return rc;
    HIP_TRY(e, hipStreamSynchronize(s));
    if (!io_ok) return io_fail("write");
    if (close(fd) != 0) { fd = -1; return io_fail("close"); }
    fd = -1;
    if (info) info->ms_format = ms_format;
    return ALGA_OK;
}

// The GFA of a node set and its edge list: the device's verdict on the input and the per-source rows come before the sizes
int gfa_export(alga_engine *e, const GfaCfg &c, const char *path, alga_gfa_info *info, std::chrono::steady_clock::time_point t0) {
    AlgaTextJob job;
    job.items = c.n_seg + c.m;                                       // segment lines, then link lines
    job.kind = "GFA"; job.head = kGfaHeader;
    job.prepare = [e, c](unsigned long long *cnt, hipStream_t s) -> int {
        int rc;
        if ((rc = alga_ensure(e, e->gfa_rowptr, ((size_t) c.n + 2) * sizeof(uint32_t)))) return rc;
        launch_gfa_check(c, cnt, s);
        if ((rc = alga_check_launch(e, "k_gfa_check"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        if (const unsigned long long bad = e->h_counters[GFA_FLAGS]) {
            const char *why = (bad & GFA_BAD_ID) ? "edge endpoint outside [0, n)" : (bad & GFA_BAD_ORDER) ? "edges must be sorted by (src, dst, offset)"
                            : (bad & GFA_BAD_LEN) ? "negative node length" : "ALGA_GFA_TWINS: len[2k] != len[2k + 1]";
            return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
        }
        if (c.m) {                                                   // the list is valid: per-source rows
            launch_edge_rowptr(c.e, c.m, c.n, (uint32_t *) e->gfa_rowptr.p, s);
            if ((rc = alga_check_launch(e, "k_edge_rowptr"))) return rc;
        }
        return ALGA_OK;
    };
    job.sizes = [e, c](uint32_t *sizes, unsigned long long *cnt, hipStream_t s) { launch_gfa_sizes(c, (const uint32_t *) e->gfa_rowptr.p, sizes, cnt, s); };
    job.format = [c](const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) { launch_gfa_format(c, off, i0, i1, buf, s); };
    return alga_text_job_run(e, job, path, info, t0);
}

}  // namespace

int alga_text_job_run(alga_engine *e, const AlgaTextJob &job, const char *path, alga_gfa_info *info, std::chrono::steady_clock::time_point t0) {
    int fd = -1;
    const int rc = gfa_impl(e, job, path, info, fd);
    if (rc != ALGA_OK) {
        (void) hipStreamSynchronize(e->own_stream);                 // nothing may still copy into the pinned buffers
        if (fd >= 0) { close(fd); unlink(path); }                  // no partial file is left behind
        return rc;
    }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}

extern "C" int alga_write_gfa_device(alga_engine *e, const alga_nodes *nodes, const alga_edge *d_edges, uint64_t n_edges, const char *path, int32_t flags,
                                     alga_gfa_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_gfa_info{};
    if (!nodes || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes and path must not be NULL");
    if (flags & ~(ALGA_GFA_TWINS | ALGA_GFA_SEQUENCES)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown GFA flag");
    if (nodes->n < 0 || (nodes->n && !nodes->len) || (n_edges && !d_edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node set or edge list");
    if ((flags & ALGA_GFA_SEQUENCES) && nodes->n && (!nodes->words || nodes->stride_words <= 0))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "ALGA_GFA_SEQUENCES needs the rows");
    if ((flags & ALGA_GFA_TWINS) && (nodes->n & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "ALGA_GFA_TWINS: the node count must be even");
    if (n_edges >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    const bool twins = flags & ALGA_GFA_TWINS;
    GfaCfg c{nodes->words, nodes->stride_words, nodes->len, nodes->n, (const alga_edge_dev *) d_edges, n_edges, twins ? (uint64_t) nodes->n / 2 : (uint64_t) nodes->n,
             twins ? 1 : 0, (flags & ALGA_GFA_SEQUENCES) ? 1 : 0};
    return gfa_export(e, c, path, info, t0);
}

// The unitig graph as GFA: the same kernels over the ragged rows (GfaCfg::row_off); pair k is segment k, oriented unitig 2k+1 is `+`.
extern "C" int alga_write_unitig_gfa_device(alga_engine *e, const alga_unitigs *u, const char *path, int32_t flags, alga_gfa_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_gfa_info{};
    if (!u || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs and path must not be NULL");
    if (flags & ~(ALGA_GFA_SEQUENCES | ALGA_GFA_CONSENSUS)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown GFA flag (unitigs are always written as twin pairs)");
    if ((flags & ALGA_GFA_CONSENSUS) && !(flags & ALGA_GFA_SEQUENCES)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "ALGA_GFA_CONSENSUS needs ALGA_GFA_SEQUENCES");
    if (!e->ut_valid || u->d_len != (const int32_t *) e->ut_ulen.p || (uint64_t) u->n_pairs != e->ut_n_pairs || u->n_edges != e->ut_n_edges ||
        u->d_words != (const uint32_t *) e->ut_words.p || u->d_edges != (const alga_edge *) e->ut_edges.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_unitigs_device call on this engine");
    if (u->n_edges >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    if ((flags & ALGA_GFA_CONSENSUS) && !e->cs_valid) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "ALGA_GFA_CONSENSUS: no consensus of this unitig result on the engine");
    // the consensus has the layout of the spelled sequences: only the rows differ
    GfaCfg c{(flags & ALGA_GFA_CONSENSUS) ? (const uint32_t *) e->cs_words.p : u->d_words, 0, (const int32_t *) e->ut_ulen2.p, 2 * u->n_pairs,
             (const alga_edge_dev *) u->d_edges, u->n_edges, (uint64_t) u->n_pairs, 1, (flags & ALGA_GFA_SEQUENCES) ? 1 : 0};
    c.row_off = (const unsigned long long *) u->d_word_off;
    return gfa_export(e, c, path, info, t0);
}

// The consensus windows as FASTA: one record per pair that is long enough
extern "C" int alga_write_consensus_fasta_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const char *path, int32_t min_length,
                                                 alga_gfa_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_gfa_info{};
    if (!u || !cons || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs, consensus and path must not be NULL");
    if (!e->ut_valid || u->d_len != (const int32_t *) e->ut_ulen.p || (uint64_t) u->n_pairs != e->ut_n_pairs || u->d_words != (const uint32_t *) e->ut_words.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_unitigs_device call on this engine");
    if (!e->cs_valid || cons->n_pairs != u->n_pairs || cons->d_words != (const uint32_t *) e->cs_words.p || cons->d_len != (const int32_t *) e->cs_len.p ||
        cons->d_trim_left != (const int32_t *) e->cs_trim.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_unitig_consensus_device call on this engine");
    HIP_TRY(e, hipSetDevice(e->device));
    GfaFasta f{cons->d_words, (const unsigned long long *) u->d_word_off, cons->d_len, cons->d_trim_left, nullptr, (uint64_t) u->n_pairs, min_length};
    if (e->ut_is_contig) {                                           // the records are numbered as they are written: a scan of the selection
        const uint64_t P = (uint64_t) u->n_pairs;
        int rc;
        if ((rc = alga_ensure(e, e->ct_names, (size_t) (2 * P + 4) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(P)))) return rc;
        uint32_t *sel = (uint32_t *) e->ct_names.p, *rank = sel + P + 1;
        launch_ct_fasta_select(cons->d_len, P, min_length, sel, e->own_stream);
        launch_exclusive_scan(sel, P, rank, (uint64_t *) e->scan_scratch.p, e->own_stream);
        if ((rc = alga_check_launch(e, "scan(fasta records)"))) return rc;
        f.rec_rank = rank;
    }
    return alga_text_records(e, f, launch_gfa_fasta_sizes, launch_gfa_fasta_write, path, info, t0);
}
