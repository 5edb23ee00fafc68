// alga_amd/csrc/stage_common.h -- the host glue the stages share (included at the end of engine_internal.h): the provenance of the
// handles a stage is given, the twin-node check, the timing events, the entry and the end of an extern "C" stage function, the index of
// the result set a double-buffered stage writes.  DESIGN.md section 13 names them; a new stage uses these and copies none of them.
#pragma once

#include <cstring>
#include <chrono>

// ---- handle provenance.  engine_place.hip, engine_polish.hip and engine_gapped.hip keep the struct they hand out (pl_out, po_out, gp_out); a
// handle is the engine's current result iff it is that struct field for field -- every size and every pointer, also those no consumer reads --
// and the result is still valid.  The structs hold 8-byte members only (no padding), so the comparison is one of bytes.
static_assert(sizeof(alga_placements) == 4 * 8 + 12 * sizeof(void *), "alga_placements has padding: compare it field by field");
static_assert(sizeof(alga_polished) == 3 * 8 + 7 * sizeof(void *), "alga_polished has padding: compare it field by field");
static_assert(sizeof(alga_gapped) == 4 * 8 + 11 * sizeof(void *), "alga_gapped has padding: compare it field by field");
template <class H> inline bool alga_same_handle(const H *a, const H &b) { return std::memcmp(a, &b, sizeof(H)) == 0; }

// `pl` is the placement the engine holds.  What the consumers rely on beyond identity is guaranteed where pl_out is written (place_impl in
// engine_place.hip): n_columns <= 0xFFFFFFFE (more is refused with ALGA_ERR_CAPACITY before the result is touched), n_hist = max_insert + 1 >= 2
// (check_params there), n_reads and n_targets >= 0.
inline bool alga_placement_is_current(const alga_engine *e, const alga_placements *pl) { return e->pl_valid && alga_same_handle(pl, e->pl_out); }
// `gp` is the gapped result the engine holds, and it was made from the placement at hand
inline bool alga_gapped_is_current(const alga_engine *e, const alga_gapped *gp) {
    return e->gp_valid && e->gp_pl_serial == e->pl_serial && alga_same_handle(gp, e->gp_out);
}
// `pol` is the polish the engine holds, and it was made from `pl` (the caller has checked that `pl` is current)
inline bool alga_polished_is_current(const alga_engine *e, const alga_placements *pl, const alga_polished *pol) {
    return e->po_valid && e->po_pl_serial == e->pl_serial && alga_same_handle(pol, e->po_out) && pol->n_targets == pl->n_targets && pol->n_columns == pl->n_columns;
}

// a node set in twin layout as the stages take it; need_words: the stage reads the bases (break and scaffold read the lengths alone)
inline int alga_check_twin_nodes(alga_engine *e, const alga_nodes *nodes, bool need_words) {
    if (nodes->n < 0 || (nodes->n & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "n must be even and >= 0");
    if (nodes->n && ((need_words && !nodes->words) || !nodes->len || nodes->stride_words <= 0)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node arrays");
    return ALGA_OK;
}

// ---- timing
template <int N> struct AlgaEvents {
    hipEvent_t ev[N] = {};
    ~AlgaEvents() { for (hipEvent_t x : ev) if (x) (void) hipEventDestroy(x); }
    int create(alga_engine *e) {
        for (hipEvent_t &x : ev) HIP_TRY(e, hipEventCreate(&x));
        return ALGA_OK;
    }
    int ms(alga_engine *e, int a, int b, double *out) const {
        float t = 0.0f;
        HIP_TRY(e, hipEventElapsedTime(&t, ev[a], ev[b]));
        *out = t;
        return ALGA_OK;
    }
};
inline double alga_ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// ---- the entry of an extern "C" stage function: false for a NULL engine, else the error text cleared and *info zeroed
template <class Info> inline bool alga_enter(alga_engine *e, Info *info) {
    if (!e) return false;
    e->err.clear();
    if (info) *info = Info{};
    return true;
}

// ... and what follows its host refusals: begin() selects the device and the stream (the caller's, else the engine's own); the end of the scope
// waits for that stream, whatever the stage returned
struct AlgaStageCall {
    hipStream_t s = nullptr;
    int begin(alga_engine *e, void *hip_stream) {
        HIP_TRY(e, hipSetDevice(e->device));
        s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
        return ALGA_OK;
    }
    ~AlgaStageCall() { if (s) (void) hipStreamSynchronize(s); }
};

// a double-buffered result (grow, merge, indel polish): the set a call writes -- the one that does not hold the current result -- and swaps in at its end
inline int alga_other_set(bool valid, int cur) { return valid ? 1 - cur : cur; }
