// alga_amd/csrc/mst_walk.h -- what ONE node `beg` does in the removal of short parallel paths (include/alga_amd.h:
// alga_remove_short_parallel_paths_device; the reference: GraphSimplifier::tryToRemoveShortPathsMST).  Plain C++ over the arrays of
// mst_kernels.hip, host and device: the kernels call these functions with one unit of work per beg.
//
// The graph is a set of mutable rows of fixed capacity: row v is rows[rowptr[v] .. rowptr[v] + len[v]), in list order; a row never grows
// beyond rowptr[v + 1] - rowptr[v], because a beg only pushes back what it took out.
//
// The state of one beg (MstState) is a map node -> value (open addressing, linear probing; the insertion order kept as a list of slots, which
// is also how the map is emptied again) and a list of collected edges.  The same code runs on a state in LDS (the short form of
// mst_kernels.hip) and on one in a device workspace sized for the whole graph (the overflow route); a state that is too small makes the
// function return false BEFORE anything outside the state has been written.
//
//   mst_ball   the nodes at shortest-path distance <= max_offset from beg on the rows as they are: label correcting, swept until nothing
//              changes.  Every node the literal walk can expand is among them (its label is at least the shortest distance).
//   mst_run    the literal step: the queue walk in list order with dst[] overwritten as the reference does it, Graph::removeDirectedEdge per
//              collected edge in collection order, the edges sorted by (offset, a, b), pushed back unless an edge into b was pushed already.
//              The queue is not stored: it is beg followed by the b of every collected edge, in collection order.
#pragma once
#include <stdint.h>
#include "prefsuf_kernels.h"

#if defined(__HIPCC__)
#define MST_HD __host__ __device__ __forceinline__
#else
#define MST_HD inline
#endif

namespace alga {

struct MstGraph {
    alga_edge_dev *rows;          // .src = the row's node, .dst / .offset = the entry
    const uint32_t *rowptr;       // n + 1
    uint32_t *len;                // n: live entries of every row
};

struct MstState {
    uint32_t *key, *val;          // 1 << hbits slots; key: node id, MST_FLAG = dirty (mst_ball) / expanded (mst_run); MST_EMPTY = free
    uint32_t hbits;
    uint32_t *slots;              // cap_nodes: the occupied slots in insertion order
    uint32_t cap_nodes;           // < 1 << hbits
    uint32_t *edges;              // 3 * cap_edges: (a, b, offset)
    uint32_t cap_edges;
};

constexpr uint32_t MST_EMPTY = 0xFFFFFFFFu, MST_FLAG = 0x80000000u, MST_PUSHED = 0xFFFFFFFFu, MST_NONE = 0xFFFFFFFFu;

// the slot of `node`, entered if it is not there (found = false); MST_NONE: the map is full
MST_HD uint32_t mst_slot(const MstState &st, uint32_t node, uint32_t &ns, bool &found) {
    const uint32_t mask = (1u << st.hbits) - 1;
    uint32_t h = (node * 2654435761u) >> (32 - st.hbits);
    for (;;) {
        const uint32_t k = st.key[h];
        if (k == MST_EMPTY) {
            found = false;
            if (ns == st.cap_nodes) return MST_NONE;
            st.key[h] = node; st.slots[ns++] = h;
            return h;
        }
        if ((k & ~MST_FLAG) == node) { found = true; return h; }
        h = (h + 1) & mask;
    }
}

MST_HD void mst_clear(const MstState &st, uint32_t ns) {
    for (uint32_t i = 0; i < ns; i++) st.key[st.slots[i]] = MST_EMPTY;
}

// -> true: key[slots[0 .. ns)] & ~MST_FLAG are the nodes of the ball (the caller empties the map); false: the map is too small (ns as far as it got)
MST_HD bool mst_ball(const MstGraph &g, int32_t beg, int32_t max_offset, const MstState &st, uint32_t &ns) {
    ns = 0;
    bool found;
    const uint32_t s0 = mst_slot(st, (uint32_t) beg, ns, found);
    st.val[s0] = 0;
    if (max_offset < 0) return true;
    st.key[s0] |= MST_FLAG;
    for (bool changed = true; changed;) {
        changed = false;
        for (uint32_t i = 0; i < ns; i++) {                         // nodes entered during the sweep are swept too
            const uint32_t sl = st.slots[i], k = st.key[sl];
            if (!(k & MST_FLAG)) continue;
            st.key[sl] = k & ~MST_FLAG;
            const uint32_t a = k & ~MST_FLAG, d = st.val[sl], base = g.rowptr[a], L = g.len[a];
            for (uint32_t j = 0; j < L; j++) {
                const uint32_t b = (uint32_t) g.rows[base + j].dst;
                const uint64_t nd = (uint64_t) d + (uint32_t) g.rows[base + j].offset;
                if (nd > (uint64_t) max_offset) continue;
                const uint32_t sb = mst_slot(st, b, ns, found);
                if (sb == MST_NONE) return false;
                if (found && st.val[sb] <= (uint32_t) nd) continue;
                st.val[sb] = (uint32_t) nd; st.key[sb] |= MST_FLAG;
                changed = true;
            }
        }
    }
    return true;
}

MST_HD bool mst_edge_less(const uint32_t *x, const uint32_t *y) {      // (offset, a, b)
    if (x[2] != y[2]) return x[2] < y[2];
    if (x[0] != y[0]) return x[0] < y[0];
    return x[1] < y[1];
}

MST_HD void mst_sift(uint32_t *e, uint32_t root, uint32_t n) {
    for (;;) {
        uint32_t c = 2 * root + 1;
        if (c >= n) return;
        if (c + 1 < n && mst_edge_less(e + 3 * c, e + 3 * (c + 1))) c++;
        if (!mst_edge_less(e + 3 * root, e + 3 * c)) return;
        for (int k = 0; k < 3; k++) { const uint32_t t = e[3 * root + k]; e[3 * root + k] = e[3 * c + k]; e[3 * c + k] = t; }
        root = c;
    }
}

// edges that compare equal are the same triple: any sort gives the reference's order
MST_HD void mst_sort_edges(uint32_t *e, uint32_t n) {
    if (n < 2) return;
    for (uint32_t i = n / 2; i-- > 0;) mst_sift(e, i, n);
    for (uint32_t m = n - 1; m > 0; m--) {
        for (int k = 0; k < 3; k++) { const uint32_t t = e[k]; e[k] = e[3 * m + k]; e[3 * m + k] = t; }
        mst_sift(e, 0, m);
    }
}

// -> false: the state is too small, nothing but the (emptied) state has been written.  n_map: the nodes the map held, n_col: collected edges.
MST_HD bool mst_run(const MstGraph &g, int32_t beg, int32_t max_offset, const MstState &st, uint32_t &n_map, uint32_t &n_col) {
    uint32_t ns = 0, ne = 0;
    bool found;
    st.val[mst_slot(st, (uint32_t) beg, ns, found)] = 0;
    for (uint32_t qi = 0; qi <= ne; qi++) {
        const uint32_t a = qi ? st.edges[3 * (qi - 1) + 1] : (uint32_t) beg;
        const uint32_t sa = mst_slot(st, a, ns, found);               // every queued node is in the map
        const uint32_t k = st.key[sa], da = st.val[sa];
        if ((k & MST_FLAG) || (int64_t) da > (int64_t) max_offset) continue;
        st.key[sa] = k | MST_FLAG;
        const uint32_t base = g.rowptr[a], L = g.len[a];
        for (uint32_t j = 0; j < L; j++) {
            const uint32_t b = (uint32_t) g.rows[base + j].dst, o = (uint32_t) g.rows[base + j].offset;
            const uint32_t nd = da + o;                                // da <= max_offset < 2^31, o < 2^31
            const uint32_t sb = mst_slot(st, b, ns, found);
            if (sb == MST_NONE || (ne == st.cap_edges && !(found && st.val[sb] < nd))) { mst_clear(st, ns); return false; }
            if (found && st.val[sb] < nd) continue;
            st.val[sb] = nd;
            st.edges[3 * ne] = a; st.edges[3 * ne + 1] = b; st.edges[3 * ne + 2] = o;
            ne++;
        }
    }
    // Graph::removeDirectedEdge(a, b) per collected edge: every entry a -> b, from the back, each replaced by the (shrinking) last one
    for (uint32_t e = 0; e < ne; e++) {
        const uint32_t a = st.edges[3 * e], b = st.edges[3 * e + 1], base = g.rowptr[a];
        int64_t p = (int64_t) g.len[a] - 1;
        for (int64_t q = p; q >= 0; q--)
            if ((uint32_t) g.rows[base + q].dst == b) { g.rows[base + q] = g.rows[base + p]; p--; }
        g.len[a] = (uint32_t) (p + 1);
    }
    mst_sort_edges(st.edges, ne);
    for (uint32_t e = 0; e < ne; e++) {                                 // the first edge into every b, in sorted order
        const uint32_t a = st.edges[3 * e], b = st.edges[3 * e + 1];
        const uint32_t sb = mst_slot(st, b, ns, found);
        if (st.val[sb] == MST_PUSHED) continue;
        st.val[sb] = MST_PUSHED;
        const uint32_t L = g.len[a];
        alga_edge_dev x;
        x.src = (int32_t) a; x.dst = (int32_t) b; x.offset = (int32_t) st.edges[3 * e + 2];
        g.rows[g.rowptr[a] + L] = x;
        g.len[a] = L + 1;
    }
    mst_clear(st, ns);
    n_map = ns; n_col = ne;
    return true;
}

}  // namespace alga
