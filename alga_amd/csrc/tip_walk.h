// alga_amd/csrc/tip_walk.h -- what ONE branching node does in a pass of the dangling-branch removal (include/alga_amd.h:
// alga_remove_dangling_branches_device; the reference: GraphSimplifier::removeDanglingBranchesFromNode).  Plain C++ over the arrays of
// tip_kernels.hip, host and device: the kernels call these functions with one thread per branching node.
//
// The graph of a pass is a CSR (edges E sorted by (row, neighbour), rowptr) with an `alive` byte per edge, indexed by the edge's id in the
// forward list (fid[slot]; NULL: the slot is the id -- the forward direction), and one 16-byte record per node and direction:
//   rec[v]  = (live out-degree, neighbour / offset / id of the first live out-edge)      -- in the direction of the pass
//   rrec[v] = the same against the direction of the pass: live in-degree, first live in-edge
// The reference marks every node a branching node `beg` reaches (was[]), keeps par[] of each, and stops a chain at a marked node.  Two forms:
//
//   tip_walk_full      the literal one: marks, par and a list of the marked nodes in per-node arrays of a workspace (one slot per node).
//   tip_walk_junction  keeps only the marked nodes of live in-degree >= 2 and the ends, in a short list.  A node x of in-degree 1 has one way
//                      in, from p = rrec[x].nbr: it is marked exactly when a chain went on from p to it -- a bit kept with p if p is in
//                      the list; a p of in-degree 1 that the current chain has just marked for the first time has sent nothing on yet.  par[x] = p
//                      needs no storage either.  beg's own neighbours are marked without being looked at first and get par = beg even if a chain
//                      had passed through them (the reference overwrites par); such a neighbour has in-degree >= 2, so it is in the list.
//                      The list is full: false is returned, nothing has been written, and the node goes the other way.
// The ends (offset, node) of the chains that stop at a node without out-edge within max_offset; a node can be an end twice (at the end of
// a chain, later as beg's own neighbour): kept once with the larger offset and a bit.  If every out-edge of beg gave an end, the largest
// (offset, node) is dropped -- which drops nothing when that node is there twice.  From every other end up par[] to beg: kill[edge id] = 1.
#pragma once
#include <stdint.h>
#include "prefsuf_kernels.h"

#if defined(__HIPCC__)
#define TIP_HD __host__ __device__ __forceinline__
#else
#define TIP_HD inline
#endif

namespace alga {

struct __attribute__((aligned(16))) TipRec { int32_t deg, nbr, off; uint32_t fid; };

struct TipGraph {
    const alga_edge_dev *E;       // row = .src, neighbour = .dst
    const uint32_t *rowptr;
    const uint32_t *fid;          // NULL: forward direction
    const uint8_t *alive;
    const TipRec *rec, *rrec;
};

constexpr int TIP_LIST = 8;       // marked nodes of in-degree >= 2 the short list holds
constexpr int TIP_ENDS = 4;       // ends
constexpr uint32_t TIP_BIT = 0x80000000u;

// lst: (TIP_LIST * 3 + TIP_ENDS * 2) words at `stride` words apart (the kernel: one column of a block's LDS array per thread)
TIP_HD bool tip_walk_junction(const TipGraph &g, int32_t beg, int32_t max_offset, uint32_t *lst, int stride, uint8_t *kill) {
    uint32_t *node = lst, *par = lst + TIP_LIST * stride, *eid = lst + 2 * TIP_LIST * stride;       // eid: TIP_BIT = a chain went on from this node
    uint32_t *enode = lst + 3 * TIP_LIST * stride, *eoff = enode + TIP_ENDS * stride;               // eoff: TIP_BIT = an end twice
    int c = 0, ne = 0;
    const int32_t d = g.rec[beg].deg;
    int32_t total = 0;
    auto find = [&](int32_t x) { for (int k = 0; k < c; k++) if (node[k * stride] == (uint32_t) x) return k; return -1; };
    for (uint32_t slot = g.rowptr[beg], end = g.rowptr[beg + 1]; slot < end; slot++) {
        const uint32_t f = g.fid ? g.fid[slot] : slot;
        if (!g.alive[f]) continue;
        int32_t v = g.E[slot].dst;
        int64_t off = g.E[slot].offset;
        int cur = -1;                                               // place of v in the list, -1: in-degree 1
        bool went_on = false;                                       // a chain went on from v before
        if (g.rrec[v].deg >= 2) {
            cur = find(v);
            if (cur >= 0) { went_on = (eid[cur * stride] & TIP_BIT) != 0; par[cur * stride] = (uint32_t) beg; eid[cur * stride] = f | (eid[cur * stride] & TIP_BIT); }
            else {
                if (c == TIP_LIST) return false;
                cur = c++; node[cur * stride] = (uint32_t) v; par[cur * stride] = (uint32_t) beg; eid[cur * stride] = f;
            }
        }
        TipRec rv = g.rec[v];
        while (rv.deg == 1) {
            const int32_t son = rv.nbr;
            const bool junction = g.rrec[son].deg >= 2;
            if (junction ? find(son) >= 0 : went_on) break;
            int at = -1;
            if (junction) {
                if (c == TIP_LIST) return false;
                at = c++; node[at * stride] = (uint32_t) son; par[at * stride] = (uint32_t) v; eid[at * stride] = rv.fid;
            }
            if (cur >= 0) eid[cur * stride] |= TIP_BIT;
            off += rv.off; v = son; cur = at; went_on = false;
            rv = g.rec[v];
            if (off > max_offset) break;
        }
        if (rv.deg == 0 && off <= max_offset) {
            total++;
            int k = 0;
            while (k < ne && enode[k * stride] != (uint32_t) v) k++;
            if (k < ne) { const uint32_t o = eoff[k * stride] & ~TIP_BIT; eoff[k * stride] = (o > (uint32_t) off ? o : (uint32_t) off) | TIP_BIT; }
            else {
                if (ne == TIP_ENDS) return false;
                enode[ne * stride] = (uint32_t) v; eoff[ne * stride] = (uint32_t) off; ne++;
            }
        }
    }
    int drop = -1;
    if (total == d) {                                               // every out-edge gave an end: not the last of the sorted ends
        for (int k = 0; k < ne; k++) {
            if (drop < 0) { drop = k; continue; }
            const uint32_t a = eoff[k * stride] & ~TIP_BIT, b = eoff[drop * stride] & ~TIP_BIT;
            if (a > b || (a == b && (int32_t) enode[k * stride] > (int32_t) enode[drop * stride])) drop = k;
        }
        if (drop >= 0 && (eoff[drop * stride] & TIP_BIT)) drop = -1;
    }
    for (int k = 0; k < ne; k++) {
        if (k == drop) continue;
        int32_t x = (int32_t) enode[k * stride];
        while (x != beg) {
            const TipRec in = g.rrec[x];
            if (in.deg >= 2) { const int at = find(x); kill[eid[at * stride] & ~TIP_BIT] = 1; x = (int32_t) par[at * stride]; }
            else { kill[in.fid] = 1; x = in.nbr; }
        }
    }
    return true;
}

// ws: five arrays of n words; parn (the first) is -1 everywhere on entry and on return
TIP_HD void tip_walk_full(const TipGraph &g, int32_t beg, int32_t max_offset, int32_t *ws, size_t n, uint8_t *kill) {
    int32_t *parn = ws, *pare = ws + n, *link = ws + 2 * n, *eoff = ws + 3 * n, *ecnt = ws + 4 * n;
    int32_t head = -1, total = 0;
    const int32_t d = g.rec[beg].deg;
    auto mark = [&](int32_t x, int32_t p, uint32_t f) {
        if (parn[x] == -1) { link[x] = head; head = x; ecnt[x] = 0; }
        parn[x] = p; pare[x] = (int32_t) f;
    };
    for (uint32_t slot = g.rowptr[beg], end = g.rowptr[beg + 1]; slot < end; slot++) {
        const uint32_t f = g.fid ? g.fid[slot] : slot;
        if (!g.alive[f]) continue;
        int32_t v = g.E[slot].dst;
        int64_t off = g.E[slot].offset;
        mark(v, beg, f);
        TipRec rv = g.rec[v];
        while (rv.deg == 1) {
            const int32_t son = rv.nbr;
            if (parn[son] != -1) break;
            mark(son, v, rv.fid);
            off += rv.off; v = son;
            rv = g.rec[v];
            if (off > max_offset) break;
        }
        if (rv.deg == 0 && off <= max_offset) {
            total++;
            if (ecnt[v] == 0 || eoff[v] < (int32_t) off) eoff[v] = (int32_t) off;
            ecnt[v]++;
        }
    }
    int32_t drop = -1;
    if (total == d) {
        for (int32_t x = head; x != -1; x = link[x])
            if (ecnt[x] > 0 && (drop < 0 || eoff[x] > eoff[drop] || (eoff[x] == eoff[drop] && x > drop))) drop = x;
        if (drop >= 0 && ecnt[drop] > 1) drop = -1;
    }
    for (int32_t e = head; e != -1; e = link[e]) {
        if (ecnt[e] == 0 || e == drop) continue;
        for (int32_t x = e; x != beg; x = parn[x]) kill[(uint32_t) pare[x]] = 1;
    }
    for (int32_t x = head; x != -1;) { const int32_t nx = link[x]; parn[x] = -1; x = nx; }
}

}  // namespace alga
