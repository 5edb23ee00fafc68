"""Dangling-branch removal, restated literally in Python: the definition alga_remove_dangling_branches_device is tested against.

The reference: GraphSimplifier::removeDanglingBranches / removeDanglingBranchesFromNode / removeDanglingUpperBranches and the loop of
simplifyGraphOld that iterates them (src/GraphSimplifiers/GraphSimplifier.cpp:191-215, :577-820), with Graph::retainOnlySmallestOffset,
Graph::removeDirectedEdge (swap with the last entry) and Graph::reverseGraph in its --threads=1 order (src/DataStructures/Graph.cpp).
A graph is a list of adjacency lists of [neighbour, offset] entries, in the reference's in-list order.

`keep`: edges (a, b) that a pass finds but never removes.  The reference's parallel removal
(WorkloadManager::parallelBlockExecution(0, size - 1, 3 * threads, ...)) leaves out the last element of its shuffled removal list when
(size - 1) % (3 * threads) == 0, and the only element when size == 1; with `keep` empty every found edge goes, which is what the engine does.

try_to_remove_short_paths_mst restates GraphSimplifier::tryToRemoveShortPathsMST (:431-518) and remove_short_parallel_paths the
sequential order of removeShortParallelPaths over the nodes; they exist for the golden test only (that step is not on the device)."""
import numpy as np


def graph_from_edges(n, edges):
    """edge array [m, 3] in list order -> adjacency lists (entry order = order in the array)"""
    g = [[] for _ in range(n)]
    for a, b, o in np.asarray(edges, dtype=np.int64).reshape(-1, 3).tolist():
        g[a].append([b, o])
    return g


def edges_from_graph(g, sort=False):
    e = [(a, b, o) for a, lst in enumerate(g) for b, o in lst]
    if sort:
        e.sort()
    return np.array(e, dtype=np.int32).reshape(-1, 3)


def retain_only_smallest_offset(g):
    """Graph::retainOnlySmallestOffsetJob: every list sorted by (neighbour, offset), the first entry of each neighbour kept"""
    for i, lst in enumerate(g):
        lst.sort()
        new = []
        for p in lst:
            if not new or new[-1][0] != p[0]:
                new.append(p)
        g[i] = new


def remove_directed_edge(g, a, b):
    """Graph::removeDirectedEdge: every entry a -> b, each swapped with the (shrinking) last position; True if one was there"""
    lst = g[a]
    removed = False
    p = len(lst) - 1
    for i in range(len(lst) - 1, -1, -1):
        if lst[i][0] == b:
            lst[i], lst[p] = lst[p], lst[i]
            lst.pop()
            p -= 1
            removed = True
    return removed


def reverse_graph(g):
    """Graph::reverseGraph with one thread: nodes in ascending order push themselves onto their neighbours' new lists"""
    r = [[] for _ in g]
    for j, lst in enumerate(g):
        for d, off in lst:
            r[d].append([j, off])
    return r


def dangling_from_node(g, beg, max_offset, was, found):
    """GraphSimplifier::removeDanglingBranchesFromNode; the edges it wants removed are added to the set `found`"""
    ends = []
    neigh = []
    par = {beg: beg}
    for v, offset in list(g[beg]):
        par[v] = beg
        was[v] = True
        neigh.append(v)
        while len(g[v]) == 1:
            son, w = g[v][0]
            if was[son]:
                break
            was[son] = True
            neigh.append(son)
            par[son] = v
            offset += w
            v = son
            if offset > max_offset:
                break
        if len(g[v]) == 0 and offset <= max_offset:
            ends.append((offset, v))
    ends.sort()
    div = 1 if len(ends) == len(g[beg]) else 0
    for _, v in ends[: len(ends) - div]:
        while v != beg:
            found.add((par[v], v))
            v = par[v]
    for a in neigh:
        was[a] = False


def dangling_pass(g, max_offset, keep=()):
    """GraphSimplifier::removeDanglingBranches: every node with >= 2 out-edges looks at the same unmodified graph, the union of what they
    find is removed afterwards -> (number removed, sorted list of the found edges)"""
    was = [False] * len(g)
    found = set()
    for j in range(len(g)):
        if len(g[j]) >= 2:
            dangling_from_node(g, j, max_offset, was, found)
    removed = 0
    for a, b in sorted(found):
        if (a, b) in keep:
            continue
        if remove_directed_edge(g, a, b):
            removed += 1
    return removed, sorted(found)


def remove_dangling_branches(n, edges, max_offset, keep=(), trace=None):
    """The whole step on an edge list in any order -> (surviving edges sorted by (src, dst, offset) as int32 [m', 3], per-pass counts:
    down, up, down, up, ...).  `keep`: a set of (a, b) (graph direction) or a list with one such set per pass.  `trace`: a list that
    receives the sorted found edges of every pass (graph direction)."""
    g = graph_from_edges(n, edges)
    retain_only_smallest_offset(g)
    counts = []
    i = 0
    while True:
        per_pass = isinstance(keep, list)
        k_down = keep[len(counts)] if per_pass and len(counts) < len(keep) else (set() if per_pass else keep)
        down, f = dangling_pass(g, max_offset, k_down)
        if trace is not None:
            trace.append(f)
        counts.append(down)
        g = reverse_graph(g)
        k_up = keep[len(counts)] if per_pass and len(counts) < len(keep) else (set() if per_pass else keep)
        up, f = dangling_pass(g, max_offset, {(b, a) for a, b in k_up})
        if trace is not None:
            trace.append([(b, a) for a, b in f])
        counts.append(up)
        g = reverse_graph(g)
        removed = down + up
        if removed == 0 or (i >= 15 and removed <= 30):
            break
        i += 1
    return edges_from_graph(g, sort=True), counts


# ---- the step before it in simplifyGraphOld, for the golden test only ------------------------------------------------------------------

def try_to_remove_short_paths_mst(g, beg, max_offset, was):
    """GraphSimplifier::tryToRemoveShortPathsMST"""
    edges = []
    neigh = [beg]
    dst = {beg: 0}
    i = 0
    while i < len(neigh):
        a = neigh[i]
        i += 1
        if was[a] or dst[a] > max_offset:
            continue
        was[a] = True
        for b, offset in g[a]:
            if b in dst and dst[b] < dst[a] + offset:
                continue
            dst[b] = dst[a] + offset
            edges.append(((a, b), offset))
            neigh.append(b)
    for (a, b), _ in edges:
        remove_directed_edge(g, a, b)
    edges.sort(key=lambda x: (x[1], x[0]))
    for a in neigh:
        was[a] = False
    for (a, b), offset in edges:
        if was[b]:
            continue
        g[a].append([b, offset])
        was[b] = True
    for (a, b), _ in edges:
        was[b] = False


def remove_short_parallel_paths(g, max_offset):
    """GraphSimplifier::removeShortParallelPaths with one thread: the nodes in ascending order, each on the graph the earlier ones left"""
    was = [False] * len(g)
    for i in range(len(g)):
        if len(g[i]) >= 2:
            try_to_remove_short_paths_mst(g, i, max_offset, was)
