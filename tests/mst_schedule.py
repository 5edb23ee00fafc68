"""The round schedule of alga_remove_short_parallel_paths_device, restated in Python (include/alga_amd.h has the definition).

The step itself is tests/tips_checker.py: try_to_remove_short_paths_mst, run for the nodes in ascending order, each on the graph the earlier
ones left.  A beg reads and writes only the lists of the nodes it expands, all of them within distance max_offset of it, and the step only
removes edges, so two begs whose balls B(beg) = {v : shortest distance beg -> v <= max_offset} on the current graph are disjoint commute.
A round: every pending beg (>= 2 out-edges now) claims the nodes of its ball with the minimum of the claiming ids; a beg wins when it holds
its whole ball; the winners run, in any order.  The smallest pending id always wins."""
import heapq

import tips_checker as T


def ball(g, beg, max_offset):
    """nodes at shortest-path distance <= max_offset from beg (beg itself always)"""
    dist = {beg: 0}
    heap = [(0, beg)]
    while heap:
        d, a = heapq.heappop(heap)
        if d > dist[a]:
            continue
        for b, o in g[a]:
            nd = d + o
            if nd <= max_offset and (b not in dist or nd < dist[b]):
                dist[b] = nd
                heapq.heappush(heap, (nd, b))
    return set(dist)


def remove_short_parallel_paths_rounds(g, max_offset, reverse_winners=True, ball_of=ball):
    """The step on the adjacency lists g (modified in place), by rounds -> dict(rounds, winners (per round), begs_run, branching_nodes,
    ball_max).  ball_of: any function that returns a superset of the ball gives the same lists (and at least as many rounds)."""
    was = [False] * len(g)
    pending = [v for v in range(len(g)) if len(g[v]) >= 2]
    info = dict(rounds=0, winners=[], begs_run=0, branching_nodes=len(pending), ball_max=0)
    while True:
        pending = [v for v in pending if len(g[v]) >= 2]           # a degree never rises again
        if not pending:
            break
        owner, balls = {}, {}
        for v in pending:
            balls[v] = ball_of(g, v, max_offset)
            info["ball_max"] = max(info["ball_max"], len(balls[v]))
            for x in balls[v]:
                if owner.get(x, v) >= v:
                    owner[x] = v
        win = [v for v in pending if all(owner[x] == v for x in balls[v])]
        assert win and win[0] == pending[0]
        for v in (reversed(win) if reverse_winners else win):
            T.try_to_remove_short_paths_mst(g, v, max_offset, was)
        won = set(win)
        pending = [v for v in pending if v not in won]
        info["winners"].append(len(win))
    info["rounds"] = len(info["winners"])
    info["begs_run"] = sum(info["winners"])
    return info


def random_graph(rng, n_max=2000):
    """-> (n, edges int32 [m, 3] grouped by src in ascending order, bound): chains with bubbles, sparse and dense random graphs; self-loops,
    parallel edges and zero offsets among them.  Within a list the entries are in random order (list order matters to the step)."""
    import numpy as np
    kind = int(rng.integers(0, 4))
    n = int(rng.integers(2, n_max + 1 if kind != 2 else min(n_max, 119) + 1))
    m = int(rng.integers(0, [int(1.3 * n) + 1, 3 * n, n * n // 2 + 1, 2 * n][kind]))
    e = np.stack([rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, [1, 4, 30, 200][int(rng.integers(0, 4))], m)], axis=1)
    if kind == 0 and n > 5:
        spine = np.stack([np.arange(n - 1), np.arange(1, n), rng.integers(0, 20, n - 1)], axis=1)
        skip = np.stack([np.arange(n - 2), np.arange(2, n), rng.integers(0, 40, n - 2)], axis=1)
        e = np.concatenate([e, spine[rng.random(n - 1) < 0.9], skip[rng.random(n - 2) < 0.3]])
    e = e[rng.permutation(len(e))]
    e = e[np.argsort(e[:, 0], kind="stable")]
    return n, np.ascontiguousarray(e, dtype=np.int32), int([0, 1, 5, 30, 100, 10 ** 6][int(rng.integers(0, 6))])


def ascending_chain(k):
    """A line 0 .. k - 1 with ids ascending along it: i -> i + 1 (offset 1), a bubble i -> i + 2 (offset 3) and a side branch i -> k + i (offset
    1), which keeps every node of the line branching whatever the earlier ones removed.  A ball holds the next nodes of the line, so no two
    pending begs next to each other are independent: one winner per round, the worst case of the schedule.  -> (2 k, edges)"""
    import numpy as np
    e = []
    for i in range(k):
        if i + 2 < k:
            e.append((i, i + 2, 3))
        if i + 1 < k:
            e.append((i, i + 1, 1))
        e.append((i, k + i, 1))
    return 2 * k, np.array(e, dtype=np.int32).reshape(-1, 3)
