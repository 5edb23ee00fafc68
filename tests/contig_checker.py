"""Contigs of an overlap graph in plain Python / numpy: the DEFINITION the device code (alga_contigs_device) has to equal array for
array.  Written from the definition in include/alga_amd.h, step by step, with walks along the successors instead of list ranking, a
dictionary instead of the group sort and the triangle cut restated in four lines (tests/test_contigs_cpu.py holds it to
oracle_cut_triangles).

Input as for tests/unitig_checker.py (twin layout: node 2k+1 = read k, 2k = its reverse complement, v ^ 1 = the twin of v), plus
`max_offset`, the bound of the triangle cut.  The result has the layout of unitig_checker.unitigs: consensus_checker takes it as it is."""
import numpy as np

import unitig_checker as U

NO_KEY = 1 << 62                                                          # key of a chain without interior: it loses every tie
ROUNDS_KEPT = 64


def cut_triangles(H, max_offset):
    """Step 2d on H = {(a, c): w}: an edge of weight w <= max_offset goes when the lightest two-edge path a -> x -> c weighs exactly w;
    every decision on the unchanged H.  -> the set of surviving (a, c)"""
    out = {}
    for (a, c), w in H.items():
        out.setdefault(a, []).append((c, w))
    gone = set()
    for (a, c), w in H.items():
        if w > max_offset:
            continue
        two = [w1 + H[(x, c)] for x, w1 in out[a] if (x, c) in H]
        if two and min(two) == w:
            gone.add((a, c))
    return set(H) - gone


def one_round(n, B, max_offset):
    """Steps 2a-2d on B (int64 [m, 3], sorted by (src, dst), twin-symmetric, one edge per (src, dst)) -> dict with P, the chains, the
    dead-edge mask and the round's counts"""
    m = len(B)
    src, dst, off = B[:, 0].tolist(), B[:, 1].tolist(), B[:, 2].tolist()
    row = np.searchsorted(B[:, 0], np.arange(n + 1)).tolist() if m else [0] * (n + 1)
    outdeg = np.diff(np.array(row))
    indeg = np.bincount(B[:, 1], minlength=n) if m else np.zeros(n, dtype=np.int64)
    succ = [dst[row[v]] if outdeg[v] == 1 else -1 for v in range(n)]
    pred = [-1] * n
    for i in range(m):
        if indeg[dst[i]] == 1:
            pred[dst[i]] = src[i]
    # 2a
    P = [bool(outdeg[v] == 1 and indeg[v] == 1 and succ[v] not in (v, v ^ 1) and pred[v] not in (v, v ^ 1)) for v in range(n)]
    seen = [False] * n
    for i in range(m):                                                    # what no walk from a node outside P reaches lies on a cycle of P nodes
        if not P[src[i]]:
            v = dst[i]
            while P[v] and not seen[v]:
                seen[v] = True
                v = succ[v]
    cycles = 0
    on_cycle = [False] * n
    opened = []
    for s0 in range(n):
        if not P[s0] or seen[s0] or on_cycle[s0]:
            continue
        cyc = [s0]
        on_cycle[s0] = True
        v = succ[s0]
        while v != s0:
            cyc.append(v)
            on_cycle[v] = True
            v = succ[v]
        mn = min(min(cyc), min(c ^ 1 for c in cyc))                    # the smallest id over the cycle and its twin cycle
        opened.append(mn)
        if mn in cyc:                                                    # (a cycle and its twin cycle count once)
            cycles += 1
    for mn in opened:
        P[mn] = P[mn ^ 1] = False
    # 2b
    chains = []
    for i in range(m):
        if P[src[i]]:
            continue
        nodes, es, w, v = [src[i], dst[i]], [i], off[i], dst[i]
        while P[v]:
            e = row[v]
            es.append(e); w += off[e]; v = dst[e]
            nodes.append(v)
        inner = nodes[1:-1]
        chains.append(dict(first=i, nodes=nodes, edges=es, w=w, key=min(x >> 1 for x in inner) if inner else NO_KEY,
                           closed=nodes[-1] in (nodes[0], nodes[0] ^ 1)))
    assert sorted(e for c in chains for e in c["edges"]) == list(range(m)), "every edge of B lies in exactly one chain"
    # 2c
    groups = {}
    for k, c in enumerate(chains):
        if not c["closed"]:
            groups.setdefault((c["nodes"][0], c["nodes"][-1]), []).append(k)
    dropped = [False] * len(chains)
    reps, H = {}, {}
    parallel = 0
    for g, ks in groups.items():
        best = min((chains[k]["w"], chains[k]["key"]) for k in ks)
        reps[g] = [k for k in ks if (chains[k]["w"], chains[k]["key"]) == best]
        H[g] = best[0]
        for k in ks:
            if (chains[k]["w"], chains[k]["key"]) != best and chains[k]["w"] <= max_offset:
                dropped[k] = True
                parallel += 1
    # 2d
    alive = cut_triangles(H, max_offset)
    for (a, c) in groups:
        if (a, c) not in alive or (c ^ 1, a ^ 1) not in alive:
            for k in reps[(a, c)]:
                dropped[k] = True
    # 2e
    index = {(src[i], dst[i]): i for i in range(m)}
    dead = np.zeros(m, dtype=bool)
    for k, c in enumerate(chains):
        if dropped[k]:
            for e in c["edges"]:
                dead[e] = True
                dead[index[(dst[e] ^ 1, src[e] ^ 1)]] = True
    touched = np.zeros(n, dtype=bool)
    if m:
        touched[B[:, 0]] = True
        touched[B[:, 1]] = True
    return dict(P=np.array(P, dtype=bool), chains=chains, dead=dead, cycles=cycles, index=index, touched=touched,
                counts=dict(chains=len(chains), parallel_drops=parallel, groups_cut=len(H) - len(alive), base_edges_dropped=int(dead.sum())))


def spell(words, path_node, path_pos, path_off, ulen):
    """Unitig step 8 on a layout -> (packed words, word_off)"""
    P = len(ulen)
    nwords = (ulen + 15) // 16
    word_off = np.zeros(P + 1, dtype=np.uint64)
    word_off[1:] = np.cumsum(nwords)
    if not len(path_node):
        return np.zeros(0, dtype=np.uint32), word_off
    pair_of_entry = np.repeat(np.arange(P), np.diff(path_off.astype(np.int64)))
    stop = np.empty(len(path_node), dtype=np.int64)
    stop[:-1] = path_pos[1:]
    stop[path_off[1:].astype(np.int64) - 1] = ulen
    cnt = stop - path_pos
    assert (cnt >= 0).all()
    ent = np.repeat(np.arange(len(path_node)), cnt)
    q = np.arange(int(cnt.sum())) - (np.cumsum(cnt) - cnt)[ent]            # base index inside the node
    codes = (words[path_node[ent], q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & np.uint32(3)
    where = word_off[pair_of_entry[ent]].astype(np.int64) * 16 + path_pos[ent] + q
    flat = np.zeros(int(word_off[-1]) * 16, dtype=np.uint64)
    flat[where] = codes
    return (flat.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32), word_off


def contigs(words, lens, edges, max_offset):
    U.check(lens, edges)
    if max_offset < 0:
        raise ValueError("max_offset must not be negative")
    words = np.ascontiguousarray(words, dtype=np.uint32)
    lens64 = np.asarray(lens, dtype=np.int64)
    n = len(lens64)
    star, _ = U.symmetrise(lens64, edges)                                 # step 1
    B = star
    per_round = []
    while True:                                                           # step 2
        r = one_round(n, B, max_offset)
        per_round.append(r["counts"])
        if not r["dead"].any():
            break
        B = B[~r["dead"]]
    # step 3
    chains = r["chains"]
    by_first = {c["first"]: c for c in chains}
    ll = lens64.tolist()
    plus = []
    for c in chains:
        nd = c["nodes"]
        mine, twin = (nd[0], nd[1]), (nd[-1] ^ 1, nd[-2] ^ 1)
        tw = by_first[r["index"][twin]]
        assert [v ^ 1 for v in reversed(nd)] == tw["nodes"], "the twin of a chain is a chain"
        if mine <= twin:
            plus.append(c)
    plus.sort(key=lambda c: (c["nodes"][0], c["nodes"][1]))
    path_node, path_pos, path_off, ulen = [], [], [0], []
    first_of, last_of, last_pos = [], [], []                              # per oriented contig id
    for c in plus:
        nd = c["nodes"]
        pos = [0]
        for e in c["edges"]:
            pos.append(pos[-1] + int(B[e, 2]))
        assert pos[-1] == c["w"]
        L = pos[-1] + ll[nd[-1]]
        if L > (1 << 31) - 1:
            raise OverflowError("a contig is longer than 2^31 - 1 bases")
        path_node += nd; path_pos += pos
        path_off.append(len(path_node)); ulen.append(L)
        first_of += [nd[-1] ^ 1, nd[0]]; last_of += [nd[0] ^ 1, nd[-1]]; last_pos += [L - ll[nd[0]], pos[-1]]
    Pn = len(plus)
    path_node = np.array(path_node, dtype=np.int64)
    path_pos = np.array(path_pos, dtype=np.int64)
    path_off = np.array(path_off, dtype=np.uint64)
    ulen = np.array(ulen, dtype=np.int64)
    packed, word_off = spell(words, path_node, path_pos, path_off, ulen)
    # step 4
    starts = {}
    for y, v in enumerate(first_of):
        starts.setdefault(v, []).append(y)
    ce = sorted((x, y, last_pos[x]) for x in range(2 * Pn) for y in starts.get(last_of[x], []))
    counts = np.diff(path_off.astype(np.int64)) if Pn else np.zeros(0, dtype=np.int64)
    info = dict(edges_in=len(np.asarray(edges).reshape(-1, 3)), edges_sym=len(star), rounds=len(per_round), final_edges=len(B),
                path_nodes=int(r["P"].sum()), junction_nodes=int((r["touched"] & ~r["P"]).sum()), cycles_cut=r["cycles"],
                closed_chains=sum(c["closed"] for c in chains), reads_dropped=int(_touched(n, star).sum() - r["touched"].sum()),
                longest_nodes=int(counts.max()) if Pn else 0, longest_bases=int(ulen.max()) if Pn else 0, total_bases=int(ulen.sum()))
    for k in ("chains", "parallel_drops", "groups_cut", "base_edges_dropped"):
        info[k] = [c[k] for c in per_round[:ROUNDS_KEPT]]
    return dict(n_pairs=Pn, words=packed, word_off=word_off, len=ulen.astype(np.int32), path_node=path_node.astype(np.int32),
                path_pos=path_pos.astype(np.int32), path_off=path_off, edges=np.array(ce, dtype=np.int32).reshape(-1, 3), final=B, info=info)


def _touched(n, E):
    t = np.zeros(n, dtype=bool)
    if len(E):
        t[E[:, 0]] = True
        t[E[:, 1]] = True
    return t
