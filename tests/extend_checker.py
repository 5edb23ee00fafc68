"""The extension of contigs through junctions that paired reads support, in plain Python / numpy: the DEFINITION the device code
(alga_extend_contigs_device) has to equal array for array.  Written from the definition in include/alga_amd.h, step by step, with walks
and Python sets instead of the list ranking and the per-wave tables.

Input: the node set (twin layout: node 2k+1 = read k, 2k = its reverse complement, v ^ 1 = the twin of v), pair_off[n] (0: unpaired,
1: the mate is v + 2, 2: the mate is v - 2), a contig result `u` (tests/contig_checker.py, or the device's via to_host()) and the three
thresholds.  The result has the layout of contig_checker.contigs plus seam_off / seam_entry; consensus_checker takes it as it is, and
final_verdicts below is the new-read filter of tests/final_checker.py stated for a result whose interior seam reads are shared too."""
import numpy as np

import contig_checker as CC
import final_checker as F


def check_pairs(n, pair_off):
    """step 0 on pair_off"""
    po = np.zeros(n, dtype=np.int64) if pair_off is None else np.asarray(pair_off, dtype=np.int64)
    if len(po) != n:
        raise ValueError("pair_off has another length than the node set")
    if n & 1:
        raise ValueError("the node count must be even (twin layout)")
    if ((po < 0) | (po > 2)).any():
        raise ValueError("pair_off above 2")
    if (po[0::2] != po[1::2]).any():
        raise ValueError("pair_off[v] != pair_off[v ^ 1]")
    for v in np.nonzero(po == 1)[0].tolist():
        if v + 2 >= n or po[v + 2] != 2:
            raise ValueError("the mate of a first read is not a second read")
    for v in np.nonzero(po == 2)[0].tolist():
        if v - 2 < 0 or po[v - 2] != 1:
            raise ValueError("the mate of a second read is not a first read")
    return po


def mate(po, v):
    return v + 2 if po[v] == 1 else v - 2 if po[v] == 2 else v


def oriented(u, lens):
    """step 1 -> per oriented contig id (2k+1 = `+` of pair k, 2k = `-`) the (entries, positions), and the weights"""
    ll = np.asarray(lens, dtype=np.int64).tolist()
    po = np.asarray(u["path_off"]).astype(np.int64)
    node = np.asarray(u["path_node"]).astype(np.int64).tolist()
    pos = np.asarray(u["path_pos"]).astype(np.int64).tolist()
    L = np.asarray(u["len"]).astype(np.int64).tolist()
    ent, w = [], []
    for k in range(int(u["n_pairs"])):
        nd, p = node[po[k]: po[k + 1]], pos[po[k]: po[k + 1]]
        minus = ([v ^ 1 for v in reversed(nd)], [L[k] - q - ll[v] for v, q in zip(reversed(nd), reversed(p))])
        assert minus[1][0] == 0
        ent += [minus, (nd, p)]
        w += [minus[1][-1], p[-1]]
    return ent, w


def head_reads(entries, positions, max_insert):
    """step 2: H"""
    return {entries[i] >> 1 for i in range(1, len(entries)) if positions[i - 1] <= max_insert}


def tail_entries(entries, positions, max_insert):
    """step 2: T"""
    w = positions[-1]
    return [i for i in range(1, len(entries)) if w - positions[i] <= max_insert]


def extend(words, lens, pair_off, u, min_chain_weight, min_connections=5, max_insert=1000):
    lens64 = np.asarray(lens, dtype=np.int64)
    n = len(lens64)
    po = check_pairs(n, pair_off).tolist()
    if min_chain_weight < 0 or max_insert < 0 or min_connections < 1:
        raise ValueError("min_chain_weight and max_insert must not be negative, min_connections must be at least 1")
    words = np.ascontiguousarray(words, dtype=np.uint32)
    ll = lens64.tolist()
    P = int(u["n_pairs"])
    ent, w = oriented(u, lens64)                                          # step 1
    n2 = 2 * P
    starts = {}
    for c in range(n2):
        starts.setdefault(ent[c][0][0], []).append(c)
    # steps 2-4
    candidates = direct_n = 0
    head_max = 0
    dlink = [-1] * n2
    for x in range(n2):
        ys = starts.get(ent[x][0][-1], [])
        if len(ys) != 1:
            continue
        y = ys[0]
        candidates += 1
        if w[x] < min_chain_weight or w[y] < min_chain_weight:
            continue
        H = head_reads(ent[y][0], ent[y][1], max_insert)
        head_max = max(head_max, sum(1 for i in range(1, len(ent[y][0])) if ent[y][1][i - 1] <= max_insert))
        e = ent[x][0]
        cnt = sum(1 for i in tail_entries(e, ent[x][1], max_insert) if po[e[i]] != 0 and (mate(po, e[i]) >> 1) in H)
        if cnt >= min_connections:
            dlink[x] = y
            direct_n += 1
    out = [set() for _ in range(n2)]
    for x in range(n2):
        if dlink[x] >= 0:
            out[x].add(dlink[x])
            out[dlink[x] ^ 1].add(x ^ 1)
    inn = [set() for _ in range(n2)]
    for x in range(n2):
        for y in out[x]:
            inn[y].add(x)
    # step 5
    nxt, prv = [-1] * n2, [-1] * n2
    for x in range(n2):
        if len(out[x]) == 1:
            y = next(iter(out[x]))
            if len(inn[y]) == 1 and y != x and y != (x ^ 1):               # (y == x ^ 1 cannot happen: it needs last(x) == last(x) ^ 1)
                nxt[x] = y
                prv[y] = x
    seen = [False] * n2
    for h in range(n2):
        if prv[h] < 0:
            v = h
            while v >= 0:
                seen[v] = True
                v = nxt[v]
    cycles = 0
    on_cycle = [False] * n2
    cuts = []
    for s in range(n2):
        if seen[s] or on_cycle[s]:
            continue
        cyc = [s]
        on_cycle[s] = True
        v = nxt[s]
        while v != s:
            cyc.append(v)
            on_cycle[v] = True
            v = nxt[v]
        m = min(min(cyc), min(c ^ 1 for c in cyc))
        if m in cyc:
            cycles += 1
            cuts.append(prv[m])
    for p in cuts:
        m = nxt[p]
        nxt[p] = -1; prv[m] = -1
        nxt[m ^ 1] = -1; prv[p ^ 1] = -1
    paths = {}
    for h in range(n2):
        if prv[h] < 0:
            path, v = [], h
            while v >= 0:
                path.append(v)
                v = nxt[v]
            paths[h] = path
    assert sum(len(p) for p in paths.values()) == n2, "every oriented contig lies in exactly one path"
    plus = []
    for h, path in paths.items():
        th = path[-1] ^ 1
        assert th != h, "an extended contig is its own twin"
        assert paths[th] == [c ^ 1 for c in reversed(path)], "the twin of a path is a path"
        if (h ^ 1) < (th ^ 1):                                            # `+` of a pair comes before its `-`
            plus.append(h)
    plus.sort(key=lambda h: h ^ 1)
    # step 6
    path_node, path_pos, path_off, ulen = [], [], [0], []
    seam_off, seam_entry = [0], []
    first_of, last_of, last_pos = [], [], []
    for h in plus:
        nd, ps, seams, base = [], [], [], 0
        for j, c in enumerate(paths[h]):
            e, p = ent[c]
            skip = 1 if j else 0                                          # a seam node occurs once
            seams.append(len(nd) - skip)
            nd += e[skip:]
            ps += [base + q for q in p[skip:]]
            base += w[c]
        seams.append(len(nd) - 1)
        L = ps[-1] + ll[nd[-1]]
        if L > (1 << 31) - 1:
            raise OverflowError("an extended contig is longer than 2^31 - 1 bases")
        path_node += nd; path_pos += ps
        path_off.append(len(path_node)); ulen.append(L)
        seam_entry += seams; seam_off.append(len(seam_entry))
        first_of += [nd[-1] ^ 1, nd[0]]; last_of += [nd[0] ^ 1, nd[-1]]; last_pos += [L - ll[nd[0]], ps[-1]]
    Pn = len(plus)
    path_node = np.array(path_node, dtype=np.int64)
    path_pos = np.array(path_pos, dtype=np.int64)
    path_off = np.array(path_off, dtype=np.uint64)
    ulen = np.array(ulen, dtype=np.int64)
    packed, word_off = CC.spell(words, path_node, path_pos, path_off, ulen)
    # step 7
    st = {}
    for y, v in enumerate(first_of):
        st.setdefault(v, []).append(y)
    ce = sorted((x, y, last_pos[x]) for x in range(2 * Pn) for y in st.get(last_of[x], []))
    counts = np.diff(path_off.astype(np.int64)) if Pn else np.zeros(0, dtype=np.int64)
    info = dict(candidates=candidates, direct_links=direct_n, links=sum(len(s) for s in out), joinable=sum(1 for v in nxt if v >= 0),
                ambiguous=sum(1 for s in inn if len(s) > 1), cycles_cut=cycles, pairs_in=P, pairs_out=Pn, head_max=head_max,
                longest_nodes=int(counts.max()) if Pn else 0, longest_bases=int(ulen.max()) if Pn else 0, total_bases=int(ulen.sum()))
    return dict(n_pairs=Pn, words=packed, word_off=word_off, len=ulen.astype(np.int32), path_node=path_node.astype(np.int32),
                path_pos=path_pos.astype(np.int32), path_off=path_off, edges=np.array(ce, dtype=np.int32).reshape(-1, 3),
                seam_off=np.array(seam_off, dtype=np.uint64), seam_entry=np.array(seam_entry, dtype=np.int32), info=info)


def final_verdicts(u, cons_len, min_length, percent):
    """The new-read filter on any result: tests/final_checker.verdicts_sequential marks every path entry, which is the definition in
    include/alga_amd.h; an extended result needs nothing else."""
    return F.verdicts_sequential(u, cons_len, min_length, percent)
