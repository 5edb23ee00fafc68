"""The unitig graph of an overlap graph in plain Python / numpy: the DEFINITION the device code (alga_unitigs_device) has to equal
byte for byte.  Written from the definition in include/alga_amd.h, step by step, with walks along next[] instead of list ranking.

Node set in ALGA's twin layout: node 2k+1 = read k, 2k = its reverse complement, v ^ 1 = the twin of v; `words` [n, stride] uint32
holds the 2-bit rows (base i in bits 2i, 2i+1 of the little-endian bit string), `lens` [n] the lengths (0 = removed), `edges` [m, 3]
int32 (src, dst, offset) in any order."""
import numpy as np


def check(lens, edges):
    """Step 1: raises ValueError where the device refuses."""
    lens = np.asarray(lens, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 3)
    n = len(lens)
    if n % 2:
        raise ValueError("the node count must be even")
    if (lens < 0).any() or (lens >= 1 << 30).any():
        raise ValueError("bad node length")
    if (lens[0::2] != lens[1::2]).any():
        raise ValueError("len[2k] != len[2k+1]")
    if len(e) == 0:
        return
    a, b, o = e[:, 0], e[:, 1], e[:, 2]
    if (a < 0).any() or (a >= n).any() or (b < 0).any() or (b >= n).any():
        raise ValueError("edge endpoint out of range")
    if (lens[a] <= 0).any() or (lens[b] <= 0).any():
        raise ValueError("edge endpoint is a removed node")
    if (o < 0).any() or (o >= lens[a]).any() or (o + lens[b] < lens[a]).any():
        raise ValueError("edge is not a dovetail")


def symmetrise(lens, edges):
    """Step 2: E* as an int64 array [m*, 3] sorted by (src, dst), and the number of (src, dst) pairs the input did not hold."""
    lens = np.asarray(lens, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 3)
    if len(e) == 0:
        return np.zeros((0, 3), dtype=np.int64), 0
    tw = np.stack([e[:, 1] ^ 1, e[:, 0] ^ 1, lens[e[:, 1]] - lens[e[:, 0]] + e[:, 2]], axis=1)
    both = np.concatenate([e, tw])
    both = both[np.lexsort((both[:, 2], both[:, 1], both[:, 0]))]
    first = np.ones(len(both), dtype=bool)
    first[1:] = (both[1:, 0] != both[:-1, 0]) | (both[1:, 1] != both[:-1, 1])
    star = both[first]
    own = np.unique(e[:, 0] * (1 << 32) + e[:, 1])
    return star, len(star) - len(own)


def unpack_rows(words, lens):
    """2-bit rows -> list of uint8 code arrays (tests only: small sets)."""
    words = np.asarray(words, dtype=np.uint32)
    out = []
    for r, L in zip(words, lens):
        q = np.arange(int(L))
        out.append(((r[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3).astype(np.uint8))
    return out


def unitigs(words, lens, edges, skip_isolated=False):
    check(lens, edges)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    lens64 = np.asarray(lens, dtype=np.int64)
    n = len(lens64)
    star, twins_added = symmetrise(lens64, edges)
    src, dst, off = star[:, 0], star[:, 1], star[:, 2]
    outdeg = np.bincount(src, minlength=n) if len(star) else np.zeros(n, dtype=np.int64)
    indeg = np.bincount(dst, minlength=n) if len(star) else np.zeros(n, dtype=np.int64)
    # step 3
    comp = (outdeg[src] == 1) & (indeg[dst] == 1) & (dst != src) & (dst != (src ^ 1)) if len(star) else np.zeros(0, dtype=bool)
    nxt = np.full(n, -1, dtype=np.int64)
    noff = np.zeros(n, dtype=np.int64)
    prv = np.full(n, -1, dtype=np.int64)
    nxt[src[comp]] = dst[comp]
    noff[src[comp]] = off[comp]
    prv[dst[comp]] = src[comp]
    live = lens64 > 0
    # step 4: whatever no walk from a head reaches lies on a cycle of compactable edges
    nx = nxt.tolist()
    seen = np.zeros(n, dtype=bool)
    for h in np.nonzero(live & (prv < 0))[0].tolist():
        v = h
        while v >= 0:
            seen[v] = True
            v = nx[v]
    cuts = []
    cycles = 0
    on_cycle = np.zeros(n, dtype=bool)
    for s in np.nonzero(live & ~seen)[0].tolist():
        if on_cycle[s]:
            continue
        cyc = [s]
        on_cycle[s] = True
        v = nx[s]
        while v != s:
            cyc.append(v)
            on_cycle[v] = True
            v = nx[v]
        m = min(min(cyc), min(c ^ 1 for c in cyc))
        if m in set(cyc):
            cycles += 1
            cuts.append(int(prv[m]))
    for p in cuts:
        m = int(nxt[p])
        nxt[p] = -1; prv[m] = -1
        nxt[m ^ 1] = -1; prv[p ^ 1] = -1
    # step 5: walks from the heads
    nx = nxt.tolist()
    no = noff.tolist()
    ll = lens64.tolist()
    heads = np.nonzero(live & (prv < 0))[0].tolist()
    head_of = np.full(n, -1, dtype=np.int64)
    pos_of = np.zeros(n, dtype=np.int64)
    paths = {}
    for h in heads:
        path, pos, v, p = [], [], h, 0
        while v >= 0:
            path.append(v); pos.append(p)
            p += no[v]
            v = nx[v]
        paths[h] = (path, pos)
        head_of[path] = h
        pos_of[path] = pos
    if (head_of[live] < 0).any():
        raise AssertionError("a live node lies in no unitig")
    # step 6 (and 10)
    has_edge = (outdeg > 0) | (indeg > 0)
    plus = []
    isolated_skipped = 0
    for h in heads:
        path = paths[h][0]
        th = path[-1] ^ 1
        if th == h:
            raise AssertionError("a unitig is its own twin")
        if h > th:
            continue
        if skip_isolated and len(path) == 1 and not has_edge[h] and not has_edge[h ^ 1]:
            isolated_skipped += 1
            continue
        plus.append(h)
    plus.sort()
    uid = np.full(n, -1, dtype=np.int64)
    path_node, path_pos, path_off, ulen = [], [], [0], []
    for k, h in enumerate(plus):
        path, pos = paths[h]
        L = pos[-1] + ll[path[-1]]
        if L > (1 << 31) - 1:
            raise OverflowError("a unitig is longer than 2^31 - 1 bases")
        uid[path] = 2 * k + 1
        uid[[v ^ 1 for v in path]] = 2 * k
        path_node += path; path_pos += pos
        path_off.append(len(path_node)); ulen.append(L)
    P = len(plus)
    path_node = np.array(path_node, dtype=np.int64)
    path_pos = np.array(path_pos, dtype=np.int64)
    path_off = np.array(path_off, dtype=np.uint64)
    ulen = np.array(ulen, dtype=np.int64)
    # step 8: entry i spells the bases pos[i] .. pos[i+1] of its unitig (the last one of a path: up to L)
    nwords = (ulen + 15) // 16
    word_off = np.zeros(P + 1, dtype=np.uint64)
    word_off[1:] = np.cumsum(nwords)
    if len(path_node):
        pair_of_entry = np.repeat(np.arange(P), np.diff(path_off.astype(np.int64)))
        stop = np.empty(len(path_node), dtype=np.int64)
        stop[:-1] = path_pos[1:]
        last = path_off[1:].astype(np.int64) - 1
        stop[last] = ulen
        cnt = stop - path_pos
        assert (cnt >= 0).all()
        ent = np.repeat(np.arange(len(path_node)), cnt)
        start = np.cumsum(cnt) - cnt
        q = np.arange(int(cnt.sum())) - start[ent]                     # base index inside the node
        node = path_node[ent]
        codes = (words[node, q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & np.uint32(3)
        where = word_off[pair_of_entry[ent]].astype(np.int64) * 16 + path_pos[ent] + q
        flat = np.zeros(int(word_off[-1]) * 16, dtype=np.uint64)
        flat[where] = codes
        packed = (flat.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    else:
        packed = np.zeros(0, dtype=np.uint32)
    # step 9
    if len(star):
        keep = nxt[src] != dst
        ue = np.stack([uid[src[keep]], uid[dst[keep]], pos_of[src[keep]] + off[keep]], axis=1)
        if len(ue):
            if (nxt[src[keep]] >= 0).any() or (prv[dst[keep]] >= 0).any():
                raise AssertionError("a unitig edge does not run from a tail to a head")
            if (ue[:, :2] < 0).any():
                raise AssertionError("a unitig edge touches a unitig that was left out")
        ue = ue[np.lexsort((ue[:, 2], ue[:, 1], ue[:, 0]))]
    else:
        ue = np.zeros((0, 3), dtype=np.int64)
    counts = np.diff(path_off.astype(np.int64)) if P else np.zeros(0, dtype=np.int64)
    return dict(n_pairs=P, words=packed, word_off=word_off, len=ulen.astype(np.int32), path_node=path_node.astype(np.int32),
                path_pos=path_pos.astype(np.int32), path_off=path_off, edges=ue.astype(np.int32).reshape(-1, 3), uid=uid,
                info=dict(edges_in=len(np.asarray(edges).reshape(-1, 3)), edges_sym=len(star), twins_added=int(twins_added),
                          compactable=len(star) - len(ue), cycles_cut=cycles, isolated_skipped=isolated_skipped,
                          longest_nodes=int(counts.max()) if P else 0, longest_bases=int(ulen.max()) if P else 0,
                          total_bases=int(ulen.sum()), total_nodes=int(counts.sum())))


def padded_rows(u):
    """The ragged rows as a padded matrix [n_pairs, max words] (what tests/gfa_writer.py takes)."""
    P = u["n_pairs"]
    wo = u["word_off"].astype(np.int64)
    width = int(np.diff(wo).max()) if P else 1
    out = np.zeros((P, max(width, 1)), dtype=np.uint32)
    for k in range(P):
        out[k, : wo[k + 1] - wo[k]] = u["words"][wo[k]: wo[k + 1]]
    return out


def sequence(u, k):
    """ACGT string of pair k."""
    wo = u["word_off"].astype(np.int64)
    w = u["words"][wo[k]: wo[k + 1]]
    q = np.arange(int(u["len"][k]))
    return "".join("ACGT"[c] for c in ((w[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3))
