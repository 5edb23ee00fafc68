"""The definition of the scaffolds (include/alga_amd.h: alga_scaffold_placed_device), twice, in Python.

scaffold_dicts() keeps a dictionary per pair key, then one per end, finds the cycles by counting joins per connected component and lays a path
out from its smaller terminal.  scaffold_walk() asks, for every (bundle, end), every other bundle at that end whether it beats or rivals it,
finds the cycles by walking from every contig until it comes back, and lays the scaffolds out by following the joins contig by contig.
Neither shares anything with the device's method: no sorted link array, no heads, no atomics, no pointer jumping.
Both take a placement as tests/place_checker.py returns it (target, pos, state, col_off)."""
import numpy as np

import place_checker as P

B_SUPPORTED, B_JOIN, B_DROPPED_CYCLE = 1, 2, 4
E_HAS_SUPPORTED, E_AMBIGUOUS, E_JOINED = 1, 2, 4
ARRAYS = ("b_a", "b_b", "b_links", "b_span", "b_gap", "b_state", "end_state", "scaffold", "rank", "orient", "start", "gap_after", "join_links", "s_off", "s_members",
          "s_len")
COUNTERS = ("pairs_split", "links", "links_too_far", "bundles", "bundles_supported", "ends_ambiguous", "joins", "joins_dropped_cycle", "scaffolds", "scaffolds_multi",
            "longest", "n50_targets", "n50_scaffolds")
DEFAULT = dict(max_insert=1000, min_links=5, max_second_percent=50, min_gap=10)


def check(rows, lens, pair_off, pl, insert, max_insert, min_links, max_second_percent, min_gap):
    """the refusals -> the split pairs as (end, reach, end, reach)"""
    if not 0 <= insert <= 2 ** 20 or not 1 <= max_insert <= 2 ** 20 or not 1 <= min_links <= 2 ** 31 - 1 or not 1 <= max_second_percent <= 100 or \
            not 1 <= min_gap <= 2 ** 20:
        raise ValueError("parameter out of range")
    n = len(lens)
    if n % 2 or n // 2 != len(pl["state"]):
        raise ValueError("not the node set that was placed")
    if pair_off is not None:
        for v in range(n):
            po = int(pair_off[v])
            if po > 2 or po != pair_off[v ^ 1] or (po == 1 and (v + 2 >= n or pair_off[v + 2] != 2)) or (po == 2 and (v < 2 or pair_off[v - 2] != 1)):
                raise ValueError("pair_off")
    col_off = pl["col_off"].astype(np.int64)
    tlen = col_off[1:] - col_off[:-1]
    stride = rows.shape[1] if n else 0
    reach = {}
    for r in range(n // 2):
        st = int(pl["state"][r])
        if not st & P.UNIQUE:
            continue
        L, t, p = int(lens[2 * r + 1]), int(pl["target"][r]), int(pl["pos"][r])
        if L < 1 or L > 16 * stride:
            raise ValueError("read length")
        if not 0 <= t < len(tlen) or p < 0 or p + L > tlen[t]:
            raise ValueError("a read leaves its target")
        reach[r] = (2 * t, p + L) if st & P.MINUS else (2 * t + 1, int(tlen[t]) - p)
    split = []
    if pair_off is not None:
        for r in range(n // 2):
            if pair_off[2 * r + 1] == 1 and r in reach and r + 1 in reach and reach[r][0] >> 1 != reach[r + 1][0] >> 1:
                split.append(reach[r] + reach[r + 1])
    return split, tlen


def n50(lengths):
    """the largest length l such that the sequences of length >= l hold at least half of all bases; 0 for an empty set"""
    v = sorted((int(x) for x in lengths), reverse=True)
    total, cum = sum(v), 0
    if total == 0:
        return 0
    for x in v:
        cum += x
        if 2 * cum >= total:
            return x


def _result(tlen, bundles, bstate, estate, paths, gap_of, counts, min_gap):
    """bundles: [(a, b, n, S, gap)] ascending; paths: [[(contig, orient)]] in any order; gap_of: {frozenset of two ends: (gap, n)} of the kept joins"""
    T = len(tlen)
    res = dict(b_a=np.array([b[0] for b in bundles], np.uint32), b_b=np.array([b[1] for b in bundles], np.uint32), b_links=np.array([b[2] for b in bundles], np.uint32),
               b_span=np.array([b[3] for b in bundles], np.uint64), b_gap=np.array([b[4] for b in bundles], np.int32), b_state=np.array(bstate, np.uint8),
               end_state=np.array(estate, np.uint8), scaffold=np.full(T, -1, np.int32), rank=np.full(T, -1, np.int32), orient=np.zeros(T, np.uint8),
               start=np.zeros(T, np.uint64), gap_after=np.zeros(T, np.int32), join_links=np.zeros(T, np.uint32))
    paths = sorted(paths, key=lambda p: p[0][0])
    s_off, members, s_len = [0], [], []
    for j, path in enumerate(paths):
        at = 0
        for k, (c, o) in enumerate(path):
            res["scaffold"][c], res["rank"][c], res["orient"][c], res["start"][c] = j, k, o, at
            at += int(tlen[c])
            if k + 1 < len(path):
                out, into = 2 * c + (o ^ 1), 2 * path[k + 1][0] + path[k + 1][1]
                gap, n = gap_of[frozenset((out, into))]
                res["gap_after"][c], res["join_links"][c] = max(gap, min_gap), n
                at += max(gap, min_gap)
            members.append(c)
        s_off.append(len(members))
        s_len.append(at)
    res.update(s_off=np.array(s_off, np.uint32), s_members=np.array(members, np.int32), s_len=np.array(s_len, np.uint64))
    info = dict(counts, bundles=len(bundles), bundles_supported=sum(1 for s in bstate if s & B_SUPPORTED), ends_ambiguous=sum(1 for s in estate if s & E_AMBIGUOUS),
                joins=sum(1 for s in bstate if s & B_JOIN and not s & B_DROPPED_CYCLE), joins_dropped_cycle=sum(1 for s in bstate if s & B_DROPPED_CYCLE),
                scaffolds=len(paths), scaffolds_multi=sum(1 for p in paths if len(p) > 1), longest=max(s_len + [0]), n50_targets=n50(tlen), n50_scaffolds=n50(s_len))
    res["info"] = info
    return res


def scaffold_dicts(rows, lens, pair_off, pl, insert, max_insert=1000, min_links=5, max_second_percent=50, min_gap=10):
    """dictionaries per pair key, then per end; cycles by counting; a path laid out from its smaller terminal"""
    split, tlen = check(rows, lens, pair_off, pl, insert, max_insert, min_links, max_second_percent, min_gap)
    T = len(tlen)
    per_key, far = {}, 0
    for x1, d1, x2, d2 in split:
        if d1 + d2 > max_insert:
            far += 1
            continue
        e = per_key.setdefault((min(x1, x2), max(x1, x2)), [0, 0])
        e[0] += 1
        e[1] += d1 + d2
    keys = sorted(per_key)
    bundles = [(a, b, per_key[a, b][0], per_key[a, b][1], insert - per_key[a, b][1] // per_key[a, b][0]) for a, b in keys]
    per_end = {}
    for a, b, n, _, _ in bundles:
        if n >= min_links:
            per_end.setdefault(a, []).append((-n, b))
            per_end.setdefault(b, []).append((-n, a))
    choice, estate = {}, [0] * (2 * T)
    for x, lst in per_end.items():
        lst.sort()
        estate[x] |= E_HAS_SUPPORTED
        if len(lst) > 1 and 100 * -lst[1][0] >= max_second_percent * -lst[0][0]:
            estate[x] |= E_AMBIGUOUS
        else:
            choice[x] = lst[0][1]
    joined = {}                                                     # end -> partner end
    for a, b, n, _, _ in bundles:
        if n >= min_links and choice.get(a) == b and choice.get(b) == a:
            joined[a], joined[b] = b, a
    # components of the contigs under the joins: one is a cycle iff it has as many joins as contigs
    comp = list(range(T))

    def find(c):
        while comp[c] != c:
            comp[c] = comp[comp[c]]
            c = comp[c]
        return c
    for a, b in joined.items():
        comp[find(a >> 1)] = find(b >> 1)
    n_contigs, n_ends = {}, {}
    for c in range(T):
        n_contigs[find(c)] = n_contigs.get(find(c), 0) + 1
    for a in joined:
        n_ends[find(a >> 1)] = n_ends.get(find(a >> 1), 0) + 1
    dropped = set()
    for root, k in n_ends.items():
        if k == 2 * n_contigs[root]:
            c = min(x for x in range(T) if find(x) == root)
            dropped.add((min(2 * c, joined[2 * c]), max(2 * c, joined[2 * c])))
    for a, b in dropped:
        del joined[a], joined[b]
    bstate = []
    for a, b, n, _, _ in bundles:
        st = B_SUPPORTED if n >= min_links else 0
        if (a, b) in dropped:
            st |= B_JOIN | B_DROPPED_CYCLE
        elif joined.get(a) == b:
            st |= B_JOIN
        bstate.append(st)
    for x in joined:
        estate[x] |= E_JOINED
    gap_of = {frozenset((a, b)): (g, n) for a, b, n, _, g in bundles if joined.get(a) == b}
    # every path from its smaller terminal
    paths, seen = [], set()
    for c in range(T):
        if tlen[c] == 0 or c in seen:
            continue
        free = [e for e in (0, 1) if 2 * c + e not in joined]
        if not free:
            continue                                                # an inner contig: its path is found from a terminal
        if len(free) == 2:
            paths.append([(c, 0)])
            seen.add(c)
            continue
        path, x = [], 2 * c + free[0]
        while True:
            path.append((x >> 1, x & 1))
            if x ^ 1 not in joined:
                break
            x = joined[x ^ 1]
        if path[-1][0] < c:
            continue                                                # the other terminal has the smaller id: laid out from there
        seen.update(p[0] for p in path)
        paths.append(path)
    counts = dict(pairs_split=len(split), links=sum(b[2] for b in bundles), links_too_far=far)
    return _result(tlen, bundles, bstate, estate, paths, gap_of, counts, min_gap)


def scaffold_walk(rows, lens, pair_off, pl, insert, max_insert=1000, min_links=5, max_second_percent=50, min_gap=10):
    """every (bundle, end) against every other bundle at that end; cycles and scaffolds by walking contig by contig"""
    split, tlen = check(rows, lens, pair_off, pl, insert, max_insert, min_links, max_second_percent, min_gap)
    T = len(tlen)
    links = [(min(x1, x2), max(x1, x2), d1 + d2) for x1, d1, x2, d2 in split if d1 + d2 <= max_insert]
    bundles = []
    for a, b in sorted({(a, b) for a, b, _ in links}):
        spans = [s for x, y, s in links if (x, y) == (a, b)]
        bundles.append((a, b, len(spans), sum(spans), insert - sum(spans) // len(spans)))
    sup = [b for b in bundles if b[2] >= min_links]
    estate = [0] * (2 * T)

    def chooses(x, y, n):
        """the bundle of n links to y is the choice of end x"""
        others = [(b[2], b[0] + b[1] - x) for b in sup if x in b[:2] and b[0] + b[1] - x != y]
        if any(m > n or (m == n and z < y) for m, z in others):
            return False                                            # it is not the first
        return not any(100 * m >= max_second_percent * n for m, _ in others)
    for b in sup:
        for x in b[:2]:
            estate[x] |= E_HAS_SUPPORTED
            n1 = max(c[2] for c in sup if x in c[:2])
            if sum(1 for c in sup if x in c[:2] and 100 * c[2] >= max_second_percent * n1) > 1:
                estate[x] |= E_AMBIGUOUS
    joined = {}
    for a, b, n, _, _ in sup:
        if chooses(a, b, n) and chooses(b, a, n):
            joined[a], joined[b] = b, a
    dropped = []
    for c in range(T):                                              # leave c at its right end and go on: back at c is a cycle
        x, low = 2 * c + 1, c
        while x in joined:
            y = joined[x]
            if y >> 1 == c:
                if low == c:
                    dropped.append((min(2 * c, joined[2 * c]), max(2 * c, joined[2 * c])))
                break
            low = min(low, y >> 1)
            x = y ^ 1
    for a, b in dropped:
        del joined[a], joined[b]
    bstate = [(B_SUPPORTED if b[2] >= min_links else 0) | (B_JOIN if joined.get(b[0]) == b[1] or b[:2] in dropped else 0) | (B_DROPPED_CYCLE if b[:2] in dropped else 0)
              for b in bundles]
    for x in joined:
        estate[x] |= E_JOINED
    gap_of = {frozenset(b[:2]): (b[4], b[2]) for b in bundles if joined.get(b[0]) == b[1]}
    paths, placed = [], set()
    for c in range(T):
        if tlen[c] == 0 or c in placed:
            continue
        ends = []
        for x in (2 * c, 2 * c + 1):                                # out of c through x as far as the joins go
            while x in joined:
                x = joined[x] ^ 1
            ends.append(x)
        a, b = ends
        x = 2 * c if a >> 1 == b >> 1 == c else a if a >> 1 < b >> 1 else b     # the free end of the smaller terminal
        path = []
        while True:
            path.append((x >> 1, x & 1))
            placed.add(x >> 1)
            if x ^ 1 not in joined:
                break
            x = joined[x ^ 1]
        paths.append(path)
    counts = dict(pairs_split=len(split), links=len(links), links_too_far=len(split) - len(links))
    return _result(tlen, bundles, bstate, estate, paths, gap_of, counts, min_gap)


def target_codes(twords, tbegin, tlen):
    return [P.codes_of(twords, tbegin[t], int(tlen[t])) for t in range(len(tlen))]


def fasta(res, seqs):
    """the scaffold FASTA as bytes; seqs: the targets as code arrays"""
    out = []
    for j in range(len(res["s_len"])):
        mem = res["s_members"][int(res["s_off"][j]):int(res["s_off"][j + 1])]
        out.append(">scaffold_id=%d_length=%d_contigs=%d\n" % (j, int(res["s_len"][j]), len(mem)))
        for c in mem:
            s = P.revcomp(seqs[c]) if res["orient"][c] else seqs[c]
            out.append("".join("ACGT"[x] for x in s) + "N" * int(res["gap_after"][c]))
        out.append("\n")
    return "".join(out).encode()


def layout_tsv(res, tlen):
    """one line per member contig in (scaffold, rank) order: scaffold rank contig orient start length gap_after links"""
    out = []
    for j in range(len(res["s_len"])):
        for c in res["s_members"][int(res["s_off"][j]):int(res["s_off"][j + 1])]:
            out.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, res["rank"][c], c, "-" if res["orient"][c] else "+", res["start"][c], tlen[c], res["gap_after"][c],
                                                          res["join_links"][c]))
    return "".join(out).encode()
