"""The definition of the merge stage (include/alga_amd.h: alga_merge_targets_device), twice, in Python.

merge_index() finds the overlaps through a dictionary of the indexed k-mers of the end sequences and the seeds of every end, finds the cycles by
counting joins per component, and builds a merged contig by appending what each further member adds.  merge_bruteforce() goes literally over
every (x, y, o), looks at the seed condition afterwards, finds cycles and paths by walking contig by contig, and takes every column of a merged
contig from the rule of item 8.  They share the refusals, the packing of bases and the rendering of the arrays, nothing else; neither shares
anything with the device's method: no column space of the ends, no keys, no directory, no pointer jumping.
Both take the targets as code arrays."""
import collections

import numpy as np

import place_checker as P
import scaffold_checker as SC

HAS_OVERLAP, AMBIGUOUS, JOINED, DROPPED_CYCLE = 1, 2, 4, 8
ARRAYS = ("partner", "olen", "mm", "hits", "end_state", "merged", "rank", "orient", "start", "overlap_after", "m_off", "m_members", "len", "col_off", "begin", "words")
COUNTERS = ("ends", "index_positions", "seeds", "seeds_over_max_occ", "ends_with_overlap", "ends_ambiguous", "hits_saturated", "joins", "joins_dropped_cycle",
            "join_mismatches", "bases_removed", "longest_overlap", "merged", "merged_multi", "longest", "columns_before", "columns_after", "n50_before", "n50_after")
DEFAULT = dict(k=21, max_mismatches=1, max_occ=256, min_overlap=42, max_overlap=512)


def check(seqs, k, max_mismatches, max_occ, min_overlap, max_overlap):
    """the refusals"""
    if not 8 <= k <= 31 or not 0 <= max_mismatches <= 254 or not 1 <= max_occ <= 65535 or not k <= min_overlap <= max_overlap or not max_overlap <= min(4096, 64 * k):
        raise ValueError("parameter out of range")
    if sum(len(s) for s in seqs) > 2 ** 32 - 2:
        raise OverflowError("more than 2^32 - 2 columns")


def check_lengths(tlen):
    """what the device checks of the target arrays: no negative length"""
    if any(int(n) < 0 for n in tlen):
        raise ValueError("negative target length")


def column_words(seqs):
    """the sequences one behind the other in column space: column g in word g >> 4 at bits 2 * (g & 15), two words of padding"""
    c = np.concatenate([np.asarray(s, np.uint32) for s in seqs] + [np.zeros(0, np.uint32)])
    words = np.zeros((len(c) + 15) // 16 + 2, dtype=np.uint32)
    i = np.arange(len(c), dtype=np.int64)
    np.bitwise_or.at(words, i >> 4, c << ((i & 15) << 1).astype(np.uint32))
    return words


def _result(seqs, per_end, joined, dropped, paths, bases, counts):
    """per_end: [(partner, olen, mm, hits)]; joined: {end: end} of the kept joins; dropped: the ends of the joins dropped for a cycle; paths:
    [[(contig, orient)]] in any order; bases: {first contig of a path: the merged contig as codes}"""
    T = len(seqs)
    tlen = [len(s) for s in seqs]
    res = dict(partner=np.array([e[0] for e in per_end], np.int32).reshape(2 * T), olen=np.array([e[1] for e in per_end], np.int32).reshape(2 * T),
               mm=np.array([e[2] for e in per_end], np.uint8).reshape(2 * T), hits=np.array([min(e[3], 255) for e in per_end], np.uint8).reshape(2 * T),
               end_state=np.array([(HAS_OVERLAP if e[3] else 0) | (AMBIGUOUS if e[3] > 1 else 0) | (JOINED if x in joined else 0) | (DROPPED_CYCLE if x in dropped else 0)
                                   for x, e in enumerate(per_end)], np.uint8).reshape(2 * T),
               merged=np.full(T, -1, np.int32), rank=np.full(T, -1, np.int32), orient=np.zeros(T, np.uint8), start=np.zeros(T, np.uint32), overlap_after=np.zeros(T, np.int32))
    paths = sorted(paths, key=lambda p: p[0][0])
    m_off, members, m_len, new = [0], [], [], []
    join_mm = removed = longest_o = 0
    for j, path in enumerate(paths):
        at = 0
        for r, (c, o) in enumerate(path):
            res["merged"][c], res["rank"][c], res["orient"][c], res["start"][c] = j, r, o, at
            at += tlen[c]
            if r + 1 < len(path):
                out = 2 * c + (o ^ 1)
                assert joined[out] == 2 * path[r + 1][0] + path[r + 1][1]
                ov = per_end[out][1]
                res["overlap_after"][c] = ov
                at -= ov
                join_mm, removed, longest_o = join_mm + per_end[out][2], removed + ov, max(longest_o, ov)
            members.append(c)
        m_off.append(len(members))
        m_len.append(at)
        assert len(bases[path[0][0]]) == at
        new.append(np.asarray(bases[path[0][0]], np.uint8))
    if max(m_len + [0]) > 2 ** 31 - 1:
        raise OverflowError("a merged contig is longer than 2^31 - 1")
    res.update(m_off=np.array(m_off, np.uint32), m_members=np.array(members, np.int32).reshape(len(members)), len=np.array(m_len, np.int32).reshape(len(paths)))
    res["col_off"] = np.concatenate([[0], np.cumsum(res["len"].astype(np.int64))]).astype(np.uint32)
    res["begin"] = res["col_off"][:-1].astype(np.uint64)
    res["words"] = column_words(new)
    info = dict(counts, ends_with_overlap=sum(1 for e in per_end if e[3]), ends_ambiguous=sum(1 for e in per_end if e[3] > 1), hits_saturated=sum(1 for e in per_end if e[3] > 255),
                joins=len(joined) // 2, joins_dropped_cycle=len(dropped) // 2, join_mismatches=join_mm, bases_removed=removed, longest_overlap=longest_o, merged=len(paths),
                merged_multi=sum(1 for p in paths if len(p) > 1), longest=max(m_len + [0]), columns_before=sum(tlen), columns_after=sum(m_len), n50_before=SC.n50(tlen),
                n50_after=SC.n50(m_len))
    res["info"] = {k: int(info[k]) for k in COUNTERS}
    return res


def _oriented(s, o):
    return P.revcomp(s) if o else np.asarray(s, np.uint8)


def merge_index(seqs, **params):
    """the definition with a dictionary index: the overlaps are the occurrences of the usable seeds"""
    p = dict(DEFAULT, **params)
    check(seqs, **p)
    k, max_mm, max_occ, min_o, max_o = (p[x] for x in ("k", "max_mismatches", "max_occ", "min_overlap", "max_overlap"))
    T = len(seqs)
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    ends = []
    for s in seqs:
        W = min(len(s) >> 1, max_o)
        ends += [P.revcomp(s[:W]), s[len(s) - W:]]
    index = collections.defaultdict(list)
    for x, E in enumerate(ends):
        for q, v in enumerate(P.kmer_values(E, k)):
            index[int(v)].append((x, q))
    counts = dict(ends=0, index_positions=sum(len(v) for v in index.values()), seeds=0, seeds_over_max_occ=0)
    per_end = []
    for x, E in enumerate(ends):
        W = len(E)
        found = set()
        if W >= min_o:
            counts["ends"] += 1
            Px = P.revcomp(E)
            for j, v in enumerate(P.kmer_values(Px, k)[::k]):
                counts["seeds"] += 1
                at = index.get(int(v), ())
                counts["seeds_over_max_occ"] += len(at) > max_occ
                if not 1 <= len(at) <= max_occ:
                    continue
                for y, q in at:
                    Wy = len(ends[y])
                    o = Wy - q + j * k                                    # P_x[jk] lies on E_y[q], the overlap ends with E_y
                    if y >> 1 == x >> 1 or not min_o <= o <= min(W, Wy):
                        continue
                    mm = int((Px[:o] != ends[y][Wy - o:]).sum())
                    if mm <= max_mm:
                        found.add((mm, y, -o))
        if found:
            mm, y, o = min(found)
            per_end.append((y, -o, mm, len(found)))
        else:
            per_end.append((-1, 0, 0, 0))
    joined = {}
    for x, (y, o, _, hits) in enumerate(per_end):
        if hits == 1 and per_end[y][3] == 1 and per_end[y][0] == x and per_end[y][1] == o:
            joined[x] = y
    # components of the contigs under the joins: one is a cycle iff it has as many joins as contigs
    comp = list(range(T))

    def find(c):
        while comp[c] != c:
            comp[c] = comp[comp[c]]
            c = comp[c]
        return c
    for a, b in joined.items():
        comp[find(a >> 1)] = find(b >> 1)
    n_contigs, n_ends = collections.Counter(find(c) for c in range(T)), collections.Counter(find(a >> 1) for a in joined)
    dropped = set()
    for root, n in n_ends.items():
        if n == 2 * n_contigs[root]:
            c = min(x for x in range(T) if find(x) == root)
            dropped.update((2 * c, joined[2 * c]))
    for a in dropped:
        del joined[a]
    # every path from its smaller terminal; a merged contig is its first member and what every further one adds
    paths, bases, seen = [], {}, set()
    for c in range(T):
        if len(seqs[c]) == 0 or c in seen:
            continue
        free = [e for e in (0, 1) if 2 * c + e not in joined]
        if not free:
            continue                                                # an inner contig: its path is found from a terminal
        path, x = [], 2 * c + free[0]
        while True:
            path.append((x >> 1, x & 1))
            if x ^ 1 not in joined:
                break
            x = joined[x ^ 1]
        if path[-1][0] < c:
            continue                                                # the other terminal has the smaller id: laid out from there
        seen.update(m for m, _ in path)
        paths.append(path)
        parts, cut = [], 0
        for m, o in path:
            parts.append(_oriented(seqs[m], o)[cut:])
            cut = per_end[2 * m + (o ^ 1)][1] if 2 * m + (o ^ 1) in joined else 0
        bases[c] = np.concatenate(parts)
    return _result(seqs, per_end, joined, dropped, paths, bases, counts)


def merge_bruteforce(seqs, **params):
    """the definition walked literally: every (x, y, o), the Hamming distance first, then whether a usable seed lies in the overlap and matches;
    cycles and paths by walking contig by contig; every column from the rule of item 8"""
    p = dict(DEFAULT, **params)
    check(seqs, **p)
    k, min_o = p["k"], p["min_overlap"]
    T = len(seqs)
    E = []
    for t in range(T):
        s = np.asarray(seqs[t], np.uint8)
        W = min(len(s) // 2, p["max_overlap"])
        E.append((3 - s[:W])[::-1])
        E.append(s[len(s) - W:] if W else s[:0])
    occ = collections.Counter()
    for e in E:
        occ.update(int(v) for v in P.kmer_values(e, k))
    n_ends = n_seeds = n_over = 0
    per_end = []
    for x in range(2 * T):
        Wx = len(E[x])
        best, n = None, 0
        if Wx >= min_o:
            n_ends += 1
            Px = (3 - E[x])[::-1]
            seeds = [int(v) for v in P.kmer_values(Px, k)[::k]]
            n_seeds += len(seeds)
            n_over += sum(occ[v] > p["max_occ"] for v in seeds)
            usable = [1 <= occ[v] <= p["max_occ"] for v in seeds]
            for y in range(2 * T):
                if y // 2 == x // 2:
                    continue
                Wy = len(E[y])
                for o in range(min_o, min(Wx, Wy) + 1):
                    diff = Px[:o] != E[y][Wy - o:]
                    mm = int(diff.sum())
                    if mm > p["max_mismatches"]:
                        continue
                    if not any(usable[j] and not diff[j * k:j * k + k].any() for j in range(o // k)):
                        continue
                    n += 1
                    key = (mm, y, -o)
                    best = key if best is None or key < best else best
        per_end.append((best[1], -best[2], best[0], n) if best else (-1, 0, 0, 0))
    joined = {}
    for x in range(2 * T):
        y = per_end[x][0]
        if per_end[x][3] == 1 and per_end[y][3] == 1 and per_end[y][0] == x and per_end[x][1] == per_end[y][1]:
            joined[x] = y
    dropped = set()
    for c in range(T):                                              # leave c at its right end and go on: back at c is a cycle
        x, low = 2 * c + 1, c
        while x in joined:
            y = joined[x]
            if y >> 1 == c:
                if low == c:
                    dropped.update((2 * c, joined[2 * c]))
                break
            low = min(low, y >> 1)
            x = y ^ 1
    for a in dropped:
        del joined[a]
    paths, bases, placed = [], {}, set()
    for c in range(T):
        if len(seqs[c]) == 0 or c in placed:
            continue
        far = []
        for x in (2 * c, 2 * c + 1):                                # out of c through x as far as the joins go
            while x in joined:
                x = joined[x] ^ 1
            far.append(x)
        a, b = far
        x = 2 * c if a >> 1 == b >> 1 == c else a if a >> 1 < b >> 1 else b     # the free end of the smaller terminal
        path = []
        while True:
            path.append((x >> 1, x & 1))
            placed.add(x >> 1)
            if x ^ 1 not in joined:
                break
            x = joined[x ^ 1]
        paths.append(path)
        # the layout, then every column by the rule
        start, at = [], 0
        for m, o in path:
            start.append(at)
            out = 2 * m + (o ^ 1)
            at += len(seqs[m]) - (per_end[out][1] if out in joined else 0)
        total = start[-1] + len(seqs[path[-1][0]])
        col = np.zeros(total, np.uint8)
        for q in range(total):
            r = max(i for i in range(len(path)) if start[i] <= q)
            if r > 0 and q < start[r - 1] + len(seqs[path[r - 1][0]]):
                r -= 1
            m, o = path[r]
            s = np.asarray(seqs[m], np.uint8)
            col[q] = 3 - s[len(s) - 1 - (q - start[r])] if o else s[q - start[r]]
        bases[path[0][0]] = col
    counts = dict(ends=n_ends, index_positions=int(sum(occ.values())), seeds=n_seeds, seeds_over_max_occ=int(n_over))
    return _result(seqs, per_end, joined, dropped, paths, bases, counts)


def sequences(res):
    """the merged contigs as code arrays"""
    return [P.codes_of(res["words"], int(res["col_off"][j]), int(res["len"][j])) for j in range(len(res["len"]))]


def fasta(res):
    """the merged FASTA as bytes: one record per merged contig"""
    out = []
    for j, s in enumerate(sequences(res)):
        out.append(">contig_id=%d_length=%d_contigs=%d\n%s\n" % (j, len(s), int(res["m_off"][j + 1]) - int(res["m_off"][j]), "".join("ACGT"[x] for x in s)))
    return "".join(out).encode()


def merge_tsv(res, tlen):
    """one line per member in (merged, rank) order: merged rank contig orient start length overlap_after mm"""
    out = []
    for j in range(len(res["len"])):
        for c in res["m_members"][int(res["m_off"][j]):int(res["m_off"][j + 1])]:
            left_at = 2 * int(c) + (1 - int(res["orient"][c]))
            out.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, res["rank"][c], c, "-" if res["orient"][c] else "+", res["start"][c], tlen[c], res["overlap_after"][c],
                                                          res["mm"][left_at] if res["overlap_after"][c] else 0))
    return "".join(out).encode()
