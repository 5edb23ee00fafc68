"""The definition of the stitch stage (include/alga_amd.h: alga_stitch_targets_device), twice, in Python.

stitch_windows() takes the end windows E_x and P_x as numpy arrays and compares a whole overlap length at a time, finds the cycles by counting
stitches per component, and builds a stitched contig by appending what each further member adds.  stitch_literal() goes over every (j, o) base
by base from the target sequences themselves -- no E or P arrays: it indexes the oriented contigs directly --, finds cycles and paths by
walking contig by contig, and takes every column of a stitched contig from the rule of item 8 of the merge definition.  They share the
refusals, the packing of bases and the rendering of the arrays, nothing else; neither shares anything with the device's method: no LDS
windows, no words, no funnel shifts, no pointer jumping.
Both take the targets as code arrays and the entries as (a, b, gap, state or None)."""
import collections

import numpy as np

import merge_checker as MC
import place_checker as P
import scaffold_checker as SC

SELECTED, HAS_OVERLAP, AMBIGUOUS, STITCHED, DROPPED_CYCLE = 1, 2, 4, 8, 16
BUNDLE_JOIN, BUNDLE_DROPPED_CYCLE = 2, 4                           # ALGA_SCAFFOLD_BUNDLE_* of the entries' state
ARRAYS = ("j_olen", "j_mm", "j_hits", "j_state", "end_entry", "stitched", "rank", "orient", "start", "overlap_after", "s_off", "s_members", "len", "col_off", "begin",
          "words")
COUNTERS = ("entries", "selected", "with_overlap", "ambiguous", "hits_saturated", "candidates_outside_slack", "stitched", "dropped_cycle", "join_mismatches",
            "bases_removed", "longest_overlap", "contigs", "contigs_multi", "longest", "columns_before", "columns_after", "n50_before", "n50_after")
DEFAULT = dict(max_mismatches=2, min_overlap=16, max_overlap=512, slack=2 ** 20)


def entries_of(a=(), b=(), gap=(), state=None):
    """the entry list in the dtypes of the C ABI"""
    return (np.asarray(a, np.uint32).reshape(-1), np.asarray(b, np.uint32).reshape(-1), np.asarray(gap, np.int32).reshape(-1),
            None if state is None else np.asarray(state, np.uint8).reshape(-1))


def check_lengths(tlen):
    """what the device checks of the target arrays: no negative length"""
    MC.check_lengths(tlen)


def check(seqs, entries, max_mismatches, min_overlap, max_overlap, slack):
    """the refusals -> the selected entries"""
    if not 0 <= max_mismatches <= 254 or not 8 <= min_overlap <= max_overlap <= 4096 or not 0 <= slack <= 2 ** 20:
        raise ValueError("parameter out of range")
    a, b, gap, state = entries
    if not len(a) == len(b) == len(gap) or (state is not None and len(state) != len(a)):
        raise ValueError("entry arrays of different lengths")
    if len(a) > 2 ** 31 - 1:
        raise OverflowError("more than 2^31 - 1 entries")
    T = len(seqs)
    sel = [j for j in range(len(a)) if state is None or (int(state[j]) & BUNDLE_JOIN and not int(state[j]) & BUNDLE_DROPPED_CYCLE)]
    named = collections.Counter()
    for j in sel:
        if int(a[j]) >= 2 * T or int(b[j]) >= 2 * T:
            raise ValueError("entry %d names an end that is not below 2 T" % j)
        if int(a[j]) >> 1 == int(b[j]) >> 1:
            raise ValueError("entry %d names two ends of one target" % j)
        named.update((int(a[j]), int(b[j])))
    if any(n > 1 for n in named.values()):
        raise ValueError("an end is named by more than one selected entry")
    if sum(len(s) for s in seqs) > 2 ** 32 - 2:
        raise OverflowError("more than 2^32 - 2 columns")
    return sel


def _result(seqs, entries, sel, per_entry, kept, dropped, outside, paths, bases):
    """per_entry: {j: (olen, mm, hits)} of the selected entries; kept: {end: (end, j)} of the stitches that are left; dropped: the entries
    dropped for a cycle; outside: the candidates outside the slack; paths: [[(contig, orient)]] in any order; bases: {first contig of a path:
    the stitched contig as codes}"""
    T, J = len(seqs), len(entries[0])
    tlen = [len(s) for s in seqs]
    res = dict(j_olen=np.zeros(J, np.int32), j_mm=np.zeros(J, np.uint8), j_hits=np.zeros(J, np.uint8), j_state=np.zeros(J, np.uint8), end_entry=np.full(2 * T, -1, np.int32),
               stitched=np.full(T, -1, np.int32), rank=np.full(T, -1, np.int32), orient=np.zeros(T, np.uint8), start=np.zeros(T, np.uint32), overlap_after=np.zeros(T, np.int32))
    kept_entries = {j for _, j in kept.values()}
    for j in sel:
        olen, mm, hits = per_entry[j]
        res["j_olen"][j], res["j_mm"][j], res["j_hits"][j] = olen, mm, min(hits, 255)
        res["j_state"][j] = SELECTED | (HAS_OVERLAP if hits else 0) | (AMBIGUOUS if hits > 1 else 0) | (STITCHED if j in kept_entries else 0) | (DROPPED_CYCLE if j in dropped else 0)
        res["end_entry"][int(entries[0][j])] = res["end_entry"][int(entries[1][j])] = j
    paths = sorted(paths, key=lambda p: p[0][0])
    s_off, members, s_len, new = [0], [], [], []
    join_mm = removed = longest_o = 0
    for i, path in enumerate(paths):
        at = 0
        for r, (c, o) in enumerate(path):
            res["stitched"][c], res["rank"][c], res["orient"][c], res["start"][c] = i, r, o, at
            at += tlen[c]
            if r + 1 < len(path):
                out = 2 * c + (o ^ 1)
                y, j = kept[out]
                assert y == 2 * path[r + 1][0] + path[r + 1][1]
                ov, mm, _ = per_entry[j]
                res["overlap_after"][c] = ov
                at -= ov
                join_mm, removed, longest_o = join_mm + mm, removed + ov, max(longest_o, ov)
            members.append(c)
        s_off.append(len(members))
        s_len.append(at)
        assert len(bases[path[0][0]]) == at
        new.append(np.asarray(bases[path[0][0]], np.uint8))
    if max(s_len + [0]) > 2 ** 31 - 1:
        raise OverflowError("a stitched contig is longer than 2^31 - 1")
    res.update(s_off=np.array(s_off, np.uint32), s_members=np.array(members, np.int32).reshape(len(members)), len=np.array(s_len, np.int32).reshape(len(paths)))
    res["col_off"] = np.concatenate([[0], np.cumsum(res["len"].astype(np.int64))]).astype(np.uint32)
    res["begin"] = res["col_off"][:-1].astype(np.uint64)
    res["words"] = MC.column_words(new)
    hits = [per_entry[j][2] for j in sel]
    info = dict(entries=J, selected=len(sel), with_overlap=sum(1 for h in hits if h), ambiguous=sum(1 for h in hits if h > 1), hits_saturated=sum(1 for h in hits if h > 255),
                candidates_outside_slack=outside, stitched=len(kept) // 2, dropped_cycle=len(dropped), join_mismatches=join_mm, bases_removed=removed,
                longest_overlap=longest_o, contigs=len(paths), contigs_multi=sum(1 for p in paths if len(p) > 1), longest=max(s_len + [0]), columns_before=sum(tlen),
                columns_after=sum(s_len), n50_before=SC.n50(tlen), n50_after=SC.n50(s_len))
    res["info"] = {k: int(info[k]) for k in COUNTERS}
    return res


def _judge(found, gap, slack):
    """found: [(mm, o)] of the candidates -> (olen, mm, hits), the candidates outside the slack"""
    adm = [(mm, -o) for mm, o in found if abs(int(gap) + o) <= slack]
    if not adm:
        return (0, 0, 0), len(found)
    mm, o = min(adm)
    return (-o, mm, len(adm)), len(found) - len(adm)


def stitch_windows(seqs, entries, **params):
    """the definition over the end windows: E_x and P_x as arrays, an overlap length compared at once"""
    p = dict(DEFAULT, **params)
    sel = check(seqs, entries, **p)
    max_mm, min_o, max_o, slack = (p[x] for x in ("max_mismatches", "min_overlap", "max_overlap", "slack"))
    T = len(seqs)
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    E = []
    for s in seqs:
        W = min(len(s) >> 1, max_o)
        E += [P.revcomp(s[:W]), s[len(s) - W:]]
    Pw = [P.revcomp(e) for e in E]
    per_entry, outside = {}, 0
    for j in sel:
        a, b, gap = int(entries[0][j]), int(entries[1][j]), int(entries[2][j])
        Wa, Wb = len(E[a]), len(E[b])
        found = []
        for o in range(min_o, min(Wa, Wb) + 1):
            mm = int((Pw[a][:o] != E[b][Wb - o:]).sum())
            assert mm == int((Pw[b][:o] != E[a][Wa - o:]).sum())     # the same seen from b
            if mm <= max_mm:
                found.append((mm, o))
        per_entry[j], out = _judge(found, gap, slack)
        outside += out
    kept = {}
    for j in sel:
        if per_entry[j][2] == 1:
            a, b = int(entries[0][j]), int(entries[1][j])
            kept[a], kept[b] = (b, j), (a, j)
    # components of the contigs under the stitches: one is a cycle iff it has as many stitches as contigs
    comp = list(range(T))

    def find(c):
        while comp[c] != c:
            comp[c] = comp[comp[c]]
            c = comp[c]
        return c
    for x, (y, _) in kept.items():
        comp[find(x >> 1)] = find(y >> 1)
    n_contigs, n_ends = collections.Counter(find(c) for c in range(T)), collections.Counter(find(x >> 1) for x in kept)
    dropped = set()
    for root, n in n_ends.items():
        if n == 2 * n_contigs[root]:
            c = min(x for x in range(T) if find(x) == root)
            y, j = kept[2 * c]
            dropped.add(j)
            del kept[2 * c], kept[y]
    paths, bases, seen = [], {}, set()
    for c in range(T):
        if len(seqs[c]) == 0 or c in seen:
            continue
        free = [e for e in (0, 1) if 2 * c + e not in kept]
        if not free:
            continue                                                # an inner contig: its path is found from a terminal
        path, x = [], 2 * c + free[0]
        while True:
            path.append((x >> 1, x & 1))
            if x ^ 1 not in kept:
                break
            x = kept[x ^ 1][0]
        if path[-1][0] < c:
            continue                                                # the other terminal has the smaller id: laid out from there
        seen.update(m for m, _ in path)
        paths.append(path)
        parts, cut = [], 0
        for m, o in path:
            parts.append((P.revcomp(seqs[m]) if o else seqs[m])[cut:])
            out = 2 * m + (o ^ 1)
            cut = per_entry[kept[out][1]][0] if out in kept else 0
        bases[c] = np.concatenate(parts)
    return _result(seqs, entries, sel, per_entry, kept, dropped, outside, paths, bases)


def stitch_literal(seqs, entries, **params):
    """the definition walked literally: every (j, o) base by base on the oriented contigs (a read so that end a is at its left, b so that end b
    is at its right: the overlap is the first o bases of the one on the last o of the other); cycles and paths by walking contig by contig;
    every column from the rule of item 8 of the merge definition"""
    p = dict(DEFAULT, **params)
    sel = check(seqs, entries, **p)
    max_mm, min_o, max_o, slack = (p[x] for x in ("max_mismatches", "min_overlap", "max_overlap", "slack"))
    T = len(seqs)
    seqs = [[int(x) for x in s] for s in seqs]

    def base(c, flip, i):                                           # base i of contig c, of its reverse complement where flip
        s = seqs[c]
        return 3 - s[len(s) - 1 - i] if flip else s[i]
    per_entry, outside = {}, 0
    for j in sel:
        a, b, gap = int(entries[0][j]), int(entries[1][j]), int(entries[2][j])
        ca, cb = a >> 1, b >> 1
        fa, fb = a & 1, (b & 1) ^ 1                                 # end a at the left: the right end turned; end b at the right: the left end turned
        nb = len(seqs[cb])
        found = []
        for o in range(min_o, min(len(seqs[ca]) // 2, nb // 2, max_o) + 1):
            mm = 0
            for i in range(o):
                mm += base(ca, fa, i) != base(cb, fb, nb - o + i)
                if mm > max_mm:
                    break
            if mm <= max_mm:
                found.append((mm, o))
        per_entry[j], out = _judge(found, gap, slack)
        outside += out
    kept = {}
    for j in sel:
        if per_entry[j][2] == 1:
            a, b = int(entries[0][j]), int(entries[1][j])
            kept[a], kept[b] = (b, j), (a, j)
    dropped = set()
    for c in range(T):                                              # leave c at its right end and go on: back at c is a cycle
        x, low = 2 * c + 1, c
        while x in kept:
            y = kept[x][0]
            if y >> 1 == c:
                if low == c:
                    dropped.add(kept[2 * c][1])
                break
            low = min(low, y >> 1)
            x = y ^ 1
    for x in [x for x, (_, j) in kept.items() if j in dropped]:
        del kept[x]
    paths, bases, placed = [], {}, set()
    for c in range(T):
        if len(seqs[c]) == 0 or c in placed:
            continue
        far = []
        for x in (2 * c, 2 * c + 1):                                # out of c through x as far as the stitches go
            while x in kept:
                x = kept[x][0] ^ 1
            far.append(x)
        a, b = far
        x = 2 * c if a >> 1 == b >> 1 == c else a if a >> 1 < b >> 1 else b     # the free end of the smaller terminal
        path = []
        while True:
            path.append((x >> 1, x & 1))
            placed.add(x >> 1)
            if x ^ 1 not in kept:
                break
            x = kept[x ^ 1][0]
        paths.append(path)
        start, at = [], 0
        for m, o in path:
            start.append(at)
            out = 2 * m + (o ^ 1)
            at += len(seqs[m]) - (per_entry[kept[out][1]][0] if out in kept else 0)
        total = start[-1] + len(seqs[path[-1][0]])
        col = np.zeros(total, np.uint8)
        for q in range(total):
            r = max(i for i in range(len(path)) if start[i] <= q)
            if r > 0 and q < start[r - 1] + len(seqs[path[r - 1][0]]):
                r -= 1
            col[q] = base(path[r][0], path[r][1], q - start[r])
        bases[path[0][0]] = col
    return _result([np.asarray(s, np.uint8) for s in seqs], entries, sel, per_entry, kept, dropped, outside, paths, bases)


def sequences(res):
    """the stitched contigs as code arrays"""
    return [P.codes_of(res["words"], int(res["col_off"][j]), int(res["len"][j])) for j in range(len(res["len"]))]


def fasta(res):
    """the stitched FASTA as bytes: one record per stitched contig (the merge stage's record)"""
    return MC.fasta(dict(words=res["words"], col_off=res["col_off"], len=res["len"], m_off=res["s_off"]))


def stitch_tsv(res, tlen):
    """one line per member in (stitched, rank) order: stitched rank contig orient start length overlap_after mm"""
    out = []
    for j in range(len(res["len"])):
        for c in res["s_members"][int(res["s_off"][j]):int(res["s_off"][j + 1])]:
            left_at = 2 * int(c) + (1 - int(res["orient"][c]))
            out.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, res["rank"][c], c, "-" if res["orient"][c] else "+", res["start"][c], tlen[c], res["overlap_after"][c],
                                                          res["j_mm"][res["end_entry"][left_at]] if res["overlap_after"][c] else 0))
    return "".join(out).encode()
