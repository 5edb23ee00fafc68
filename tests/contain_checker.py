"""The definition of the containment stage (include/alga_amd.h: alga_drop_contained_device), twice, in Python.

contain_index() finds the containers through a dictionary of the indexed k-mers of the targets to the candidate diagonals (h, p) of every query,
and finds the roots by walking host by host.  contain_bruteforce() goes literally over every (c, h, p, s) with the Hamming distance by numpy,
looks at the seed condition afterwards (the occurrences counted over one array of all k-mers), and takes the root of a target from the root of
its host.  They share the refusals, the packing of the result and the rendering of FASTA and TSV, nothing else; neither shares anything with
the device's method: no column space, no keys, no directory, no wave, no pointer jumping.
Both take the targets as code arrays."""
import collections

import numpy as np

import merge_checker as MC
import place_checker as P
import scaffold_checker as SC

CONTAINED, MINUS, AMBIGUOUS, DUPLICATE, KEPT = 1, 2, 4, 8, 16
ARRAYS = ("host", "host_pos", "host_orient", "mm", "hits", "state", "root", "root_pos", "root_orient", "absorbed", "new", "old", "len", "col_off", "begin", "words")
COUNTERS = ("queries", "index_positions", "seeds", "seeds_over_max_occ", "candidates", "contained", "contained_minus", "duplicates", "ambiguous", "hits_saturated", "kept",
            "bases_removed", "longest_contained", "columns_before", "columns_after", "n50_before", "n50_after")
DEFAULT = dict(k=21, max_permille=10, max_occ=256)


def check(seqs, k, max_permille, max_occ):
    """the refusals"""
    if not 8 <= k <= 31 or not 0 <= max_permille <= 100 or not 1 <= max_occ <= 65535:
        raise ValueError("parameter out of range")
    if sum(len(s) for s in seqs) > 2 ** 32 - 2 or len(seqs) > 2 ** 30:
        raise OverflowError("more than 2^32 - 2 columns or 2^30 targets")


def check_lengths(tlen):
    """what the device checks of the target arrays: no negative length"""
    if any(int(n) < 0 for n in tlen):
        raise ValueError("negative target length")


def bound(n, max_permille):
    return n * max_permille // 1000


def can_host(seqs, h, c):
    """the order condition of item 3"""
    return h != c and (len(seqs[h]) > len(seqs[c]) or (len(seqs[h]) == len(seqs[c]) and h < c))


def compose(n, inner, len_h, outer):
    """c (n bases) lies in h at inner = (p, s), h (len_h bases) in g at outer = (p', s') -> where c lies in g (item 5)"""
    (p, s), (pp, ss) = inner, outer
    return (pp + p, s) if ss == 0 else (pp + len_h - p - n, s ^ 1)


def _result(seqs, containers, roots, counts):
    """containers: per target the list of (mm, h, p, s); roots: per target (root, pos, orient)"""
    T = len(seqs)
    tlen = [len(s) for s in seqs]
    res = dict(host=np.full(T, -1, np.int32), host_pos=np.zeros(T, np.int32), host_orient=np.zeros(T, np.uint8), mm=np.zeros(T, np.uint32), hits=np.zeros(T, np.uint8),
               state=np.zeros(T, np.uint8), root=np.full(T, -1, np.int32), root_pos=np.zeros(T, np.int32), root_orient=np.zeros(T, np.uint8), absorbed=np.zeros(T, np.uint32),
               new=np.full(T, -1, np.int32))
    old = []
    info = dict(counts, contained=0, contained_minus=0, duplicates=0, ambiguous=0, hits_saturated=0, bases_removed=0, longest_contained=0)
    for c in range(T):
        found = sorted(set(containers[c]))
        assert len(found) == len(containers[c])
        if found:
            mm, h, p, s = found[0]
            dup = tlen[h] == tlen[c]
            res["host"][c], res["host_pos"][c], res["host_orient"][c], res["mm"][c], res["hits"][c] = h, p, s, mm, min(len(found), 255)
            res["state"][c] = CONTAINED | (MINUS if s else 0) | (AMBIGUOUS if len(found) > 1 else 0) | (DUPLICATE if dup else 0)
            info["contained"] += 1
            info["contained_minus"] += s
            info["duplicates"] += dup
            info["ambiguous"] += len(found) > 1
            info["hits_saturated"] += len(found) > 255
            info["bases_removed"] += tlen[c]
            info["longest_contained"] = max(info["longest_contained"], tlen[c])
            res["root"][c], res["root_pos"][c], res["root_orient"][c] = roots[c]
            res["absorbed"][roots[c][0]] += 1
        elif tlen[c]:
            res["state"][c] = KEPT
            res["new"][c] = len(old)
            res["root"][c] = c
            old.append(c)
    kept = [seqs[c] for c in old]
    klen = [len(s) for s in kept]
    res.update(old=np.array(old, np.int32).reshape(len(old)), len=np.array(klen, np.int32).reshape(len(old)),
               col_off=np.concatenate([[0], np.cumsum(klen)]).astype(np.uint32), words=MC.column_words(kept))
    res["begin"] = res["col_off"][:-1].astype(np.uint64)
    info.update(kept=len(old), columns_before=sum(tlen), columns_after=sum(klen), n50_before=SC.n50(tlen), n50_after=SC.n50(klen))
    res["info"] = {k: int(info[k]) for k in COUNTERS}
    return res


def contain_index(seqs, **params):
    pr = dict(DEFAULT, **params)
    k, max_permille, max_occ = pr["k"], pr["max_permille"], pr["max_occ"]
    check(seqs, k, max_permille, max_occ)
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    T = len(seqs)
    index = collections.defaultdict(list)
    for t, s in enumerate(seqs):
        for q, v in enumerate(P.kmer_values(s, k).tolist()):
            index[v].append((t, q))
    counts = dict(queries=0, index_positions=sum(len(v) for v in index.values()), seeds=0, seeds_over_max_occ=0, candidates=0)
    containers = [[] for _ in range(T)]
    for c, fw in enumerate(seqs):
        n = len(fw)
        if n < k:
            continue
        counts["queries"] += 1
        for s, Q in enumerate((fw, P.revcomp(fw))):
            S = min(n // k, 64)
            qv = P.kmer_values(Q, k).tolist()
            diagonals = set()
            for j in range(S):
                where = index.get(qv[j * k], ())
                counts["seeds"] += 1
                if len(where) > max_occ:
                    counts["seeds_over_max_occ"] += 1
                    continue
                for h, q in where:
                    p = q - j * k
                    if can_host(seqs, h, c) and p >= 0 and p + n <= len(seqs[h]):
                        diagonals.add((h, p))
            counts["candidates"] += len(diagonals)
            for h, p in diagonals:
                mm = int(np.count_nonzero(Q != seqs[h][p:p + n]))
                if mm <= bound(n, max_permille):
                    containers[c].append((mm, h, p, s))
    roots = [None] * T
    for c in range(T):                                       # host by host
        if not containers[c]:
            continue
        n, r, at = len(seqs[c]), c, (0, 0)
        while containers[r]:
            _, h, p, s = min(containers[r])
            at = compose(n, at, len(seqs[r]), (p, s))
            r = h
        roots[c] = (r,) + at
    return _result(seqs, containers, roots, counts)


def contain_bruteforce(seqs, **params):
    pr = dict(DEFAULT, **params)
    k, max_permille, max_occ = pr["k"], pr["max_permille"], pr["max_occ"]
    check(seqs, k, max_permille, max_occ)
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    T = len(seqs)
    kv = [P.kmer_values(s, k) for s in seqs]
    every = np.concatenate(kv + [np.zeros(0, np.uint64)])
    counts = dict(queries=sum(1 for s in seqs if len(s) >= k), index_positions=len(every), seeds=0, seeds_over_max_occ=0, candidates=0)
    containers = [[] for _ in range(T)]
    for c, fw in enumerate(seqs):
        n = len(fw)
        if n < k:
            continue
        for s, Q in enumerate((fw, P.revcomp(fw))):
            S = min(n // k, 64)
            seeds = [Q[j * k:(j + 1) * k] for j in range(S)]
            occ = [int(np.count_nonzero(every == P.kmer_values(sd, k)[0])) for sd in seeds]
            counts["seeds"] += S
            counts["seeds_over_max_occ"] += sum(1 for o in occ if o > max_occ)
            for h, H in enumerate(seqs):
                if not can_host(seqs, h, c):
                    continue
                mm = (np.lib.stride_tricks.sliding_window_view(H, n) != Q).sum(axis=1)          # every p with p + n <= len[h]
                seeded = np.zeros(len(mm), bool)                                                # the seed condition, looked at afterwards
                for j in range(S):
                    if 1 <= occ[j] <= max_occ:
                        seeded |= (np.lib.stride_tricks.sliding_window_view(H, k)[j * k:j * k + len(mm)] == seeds[j]).all(axis=1)
                counts["candidates"] += int(seeded.sum())
                for p in np.nonzero(seeded & (mm <= bound(n, max_permille)))[0].tolist():
                    containers[c].append((int(mm[p]), h, p, s))
    roots = [None] * T

    def root_of(c):                                          # from the root of the host
        if roots[c] is None:
            if not containers[c]:
                roots[c] = (c, 0, 0)
            else:
                _, h, p, s = min(containers[c])
                g, pp, ss = root_of(h)
                roots[c] = (g,) + compose(len(seqs[c]), (p, s), len(seqs[h]), (pp, ss))
        return roots[c]

    for c in sorted(range(T), key=lambda c: -len(seqs[c])):  # longest first: the recursion stays shallow
        root_of(c)
    return _result(seqs, containers, roots, counts)


def sequences(res):
    """the kept contigs of a result as code arrays"""
    return [P.codes_of(res["words"], int(res["col_off"][j]), int(res["len"][j])) for j in range(len(res["len"]))]


def fasta(res):
    """the bytes alga_write_kept_fasta_device writes"""
    out = []
    for j, s in enumerate(sequences(res)):
        out.append(">contig_id=%d_length=%d_absorbed=%d\n%s\n" % (j, len(s), int(res["absorbed"][int(res["old"][j])]), "".join("ACGT"[b] for b in s)))
    return "".join(out).encode()


def contain_tsv(res, tlen):
    """the bytes of alga_hip --contain_layout=: one line per input target"""
    sign = lambda o: "-" if o else "+"
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n" % (
        c, int(tlen[c]), int(res["state"][c]), int(res["new"][c]), int(res["host"][c]), int(res["host_pos"][c]), sign(res["host_orient"][c]), int(res["mm"][c]),
        int(res["hits"][c]), int(res["root"][c]), int(res["root_pos"][c]), sign(res["root_orient"][c])) for c in range(len(tlen))).encode()
