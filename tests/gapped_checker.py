"""The definition of the gapped placement (include/alga_amd.h: alga_place_gapped_device), twice, in Python.

gapped_full() finds the candidates by comparing every seed with every target position, counts the occurrences the same way, and fills the plain
full edit-distance table of both parts of every candidate.  gapped_banded() goes another way: a dictionary of the indexed k-mers, tables banded
to |c - i| <= E and anchored at the seed, stored by diagonal.  Each traces its own tables.  Neither shares anything with the device's method: no
column space, no keys, no halves of a wave.  `pl` is a placement as tests/place_checker.py returns it (state, cover, col_off are read)."""
import numpy as np

import place_checker as P

PLACED, UNIQUE, MINUS, INDEL = 1, 2, 4, 8
OP_M, OP_I, OP_D = 0, 1, 2
MAX_READ = 1024
DEFAULT = dict(k=21, max_edits=6, max_occ=256)
ARRAYS = ("target", "pos", "end", "edits", "state", "cigar_off", "cigar", "cover", "t_reads", "t_bases", "t_edits")
COUNTERS = ("tried", "skipped_long", "placed", "unique", "with_indel", "edits", "insertions", "deletions", "candidates", "seeds", "seeds_over_max_occ")
INF = 1 << 20


def check(rows, lens, pl, tlen, k, max_edits, max_occ, flags=0):
    if not 8 <= k <= 31 or not 1 <= max_edits <= 15 or not 1 <= max_occ <= 65535 or flags:
        raise ValueError("parameter out of range")
    P.check(rows, lens, None, tlen, k, 0, max_occ, 1, 0)
    if len(pl["state"]) != len(lens) // 2:
        raise ValueError("the placement has other reads")
    off = np.concatenate([[0], np.cumsum(np.asarray(tlen, dtype=np.int64))])
    if len(pl["col_off"]) != len(off) or (pl["col_off"].astype(np.int64) != off).any() or len(pl["cover"]) != int(off[-1]):
        raise ValueError("the placement has other targets")


def takes_part(pl, lens, r, k):
    L = int(lens[2 * r + 1])
    return not (int(pl["state"][r]) & P.PLACED) and k <= L <= MAX_READ


# ---- the plain statement ----------------------------------------------------------------------------------------------------------------
def full_table(a, b):
    """D[i][c], 0 <= i <= len(a), 0 <= c <= len(b): the edit distance of a[:i] and b[:c]"""
    n, m = len(a), len(b)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    D[0] = np.arange(m + 1)
    ar = np.arange(m + 1)
    for i in range(1, n + 1):
        x = np.empty(m + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(D[i - 1][:-1] + (b != a[i - 1]), D[i - 1][1:] + 1)
        D[i] = np.minimum.accumulate(x - ar) + ar                 # ... and from the left neighbour
    return D


def end_of(row_n, n, avail, E):
    """(value, c) of the end cell among c in [max(0, n - E), min(avail, n + E)], or None; row_n(c) = D[n][c]"""
    best = None
    for c in range(max(0, n - E), min(avail, n + E) + 1):
        key = (int(row_n(c)), abs(c - n), c)
        if best is None or key < best:
            best = key
    return None if best is None else (best[0], best[2])


def trace(get, a, b, n, c):
    """ops from the end cell (n, c) back to (0, 0): the first of diagonal, up, left whose predecessor attains the value"""
    ops, i = [], n
    while i > 0 or c > 0:
        v = get(i, c)
        if i > 0 and c > 0 and get(i - 1, c - 1) + (a[i - 1] != b[c - 1]) == v:
            ops.append(OP_M); i -= 1; c -= 1
        elif i > 0 and get(i - 1, c) + 1 == v:
            ops.append(OP_I); i -= 1
        else:
            assert c > 0 and get(i, c - 1) + 1 == v
            ops.append(OP_D); c -= 1
    return ops


def part_full(a, b_all, E):
    """a part by the full table: (d, c_end, ops as traced) or None"""
    n = len(a)
    b = b_all[:min(len(b_all), n + E)]                             # later columns change no cell before them
    D = full_table(a, b)
    end = end_of(lambda c: D[n][c], n, len(b_all), E)
    if end is None or end[0] > E:
        return None
    return end[0], end[1], trace(lambda i, c: int(D[i][c]), a, b, n, end[1])


# ---- the other route: banded by diagonal ------------------------------------------------------------------------------------------------
def banded_table(a, b, E):
    """B[i][h] = D[i][i + h - E] inside the band |c - i| <= E (INF outside the table); values <= E are exact"""
    n, m, W = len(a), len(b), 2 * E + 1
    B = np.full((n + 1, W), INF, dtype=np.int64)
    hh = np.arange(W)
    B[0] = np.where((hh - E >= 0) & (hh - E <= m), hh - E, INF)
    bb = np.concatenate([np.asarray(b, dtype=np.int64), [-1]])    # (b[-1]: a cell that is not there)
    for i in range(1, n + 1):
        c = i + hh - E
        valid = (c >= 0) & (c <= m)
        diag = np.where(valid & (c >= 1), B[i - 1] + (bb[np.clip(c - 1, -1, m - 1)] != a[i - 1]), INF)
        up = np.concatenate([B[i - 1][1:], [INF]]) + 1
        x = np.where(valid, np.minimum(diag, up), INF)
        row = np.minimum.accumulate(x - hh) + hh                     # ... and from the diagonal below, the left neighbour
        B[i] = np.where(valid, np.minimum(row, INF), INF)
    return B


def part_banded(a, b_all, E):
    n = len(a)
    b = b_all[:min(len(b_all), n + E)]
    B = banded_table(a, b, E)

    def get(i, c):
        h = c - i + E
        return int(B[i][h]) if 0 <= h <= 2 * E and 0 <= c <= len(b) else INF
    end = end_of(lambda c: get(n, c), n, len(b_all), E)
    if end is None or end[0] > E:
        return None
    return end[0], end[1], trace(get, a, b, n, end[1])


def banded_equals_full(a, b_all, E):
    """what rule 5 claims, on one part: inside the band a value <= E is the full table's and a value > E says the full one is > E; every cell
    the trace visits is <= E; both tables give the same end and the same script"""
    n = len(a)
    b = b_all[:min(len(b_all), n + E)]
    D, B = full_table(a, b), banded_table(a, b, E)
    for i in range(n + 1):
        for h in range(2 * E + 1):
            c = i + h - E
            if 0 <= c <= len(b):
                assert (B[i][h] == D[i][c]) if (B[i][h] <= E or D[i][c] <= E) else (B[i][h] > E and D[i][c] > E), (i, c)
    pf, pb = part_full(a, b_all, E), part_banded(a, b_all, E)
    assert pf == pb
    if pf is not None:
        i, c = n, pf[1]
        assert D[i][c] <= E
        for op in pf[2]:
            i, c = i - (op != OP_D), c - (op != OP_I)
            assert D[i][c] <= E and abs(c - i) <= E
    return pf


def runs_of(ops):
    out = []
    for op in ops:
        if out and out[-1][1] == op:
            out[-1][0] += 1
        else:
            out.append([1, op])
    return [(n, op) for n, op in out]


def _finish(found, lens, pl, targets, E, info):
    """rules 6 - 8 from the candidates that are placements: found[r] = list of (d, strand, t, p, e, j, q, ops)"""
    R, T = len(lens) // 2, len(targets)
    col_off = pl["col_off"].astype(np.int64)
    out = dict(target=np.full(R, -1, np.int32), pos=np.full(R, -1, np.int32), end=np.full(R, -1, np.int32), edits=np.zeros(R, np.uint8), state=np.zeros(R, np.uint8),
               cover=pl["cover"].copy(), t_reads=np.zeros(T, np.uint64), t_bases=np.zeros(T, np.uint64), t_edits=np.zeros(T, np.uint64))
    cigar, cigar_off = [], [0]
    for r in range(R):
        if found[r]:
            best = min(found[r], key=lambda x: x[:7])
            d, strand, t, p, e = best[:5]
            unique = all(x[1] == strand and x[2] == t and x[3] <= p + E for x in found[r] if x[0] == d)
            runs = runs_of(best[7])
            assert len(runs) <= 2 * E + 1
            ins, dele = sum(n for n, op in runs if op == OP_I), sum(n for n, op in runs if op == OP_D)
            assert sum(n for n, op in runs if op != OP_D) == int(lens[2 * r + 1]) and sum(n for n, op in runs if op != OP_I) == e - p and ins + dele <= d
            out["target"][r], out["pos"][r], out["end"][r], out["edits"][r] = t, p, e, d
            out["state"][r] = PLACED | (UNIQUE if unique else 0) | (MINUS if strand else 0) | (INDEL if ins + dele else 0)
            cigar += [(n << 2) | op for n, op in runs]
            info["placed"] += 1
            info["unique"] += unique
            info["with_indel"] += (ins + dele) > 0
            info["edits"] += d
            info["insertions"] += ins
            info["deletions"] += dele
            if unique:
                out["cover"][int(col_off[t]) + p:int(col_off[t]) + e] += 1
                out["t_reads"][t] += 1
                out["t_bases"][t] += e - p
                out["t_edits"][t] += d
        cigar_off.append(len(cigar))
    out["cigar_off"], out["cigar"] = np.array(cigar_off, dtype=np.uint32), np.array(cigar, dtype=np.uint32)
    out["info"] = {k_: int(v) for k_, v in info.items()}
    out["found"] = [[x[:7] for x in f] for f in found]                 # every placement found, (d, strand, t, p, e, j, q): no result, for the tests' own questions
    return out


def _place_candidate(c, tc, j, q, k, E, part):
    """rules 4 and 5 for candidate (j, q) of node codes c on target codes tc: (d, p, e, ops) or None"""
    right = part(c[j * k + k:], tc[q + k:], E)
    if right is None:
        return None
    left = part(c[:j * k][::-1], tc[:q][::-1], E)
    if left is None or left[0] + right[0] > E:
        return None
    return left[0] + right[0], q - left[1], q + k + right[1], left[2] + [OP_M] * k + right[2][::-1]


def gapped_full(rows, lens, pl, twords, tbegin, tlen, k=21, max_edits=6, max_occ=256, flags=0):
    """the definition walked literally: every seed against every target position, the full tables"""
    check(rows, lens, pl, tlen, k, max_edits, max_occ, flags)
    E = max_edits
    targets = P._targets(twords, tbegin, tlen)
    tk = [P.kmer_values(c, k) for c in targets]
    info = dict.fromkeys(COUNTERS, 0)
    found = []
    for r in range(len(lens) // 2):
        got = []
        L = int(lens[2 * r + 1])
        if not (int(pl["state"][r]) & P.PLACED) and L > MAX_READ:
            info["skipped_long"] += 1
        if takes_part(pl, lens, r, k):
            info["tried"] += 1
            for strand, v in ((0, 2 * r + 1), (1, 2 * r)):
                c = P.codes_of(rows[v], 0, L)
                seeds = P.kmer_values(c, k)[::k][:L // k]
                hits = [[(t, int(q)) for t in range(len(targets)) for q in np.nonzero(tk[t] == x)[0]] for x in seeds]
                usable = [1 <= len(h) <= max_occ for h in hits]
                info["seeds"] += len(seeds)
                info["seeds_over_max_occ"] += sum(len(h) > max_occ for h in hits)
                for j in range(len(seeds)):
                    if not usable[j]:
                        continue
                    for t, q in hits[j]:
                        tc = targets[t]
                        if any(usable[j2] and q - (j - j2) * k >= 0 and (tc[q - (j - j2) * k:q - (j - j2) * k + k] == c[j2 * k:j2 * k + k]).all() for j2 in range(j)):
                            continue
                        info["candidates"] += 1
                        res = _place_candidate(c, tc, j, q, k, E, part_full)
                        if res is not None:
                            got.append((res[0], strand, t, res[1], res[2], j, q, res[3]))
        found.append(got)
    return _finish(found, lens, pl, targets, E, info)


def gapped_banded(rows, lens, pl, twords, tbegin, tlen, k=21, max_edits=6, max_occ=256, flags=0):
    """the definition with a dictionary index and tables banded to +-E, anchored at the seed; a read seen before (same bases) is not aligned again"""
    check(rows, lens, pl, tlen, k, max_edits, max_occ, flags)
    E = max_edits
    targets = P._targets(twords, tbegin, tlen)
    index = P._index(targets, k)
    info = dict.fromkeys(COUNTERS, 0)
    found, seen = [], {}
    for r in range(len(lens) // 2):
        got = []
        L = int(lens[2 * r + 1])
        if not (int(pl["state"][r]) & P.PLACED) and L > MAX_READ:
            info["skipped_long"] += 1
        if takes_part(pl, lens, r, k):
            fwd = P.codes_of(rows[2 * r + 1], 0, L)
            memo = seen.get(fwd.tobytes())
            if memo is None:
                memo = [[], 0, 0, 0]                                # placements, seeds, over, candidates
                for strand, c in ((0, fwd), (1, P.codes_of(rows[2 * r], 0, L))):
                    vals = [int(x) for x in P.kmer_values(c, k)[::k][:L // k]]
                    memo[1] += len(vals)
                    memo[2] += sum(len(index.get(x, ())) > max_occ for x in vals)
                    usable = [1 <= len(index.get(x, ())) <= max_occ for x in vals]
                    for j, x in enumerate(vals):
                        if not usable[j]:
                            continue
                        for t, q in index[x]:
                            if any(usable[j2] and (t, q - (j - j2) * k) in index.get(vals[j2], ()) for j2 in range(j)):
                                continue
                            memo[3] += 1
                            res = _place_candidate(c, targets[t], j, q, k, E, part_banded)
                            if res is not None:
                                memo[0].append((res[0], strand, t, res[1], res[2], j, q, res[3]))
                seen[fwd.tobytes()] = memo
            got = memo[0]
            info["tried"] += 1
            info["seeds"] += memo[1]
            info["seeds_over_max_occ"] += memo[2]
            info["candidates"] += memo[3]
        found.append(got)
    return _finish(found, lens, pl, targets, E, info)


def cigar_strings(w):
    """the CIGAR of every read as text ('' where it is not placed)"""
    off = w["cigar_off"]
    return ["".join("%d%s" % (int(x) >> 2, "MID"[int(x) & 3]) for x in w["cigar"][int(off[r]):int(off[r + 1])]) for r in range(len(off) - 1)]


def tsv(w):
    """one line per gapped-placed read: read, target, pos, end, strand, edits, unique, cigar (tabs)"""
    cg = cigar_strings(w)
    return "".join("%d\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (r, int(w["target"][r]), int(w["pos"][r]), int(w["end"][r]), "-" if w["state"][r] & MINUS else "+",
                                                       int(w["edits"][r]), 1 if w["state"][r] & UNIQUE else 0, cg[r])
                   for r in range(len(cg)) if w["state"][r] & PLACED).encode()
