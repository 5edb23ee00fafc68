"""The definition of the read placement (include/alga_amd.h: alga_place_reads_device), twice, in Python.

place() finds the candidates through a dictionary of the indexed k-mers (first base most significant; the device: last base first, sorted, behind a
directory); place_bruteforce() walks every (node, target, position) literally and looks at the seeds afterwards.  Neither shares anything with
the device's method: no column space, no keys, placements are collected in a set."""
import collections

import numpy as np

PLACED, UNIQUE, MINUS = 1, 2, 4
DEPTH_MULTI = 1
ARRAYS = ("target", "pos", "mm", "hits", "state", "col_off", "cover", "t_reads", "t_bases", "t_mismatches", "t_uncovered", "insert_hist")
COUNTERS = ("reads", "placed", "unique", "multi", "unplaced", "hits_saturated", "seeds", "seeds_over_max_occ", "index_positions", "index_distinct",
            "pairs", "pairs_proper", "pairs_improper", "pairs_split", "pairs_not_unique", "insert_median", "insert_mean_x100")


def blocks_of(length):
    return 0 if length <= 0 else (2 * length - 1) // 32 + 1


def codes_of(words, begin, length):
    """`length` bases (0 .. 3) of a packed array from base index `begin` on"""
    w = np.asarray(words, dtype=np.uint32).reshape(-1)
    i = np.arange(length, dtype=np.int64) + int(begin)
    return ((w[i >> 4] >> ((i & 15) << 1).astype(np.uint32)) & 3).astype(np.uint8)


def pack(codes, stride):
    out = np.zeros(stride, dtype=np.uint32)
    c = np.asarray(codes, dtype=np.uint32)
    i = np.arange(len(c))
    np.bitwise_or.at(out, i >> 4, c << ((i & 15) << 1).astype(np.uint32))
    return out


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def nodes_of(reads, stride=None):
    """forward reads (code arrays; None = a removed read, len -1) -> rows, lens in twin layout: node 2r = reverse complement, 2r + 1 = read r"""
    need = max([blocks_of(len(r)) for r in reads if r is not None] + [1])
    stride = need if stride is None else stride
    rows = np.zeros((2 * len(reads), stride), dtype=np.uint32)
    lens = np.full(2 * len(reads), -1, dtype=np.int32)
    for r, c in enumerate(reads):
        if c is None:
            continue
        lens[2 * r] = lens[2 * r + 1] = len(c)
        rows[2 * r + 1] = pack(c, stride)
        rows[2 * r] = pack(revcomp(c), stride)
    return rows, lens


def ragged(seqs, shifts, gaps=None):
    """sequences laid out in one packed array, sequence i beginning at a base with begin & 15 == shifts[i] (gaps[i] = False: directly behind the
    sequence before it) -> words u32, begin i64, len i32"""
    begin, at = [], 0
    for i, s in enumerate(seqs):
        if gaps is None or gaps[i]:
            at = (at + 15) // 16 * 16 + 16 + int(shifts[i])
        begin.append(at)
        at += len(s)
    words = np.zeros((at + 15) // 16 + 2, dtype=np.uint32)
    for b, s in zip(begin, seqs):
        c = np.asarray(s, dtype=np.uint32)
        i = np.arange(len(c), dtype=np.int64) + b
        np.bitwise_or.at(words, i >> 4, c << ((i & 15) << 1).astype(np.uint32))
    return words, np.array(begin, dtype=np.int64), np.array([len(s) for s in seqs], dtype=np.int32)


def kmer_values(codes, k):
    c = np.asarray(codes, dtype=np.uint64)
    if len(c) < k:
        return np.zeros(0, dtype=np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(c, k)
    return (win * (np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def check(rows, lens, pair_off, tlen, k, max_mismatches, max_occ, max_insert, flags):
    if not 8 <= k <= 31 or not 0 <= max_mismatches <= 254 or not 1 <= max_occ <= 65535 or not 1 <= max_insert <= 1 << 20 or flags & ~DEPTH_MULTI:
        raise ValueError("parameter out of range")
    n = len(lens)
    if n % 2:
        raise ValueError("n must be even")
    if (np.asarray(tlen) < 0).any():
        raise ValueError("negative target length")
    if int(np.asarray(tlen, dtype=np.int64).sum()) > 2 ** 32 - 2:
        raise OverflowError("more than 2^32 - 2 columns")
    stride = rows.shape[1] if n else 0
    for r in range(n // 2):
        if lens[2 * r] != lens[2 * r + 1] or blocks_of(int(lens[2 * r])) > stride:
            raise ValueError("twin lengths")
        if lens[2 * r] > 0:
            L = int(lens[2 * r])
            if (pack(revcomp(codes_of(rows[2 * r + 1], 0, L)), stride)[:blocks_of(L)] != rows[2 * r][:blocks_of(L)]).any():
                raise ValueError("row 2r is not the reverse complement of row 2r + 1")
    if pair_off is not None:
        po = np.asarray(pair_off)
        for v in range(n):
            if po[v] > 2 or po[v] != po[v ^ 1] or (po[v] == 1 and (v + 2 >= n or po[v + 2] != 2)) or (po[v] == 2 and (v < 2 or po[v - 2] != 1)):
                raise ValueError("pair_off")


def _finish(placements, rows, lens, pair_off, targets, k, max_occ, max_insert, flags, occ):
    """steps 4 - 7 from the placement sets: placements[r] = set of (mm, t, p, strand)"""
    R, T = len(lens) // 2, len(targets)
    tlen = np.array([len(t) for t in targets], dtype=np.int64)
    col_off = np.concatenate([[0], np.cumsum(tlen)]).astype(np.uint32)
    out = dict(target=np.full(R, -1, np.int32), pos=np.full(R, -1, np.int32), mm=np.zeros(R, np.uint8), hits=np.zeros(R, np.uint8), state=np.zeros(R, np.uint8),
               col_off=col_off, cover=np.zeros(int(tlen.sum()), np.uint32), t_reads=np.zeros(T, np.uint64), t_bases=np.zeros(T, np.uint64),
               t_mismatches=np.zeros(T, np.uint64), t_uncovered=np.zeros(T, np.uint64), insert_hist=np.zeros(max_insert + 1, np.uint64))
    info = dict.fromkeys(COUNTERS, 0)
    info["reads"] = R
    for r in range(R):
        L = int(lens[2 * r + 1])
        if L >= k:
            for v in (2 * r + 1, 2 * r):
                vals = kmer_values(codes_of(rows[v], 0, L), k)[::k]
                info["seeds"] += len(vals)
                info["seeds_over_max_occ"] += sum(occ.get(int(x), 0) > max_occ for x in vals)
        if not placements[r]:
            continue
        best = min(placements[r])
        hits = sum(1 for x in placements[r] if x[0] == best[0])
        info["hits_saturated"] += hits > 255
        out["target"][r], out["pos"][r], out["mm"][r], out["hits"][r] = best[1], best[2], best[0], min(hits, 255)
        out["state"][r] = PLACED | (UNIQUE if hits == 1 else 0) | (MINUS if best[3] else 0)
        info["placed"] += 1
        info["unique"] += hits == 1
        if out["state"][r] & (PLACED if flags & DEPTH_MULTI else UNIQUE):
            t, p = best[1], best[2]
            out["cover"][int(col_off[t]) + p:int(col_off[t]) + p + L] += 1
            out["t_reads"][t] += 1
            out["t_bases"][t] += L
            out["t_mismatches"][t] += best[0]
    info["multi"] = info["placed"] - info["unique"]
    info["unplaced"] = R - info["placed"]
    for t in range(T):
        out["t_uncovered"][t] = int((out["cover"][int(col_off[t]):int(col_off[t + 1])] == 0).sum())
    info["index_positions"] = sum(occ.values())
    info["index_distinct"] = len(occ)
    total = 0
    if pair_off is not None:
        for r in range(R):
            if pair_off[2 * r + 1] != 1:
                continue
            r2 = r + 1
            info["pairs"] += 1
            s1, s2 = int(out["state"][r]), int(out["state"][r2])
            if not (s1 & UNIQUE and s2 & UNIQUE):
                info["pairs_not_unique"] += 1
            elif out["target"][r] != out["target"][r2]:
                info["pairs_split"] += 1
            else:
                proper = False
                if (s1 & MINUS) != (s2 & MINUS):
                    rp, rm = (r2, r) if s1 & MINUS else (r, r2)
                    a, la, b, lb = int(out["pos"][rp]), int(lens[2 * rp + 1]), int(out["pos"][rm]), int(lens[2 * rm + 1])
                    ins = b + lb - a
                    proper = a <= b and a + la <= b + lb and ins <= max_insert
                if proper:
                    info["pairs_proper"] += 1
                    out["insert_hist"][ins] += 1
                    total += ins
                else:
                    info["pairs_improper"] += 1
    info["insert_median"] = info["insert_mean_x100"] = -1
    if info["pairs_proper"]:
        cum = np.cumsum(out["insert_hist"].astype(np.int64))
        info["insert_median"] = int(np.nonzero(cum >= (info["pairs_proper"] + 1) // 2)[0][0])
        info["insert_mean_x100"] = 100 * total // info["pairs_proper"]
    out["info"] = {k_: int(v) for k_, v in info.items()}
    return out


def _targets(twords, tbegin, tlen):
    return [codes_of(twords, tbegin[t], int(tlen[t])) for t in range(len(tlen))]


def _index(targets, k):
    index = collections.defaultdict(list)
    for t, c in enumerate(targets):
        for q, x in enumerate(kmer_values(c, k)):
            index[int(x)].append((t, q))
    return index


def place(rows, lens, pair_off, twords, tbegin, tlen, k=21, max_mismatches=4, max_occ=256, max_insert=1000, flags=0):
    """the definition with a dictionary index: the candidates are the occurrences of the usable seeds"""
    check(rows, lens, pair_off, tlen, k, max_mismatches, max_occ, max_insert, flags)
    targets = _targets(twords, tbegin, tlen)
    index = _index(targets, k)
    occ = {x: len(v) for x, v in index.items()}
    placements = []
    for r in range(len(lens) // 2):
        found = set()
        L = int(lens[2 * r + 1])
        if L >= k:
            for strand, v in ((0, 2 * r + 1), (1, 2 * r)):
                c = codes_of(rows[v], 0, L)
                for j, x in enumerate(kmer_values(c, k)[::k]):
                    hits = index.get(int(x), ())
                    if not 1 <= len(hits) <= max_occ:
                        continue
                    for t, q in hits:
                        p = q - j * k
                        if p < 0 or p + L > len(targets[t]):
                            continue
                        mm = int((targets[t][p:p + L] != c).sum())
                        if mm <= max_mismatches:
                            found.add((mm, t, p, strand))
        placements.append(found)
    return _finish(placements, rows, lens, pair_off, targets, k, max_occ, max_insert, flags, occ)


def place_bruteforce(rows, lens, pair_off, twords, tbegin, tlen, k=21, max_mismatches=4, max_occ=256, max_insert=1000, flags=0):
    """the definition walked literally: every (node, t, p), the Hamming distance first, then whether a usable seed matches there"""
    check(rows, lens, pair_off, tlen, k, max_mismatches, max_occ, max_insert, flags)
    targets = _targets(twords, tbegin, tlen)
    occ = collections.Counter()
    for c in targets:
        occ.update(int(x) for x in kmer_values(c, k))
    occ = dict(occ)
    placements = []
    for r in range(len(lens) // 2):
        found = set()
        L = int(lens[2 * r + 1])
        if L >= k:
            for strand, v in ((0, 2 * r + 1), (1, 2 * r)):
                c = codes_of(rows[v], 0, L)
                usable = [1 <= occ.get(int(x), 0) <= max_occ for x in kmer_values(c, k)[::k]]
                for t, tc in enumerate(targets):
                    if len(tc) < L:
                        continue
                    every = np.lib.stride_tricks.sliding_window_view(tc, L) != c          # row p: t[p .. p + L) against the node
                    for p in np.nonzero(every.sum(axis=1) <= max_mismatches)[0]:
                        diff = every[p]
                        if any(u and not diff[j * k:j * k + k].any() for j, u in enumerate(usable)):
                            found.add((int(diff.sum()), t, int(p), strand))
        placements.append(found)
    return _finish(placements, rows, lens, pair_off, targets, k, max_occ, max_insert, flags, occ)


def depth_header(j, length, t_reads, t_bases):
    v = 100 * int(t_bases) // int(length)
    return ">contig_id=%d_length=%d_reads=%d_depth=%d.%02d" % (j, length, int(t_reads), v // 100, v % 100)
