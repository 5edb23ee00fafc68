"""The definition of the polish (include/alga_amd.h: alga_polish_placed_device), twice, in Python.

polish_scatter() walks the reads: every voter adds its bases to the counts of the columns it covers, then all columns are decided at once.
polish_gather() walks the columns: for every column it asks every voter whether it covers the column, counts, and decides that column alone.
Neither shares anything with the device's method: no sort, no bit-sliced counters, no words -- the packed output is made at the very end.
Both take a placement as tests/place_checker.py returns it (target, pos, state, col_off) and the targets that were placed on."""
import numpy as np

import place_checker as P

MULTI, COUNTS = 1, 2
ARRAYS = ("col_off", "words", "changed_cols", "changed_bases", "t_changed", "t_ambiguous")
COUNTERS = ("columns", "voters", "votes", "voted_columns", "changed", "ambiguous", "max_cover")


def check(rows, lens, pl, min_cover, min_percent, flags):
    """the refusals -> the voters as (read, node, first column, length)"""
    if not 1 <= min_cover <= 2 ** 31 - 1 or not 1 <= min_percent <= 100 or flags & ~(MULTI | COUNTS):
        raise ValueError("parameter out of range")
    n = len(lens)
    if n % 2 or n // 2 != len(pl["state"]):
        raise ValueError("not the node set that was placed")
    col_off = pl["col_off"].astype(np.int64)
    stride = rows.shape[1] if n else 0
    bit = P.PLACED if flags & MULTI else P.UNIQUE
    voters = []
    for r in range(n // 2):
        st = int(pl["state"][r])
        if not st & bit:
            continue
        v = 2 * r if st & P.MINUS else 2 * r + 1
        L, t, p = int(lens[v]), int(pl["target"][r]), int(pl["pos"][r])
        if L < 1 or L > 16 * stride:
            raise ValueError("voter length")
        if not 0 <= t < len(col_off) - 1 or p < 0 or p + L > col_off[t + 1] - col_off[t]:
            raise ValueError("a voter leaves its target")
        voters.append((r, v, int(col_off[t]) + p, L))
    return voters


def _cur(pl, twords, tbegin, tlen):
    parts = [P.codes_of(twords, tbegin[t], int(tlen[t])) for t in range(len(tlen))]
    cur = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    assert len(cur) == int(pl["col_off"][-1])
    return cur.astype(np.uint8)


def _result(pl, cur, count, seq, changed, ambiguous, voters, min_cover):
    n = len(cur)
    col_off = pl["col_off"].astype(np.int64)
    T = len(col_off) - 1
    words = np.zeros((n + 15) // 16 + 2, dtype=np.uint32)
    g = np.arange(n, dtype=np.int64)
    np.bitwise_or.at(words, g >> 4, seq.astype(np.uint32) << ((g & 15) << 1).astype(np.uint32))
    cols = np.nonzero(changed)[0]
    tc, ta = np.zeros(T, np.uint64), np.zeros(T, np.uint64)
    for t in range(T):
        tc[t] = int(changed[col_off[t]:col_off[t + 1]].sum())
        ta[t] = int(ambiguous[col_off[t]:col_off[t + 1]].sum())
    cover = count.sum(axis=1, dtype=np.int64)
    info = dict(columns=n, voters=len(voters), votes=sum(v[3] for v in voters), voted_columns=int((cover >= min_cover).sum()), changed=int(changed.sum()),
                ambiguous=int(ambiguous.sum()), max_cover=int(cover.max()) if n else 0)
    return dict(col_off=pl["col_off"].astype(np.uint32), words=words, changed_cols=cols.astype(np.uint32),
                changed_bases=(cur[cols] | (seq[cols] << 2)).astype(np.uint8), t_changed=tc, t_ambiguous=ta, counts=count.astype(np.uint32),
                cover=cover.astype(np.uint32), seq=seq.astype(np.uint8), ambiguous_cols=np.nonzero(ambiguous)[0].astype(np.uint32), info=info)


def polish_scatter(rows, lens, pl, twords, tbegin, tlen, min_cover=3, min_percent=60, flags=0):
    """per read: its bases into the counts; then every column at once"""
    voters = check(rows, lens, pl, min_cover, min_percent, flags)
    cur = _cur(pl, twords, tbegin, tlen)
    n = len(cur)
    count = np.zeros((n, 4), dtype=np.int64)
    for _, v, g0, L in voters:
        np.add.at(count, (np.arange(g0, g0 + L), P.codes_of(rows[v], 0, L)), 1)
    cover = count.sum(axis=1)
    top = count.max(axis=1) if n else np.zeros(0, np.int64)
    at = np.arange(n)
    w = np.where(count[at, cur] == top, cur, count.argmax(axis=1) if n else cur).astype(np.uint8)      # argmax: the smallest code among the tied
    differs = (w != cur) & (cover >= min_cover)
    enough = 100 * top >= min_percent * cover
    changed, ambiguous = differs & enough, differs & ~enough
    return _result(pl, cur, count, np.where(changed, w, cur).astype(np.uint8), changed, ambiguous, voters, min_cover)


def polish_gather(rows, lens, pl, twords, tbegin, tlen, min_cover=3, min_percent=60, flags=0):
    """per column: every voter is asked whether it covers it"""
    voters = check(rows, lens, pl, min_cover, min_percent, flags)
    cur = _cur(pl, twords, tbegin, tlen)
    n = len(cur)
    longest = max([v[3] for v in voters] + [1])
    codes = np.full((len(voters), longest), 255, dtype=np.uint8)
    for i, (_, v, _, L) in enumerate(voters):
        codes[i, :L] = P.codes_of(rows[v], 0, L)
    start = np.array([v[2] for v in voters], dtype=np.int64)
    end = start + np.array([v[3] for v in voters], dtype=np.int64)
    count = np.zeros((n, 4), dtype=np.int64)
    seq = cur.copy()
    changed, ambiguous = np.zeros(n, bool), np.zeros(n, bool)
    for g in range(n):
        over = np.nonzero((start <= g) & (g < end))[0]
        c = [int((codes[over, g - start[over]] == b).sum()) for b in range(4)]
        count[g] = c
        cover, c0 = sum(c), int(cur[g])
        tied = [b for b in range(4) if c[b] == max(c)]
        w = c0 if c0 in tied else tied[0]
        if w != c0 and cover >= min_cover:
            if 100 * c[w] >= min_percent * cover:
                changed[g], seq[g] = True, w
            else:
                ambiguous[g] = True
    return _result(pl, cur, count, seq, changed, ambiguous, voters, min_cover)


def sequences(res):
    """the polished targets as code arrays"""
    off = res["col_off"].astype(np.int64)
    return [P.codes_of(res["words"], off[t], int(off[t + 1] - off[t])) for t in range(len(off) - 1)]


def targets_of(res):
    """(words, begin, len) of the polished targets: the ragged form the placement takes"""
    off = res["col_off"].astype(np.int64)
    return res["words"], off[:-1].copy(), (off[1:] - off[:-1]).astype(np.int32)
