"""The definition of the polish with the gapped reads (include/alga_amd.h: alga_polish_indels_device), twice, in Python.

ipolish_scatter() walks the voters: a G voter's script is normalised as a LIST OF RUNS (the M run in front of a gap shrinks, a run of M cells is
put behind it), then every cell adds its vote where it falls, and all columns and slots are decided at once.  ipolish_gather() walks the columns
and the slots: a G voter is a list of GAP EVENTS (kind, column, read offset, length), each moved one base at a time; for every column it asks
every voter what it holds there (a base, found by counting the gaps in front of the column, or a deleted cell), for every slot which voters span
it and which insert there, and decides that column and that slot alone.  Neither uses a sort or bit tricks; they share only the refusals
(check) and the rendering of the decisions into the result's arrays and texts (_render).  `pl` / `gp` are a placement and a gapped placement as
tests/place_checker.py and tests/gapped_checker.py return them."""
import numpy as np

import gapped_checker as GC
import place_checker as P

COUNTS = 1
MAX_INS = 13
OP_M, OP_I, OP_D = 0, 1, 2
EV_S, EV_I, EV_D = 0, 1, 2
DEFAULT = dict(min_cover=3, min_percent=60, max_ins=6)
ARRAYS = ("len", "col_off", "begin", "words", "new_col", "ev_col", "ev_kind", "ev_len", "ev_bases", "ev_votes", "ev_cover", "t_subs", "t_dels", "t_ins_bases", "t_ambiguous")
COUNTERS = ("columns", "voters_hamming", "voters_gapped", "votes", "del_votes", "ins_votes", "ins_too_long", "ins_edge", "shifted_runs", "shifted_bases", "voted_columns",
            "substituted", "deleted", "inserted_slots", "inserted_bases", "ambiguous_columns", "ambiguous_slots", "columns_after", "max_cover")


# ---- shared: the refusals --------------------------------------------------------------------------------------------------------------------
def check(rows, lens, pl, gp, min_cover, min_percent, max_ins, flags, reserved=0):
    """the refusals -> the voters as (kind 'H' | 'G', node, first column, end column, script [(op, n)])"""
    if not 1 <= min_cover <= 2 ** 31 - 1 or not 1 <= min_percent <= 100 or not 1 <= max_ins <= MAX_INS or flags & ~COUNTS or reserved:
        raise ValueError("parameter out of range")
    n = len(lens)
    if n % 2 or n // 2 != len(pl["state"]) or n // 2 != len(gp["state"]):
        raise ValueError("not the node set that was placed")
    if len(gp["cover"]) != int(pl["col_off"][-1]) or len(gp["t_reads"]) != len(pl["col_off"]) - 1:
        raise ValueError("the gapped result was made from another placement")
    P.check(rows, lens, None, np.zeros(0, np.int32), 8, 0, 1, 1, 0)                       # the twin property
    col_off = pl["col_off"].astype(np.int64)
    T = len(col_off) - 1
    stride = rows.shape[1] if n else 0
    voters = []
    for r in range(n // 2):
        st, sg = int(pl["state"][r]), int(gp["state"][r])
        if st & P.UNIQUE:
            v = 2 * r if st & P.MINUS else 2 * r + 1
            L, t, p = int(lens[v]), int(pl["target"][r]), int(pl["pos"][r])
            if L < 1 or L > 16 * stride:
                raise ValueError("voter length")
            if not 0 <= t < T or p < 0 or p + L > col_off[t + 1] - col_off[t]:
                raise ValueError("a voter leaves its target")
            voters.append(("H", v, int(col_off[t]) + p, int(col_off[t]) + p + L, [(OP_M, L)]))
        elif sg & GC.UNIQUE:
            v = 2 * r if sg & GC.MINUS else 2 * r + 1
            L, t, p, e = int(lens[v]), int(gp["target"][r]), int(gp["pos"][r]), int(gp["end"][r])
            script = [(int(x) & 3, int(x) >> 2) for x in gp["cigar"][int(gp["cigar_off"][r]):int(gp["cigar_off"][r + 1])]]
            if not 1 <= len(script) <= 31 or any(op == 3 for op, _ in script):
                raise ValueError("a gapped voter's runs")
            if not 0 <= t < T or p < 0 or e <= p or e > col_off[t + 1] - col_off[t]:
                raise ValueError("a gapped voter leaves its target")
            if L < 1 or L > 16 * stride or sum(k for op, k in script if op != OP_D) != L:
                raise ValueError("a gapped voter's read length")
            if sum(k for op, k in script if op != OP_I) != e - p:
                raise ValueError("a gapped voter's column length")
            voters.append(("G", v, int(col_off[t]) + p, int(col_off[t]) + e, script))
    return voters


def _cur(pl, twords, tbegin, tlen):
    parts = [P.codes_of(twords, tbegin[t], int(tlen[t])) for t in range(len(tlen))]
    cur = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    assert len(cur) == int(pl["col_off"][-1])
    return cur.astype(np.uint8)


def key_of(bases):
    """(n, string) as n << 26 | string, the first base in the highest used bits"""
    s = 0
    for b in bases:
        s = (s << 2) | int(b)
    return (len(bases) << 26) | s


def bases_of(key):
    n = key >> 26
    return [(key >> (2 * (n - 1 - i))) & 3 for i in range(n)]


# ---- shared: the rendering -------------------------------------------------------------------------------------------------------------------
def _render(pl, cur, count, span, col_verdict, slot_verdict, tallies, min_cover, flags):
    """col_verdict[g] = (new base | 4 for deleted | None for unchanged, ambiguous); slot_verdict[c] = (key | 0, votes of the winner, ambiguous)"""
    n = len(cur)
    col_off = pl["col_off"].astype(np.int64)
    T = len(col_off) - 1
    seq, new_col, events = [], np.zeros(n + 1, np.int64), []
    cover = count.sum(axis=1, dtype=np.int64) if n else np.zeros(0, np.int64)
    tstat = np.zeros((4, T), np.uint64)
    target_of = np.zeros(n, np.int64)
    for t in range(T):
        target_of[col_off[t]:col_off[t + 1]] = t
    amb_c = amb_s = 0
    for g in range(n):
        t = target_of[g]
        new_col[g] = len(seq)
        key, kv, sa = slot_verdict[g]
        if key:
            seq.extend(bases_of(key))
            events.append((g, EV_I, key >> 26, key & ((1 << 26) - 1), kv, int(span[g])))
            tstat[2, t] += key >> 26
        w, ca = col_verdict[g]
        if w is None:
            seq.append(int(cur[g]))
        elif w == 4:
            events.append((g, EV_D, 1, int(cur[g]), int(count[g, 4]), int(cover[g])))
            tstat[1, t] += 1
        else:
            seq.append(w)
            events.append((g, EV_S, 1, int(cur[g]) | (w << 2), int(count[g, w]), int(cover[g])))
            tstat[0, t] += 1
        tstat[3, t] += int(ca) + int(sa)
        amb_c += int(ca)
        amb_s += int(sa)
    new_col[n] = len(seq)
    nc = len(seq)
    words = np.zeros((nc + 15) // 16 + 2, dtype=np.uint32)
    j = np.arange(nc, dtype=np.int64)
    np.bitwise_or.at(words, j >> 4, np.asarray(seq, dtype=np.uint32) << ((j & 15) << 1).astype(np.uint32))
    new_off = new_col[col_off]
    ev = lambda i, dt: np.array([e[i] for e in events], dtype=dt)
    info = dict(tallies)
    info.update(columns=n, voted_columns=int((cover >= min_cover).sum()), substituted=int(tstat[0].sum()), deleted=int(tstat[1].sum()),
                inserted_slots=sum(1 for e in events if e[1] == EV_I), inserted_bases=int(tstat[2].sum()), ambiguous_columns=amb_c, ambiguous_slots=amb_s,
                columns_after=nc, max_cover=int(cover.max()) if n else 0)
    assert sorted(info) == sorted(COUNTERS)
    res = dict(len=(new_off[1:] - new_off[:-1]).astype(np.int32), col_off=new_off.astype(np.uint32), begin=new_off[:-1].astype(np.uint64), words=words,
               new_col=new_col.astype(np.uint32), ev_col=ev(0, np.uint32), ev_kind=ev(1, np.uint8), ev_len=ev(2, np.uint8), ev_bases=ev(3, np.uint32),
               ev_votes=ev(4, np.uint32), ev_cover=ev(5, np.uint32), t_subs=tstat[0], t_dels=tstat[1], t_ins_bases=tstat[2], t_ambiguous=tstat[3], info=info,
               cover=cover.astype(np.uint32), old_col_off=pl["col_off"].astype(np.uint32))
    if flags & COUNTS:
        res["counts"], res["span"] = count.astype(np.uint32), np.asarray(span).astype(np.uint32)
    return res


def sequences(res):
    """the new targets as code arrays"""
    off = res["col_off"].astype(np.int64)
    return [P.codes_of(res["words"], off[t], int(off[t + 1] - off[t])) for t in range(len(off) - 1)]


def targets_of(res):
    """(words, begin, len) of the new targets: the ragged form the placement takes"""
    return res["words"], res["begin"].astype(np.int64), res["len"].copy()


def fasta(res):
    out = []
    for t, s in enumerate(sequences(res)):
        if len(s):
            out.append(">contig_id=%d_length=%d_subs=%d_ins=%d_dels=%d\n%s\n" % (t, len(s), int(res["t_subs"][t]), int(res["t_ins_bases"][t]), int(res["t_dels"][t]),
                                                                                "".join("ACGT"[b] for b in s)))
    return "".join(out)


def events_tsv(res):
    off = res["old_col_off"].astype(np.int64)
    out = []
    for i in range(len(res["ev_col"])):
        g, kind, n, bases = int(res["ev_col"][i]), int(res["ev_kind"][i]), int(res["ev_len"][i]), int(res["ev_bases"][i])
        t = max(x for x in range(len(off) - 1) if off[x] <= g and off[x + 1] > g)
        if kind == EV_S:
            old, new = "ACGT"[bases & 3], "ACGT"[bases >> 2]
        elif kind == EV_D:
            old, new = "ACGT"[bases & 3], "-"
        else:
            old, new = "-", "".join("ACGT"[b] for b in bases_of((n << 26) | bases))
        out.append("%d\t%d\t%s\t%d\t%s\t%s\t%d\t%d\n" % (t, g - int(off[t]), "SID"[kind], n, old, new, int(res["ev_votes"][i]), int(res["ev_cover"][i])))
    return "".join(out)


# ---- the statement by voters -----------------------------------------------------------------------------------------------------------------
def normalise_runs(script, read, cur, g0):
    """rule 2 on a list of runs -> (the new list of runs, shifted runs, shifted bases)"""
    at_c, at_a, c, a = [], [], g0, 0                                   # the column and the read offset every ORIGINAL run starts at
    for op, n in script:
        at_c.append(c)
        at_a.append(a)
        c += n if op != OP_I else 0
        a += n if op != OP_D else 0
    shift = [0] * len(script)
    for i in range(1, len(script) - 1):
        op, n = script[i]
        if op == OP_M or script[i - 1][0] != OP_M:
            continue
        m, s = script[i - 1][1], 0
        if op == OP_D:
            while s < m and cur[at_c[i] - (s + 1)] == cur[at_c[i] + n - (s + 1)]:
                s += 1
        else:
            while s < m and read[at_a[i] - (s + 1)] == read[at_a[i] + n - (s + 1)]:
                s += 1
        shift[i] = s
    out = []
    for i, (op, n) in enumerate(script):
        if op == OP_M:
            out.append((OP_M, n - (shift[i + 1] if i + 1 < len(script) else 0)))
        else:
            out.append((op, n))
            if shift[i]:
                out.append((OP_M, shift[i]))
    return out, sum(1 for s in shift if s), sum(shift)


def ipolish_scatter(rows, lens, pl, gp, twords, tbegin, tlen, min_cover=3, min_percent=60, max_ins=6, flags=0, reserved=0):
    voters = check(rows, lens, pl, gp, min_cover, min_percent, max_ins, flags, reserved)
    cur = _cur(pl, twords, tbegin, tlen)
    n = len(cur)
    count, span, long_ins = np.zeros((n, 5), np.int64), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    ins = [dict() for _ in range(n + 1)]
    tal = dict(voters_hamming=0, voters_gapped=0, votes=0, del_votes=0, ins_votes=0, ins_too_long=0, ins_edge=0, shifted_runs=0, shifted_bases=0)
    for kind, v, p, e, script in voters:
        read = P.codes_of(rows[v], 0, int(lens[v]))
        tal["voters_hamming" if kind == "H" else "voters_gapped"] += 1
        runs = script
        if kind == "G":
            runs, sr, sb = normalise_runs(script, read, cur, p)
            tal["shifted_runs"] += sr
            tal["shifted_bases"] += sb
        c, a = p, 0
        for i, (op, k) in enumerate(runs):
            if op == OP_M:
                for j in range(k):
                    count[c + j, read[a + j]] += 1
                tal["votes"] += k
                c, a = c + k, a + k
            elif op == OP_D:
                for j in range(k):
                    count[c + j, 4] += 1
                tal["del_votes"] += k
                c += k
            else:
                if i == 0 or i == len(runs) - 1:
                    tal["ins_edge"] += 1
                elif k > max_ins:
                    tal["ins_too_long"] += 1
                    long_ins[c] += 1
                else:
                    tal["ins_votes"] += 1
                    key = key_of(read[a:a + k])
                    ins[c][key] = ins[c].get(key, 0) + 1
                a += k
        assert c == e and a == len(read)
        span[p + 1:e] += 1
    # every column and every slot at once
    col_verdict, slot_verdict = [], []
    for g in range(n):
        cnt = [int(x) for x in count[g]]
        cover, c0 = sum(cnt), int(cur[g])
        top = max(cnt)
        w = c0 if cnt[c0] == top else cnt.index(top)
        if w != c0 and cover >= min_cover:
            col_verdict.append((w, False) if 100 * top >= min_percent * cover else (None, True))
        else:
            col_verdict.append((None, False))
        sp, votes = int(span[g]), ins[g]
        key, kv = 0, 0
        for k2 in votes:                                               # the most votes, among equals the smallest key
            if votes[k2] > kv or (votes[k2] == kv and k2 < key):
                key, kv = k2, votes[k2]
        if key and sp >= min_cover and 100 * kv >= min_percent * sp:
            slot_verdict.append((key, kv, False))
        else:
            slot_verdict.append((0, 0, sp >= min_cover and 100 * (sum(votes.values()) + int(long_ins[g])) >= min_percent * sp))
    return _render(pl, cur, count, span[:n], col_verdict, slot_verdict, tal, min_cover, flags)


# ---- the statement by columns and slots ------------------------------------------------------------------------------------------------------
def gap_events(script, read, cur, g0):
    """a script as its gaps [kind, column, read offset, length, inner], each inner one moved left one base at a time (rule 2)
    -> (the events, shifted runs, shifted bases)"""
    events, room, c, a = [], [], g0, 0
    for i, (op, n) in enumerate(script):
        if op == OP_M:
            c, a = c + n, a + n
            continue
        inner = 0 < i < len(script) - 1
        room.append(script[i - 1][1] if inner and script[i - 1][0] == OP_M else 0)
        events.append([op, c, a, n, inner])
        if op == OP_D:
            c += n
        else:
            a += n
    runs = bases = 0
    for ev, m in zip(events, room):
        moved = 0
        while moved < m:
            op, c, a, n, _ = ev
            if op == OP_D and cur[c - 1] == cur[c + n - 1]:
                ev[1] -= 1
            elif op == OP_I and read[a - 1] == read[a + n - 1]:
                ev[1] -= 1
                ev[2] -= 1
            else:
                break
            moved += 1
        runs += moved > 0
        bases += moved
    return events, runs, bases


def cells_of(p, e, events, read):
    """what a voter holds at every column of [p, e): the base of the read that stands there, or 4 for a deleted cell"""
    out = np.zeros(e - p, np.uint8)
    for g in range(p, e):
        deleted = any(op == OP_D and c <= g < c + n for op, c, a, n, _ in events)
        if deleted:
            out[g - p] = 4
            continue
        inserted = sum(n for op, c, a, n, _ in events if op == OP_I and c <= g)
        dropped = sum(n for op, c, a, n, _ in events if op == OP_D and c + n <= g)
        out[g - p] = read[g - p + inserted - dropped]
    return out


def ipolish_gather(rows, lens, pl, gp, twords, tbegin, tlen, min_cover=3, min_percent=60, max_ins=6, flags=0, reserved=0):
    voters = check(rows, lens, pl, gp, min_cover, min_percent, max_ins, flags, reserved)
    cur = _cur(pl, twords, tbegin, tlen)
    n = len(cur)
    tal = dict(voters_hamming=0, voters_gapped=0, votes=0, del_votes=0, ins_votes=0, ins_too_long=0, ins_edge=0, shifted_runs=0, shifted_bases=0)
    longest = max([v[3] - v[2] for v in voters] + [1])
    cells = np.full((len(voters), longest), 255, dtype=np.uint8)
    start = np.array([v[2] for v in voters], dtype=np.int64)
    end = np.array([v[3] for v in voters], dtype=np.int64)
    inserts = []                                                      # (slot, key or None for a long one)
    for i, (kind, v, p, e, script) in enumerate(voters):
        read = P.codes_of(rows[v], 0, int(lens[v]))
        if kind == "H":
            tal["voters_hamming"] += 1
            cells[i, :e - p] = read
            continue
        tal["voters_gapped"] += 1
        events, sr, sb = gap_events(script, read, cur, p)
        tal["shifted_runs"] += sr
        tal["shifted_bases"] += sb
        cells[i, :e - p] = cells_of(p, e, events, read)
        for op, c, a, k, inner in events:
            if op != OP_I:
                continue
            if not inner:
                tal["ins_edge"] += 1
            elif k > max_ins:
                tal["ins_too_long"] += 1
                inserts.append((c, None))
            else:
                tal["ins_votes"] += 1
                inserts.append((c, key_of(read[a:a + k])))
    count, span = np.zeros((n, 5), np.int64), np.zeros(n, np.int64)
    col_verdict, slot_verdict = [], []
    for g in range(n):
        over = np.nonzero((start <= g) & (g < end))[0]
        held = cells[over, g - start[over]]
        cnt = [int((held == b).sum()) for b in range(5)]
        count[g] = cnt
        cover, c0 = sum(cnt), int(cur[g])
        tied = [b for b in range(5) if cnt[b] == max(cnt)]
        w = c0 if c0 in tied else tied[0]
        verdict = (None, False)
        if w != c0 and cover >= min_cover:
            verdict = (w, False) if 100 * cnt[w] >= min_percent * cover else (None, True)
        col_verdict.append(verdict)
        sp = int(((start < g) & (g < end)).sum())
        span[g] = sp
        here = [k for c, k in inserts if c == g]
        best = None
        for k in here:
            if k is not None and (best is None or here.count(k) > here.count(best) or (here.count(k) == here.count(best) and k < best)):
                best = k
        if best is not None and sp >= min_cover and 100 * here.count(best) >= min_percent * sp:
            slot_verdict.append((best, here.count(best), False))
        else:
            slot_verdict.append((0, 0, sp >= min_cover and 100 * len(here) >= min_percent * sp))
    tal["votes"] = int(count[:, :4].sum())
    tal["del_votes"] = int(count[:, 4].sum())
    return _render(pl, cur, count, span, col_verdict, slot_verdict, tal, min_cover, flags)
