"""The definition of the break stage (include/alga_amd.h: alga_break_placed_device), twice, in Python.

break_columns() asks, for every column, every proper pair of its target whether it spans the column, and walks the columns of a target one by
one for the runs.  break_pairs() adds every pair to the slice of columns it spans and takes the runs from the differences of the weak mask.
Neither shares anything with the device's method: no difference array of the spans with a scan, no compaction.
Both take a placement as tests/place_checker.py returns it (target, pos, state, col_off, insert_hist) and the bases of the placed targets as
code arrays (the targets, or the polished sequences)."""
import numpy as np

import place_checker as P
import scaffold_checker as SC

ARRAYS = ("span", "cut_cols", "cut_first", "cut_last", "t_cuts", "piece_off", "begin", "len", "piece_target", "piece_start", "words")
COUNTERS = ("pairs_proper", "pairs_spanning", "candidate_columns", "weak_columns", "runs", "runs_open", "cuts", "targets_cut", "pieces", "max_span", "longest_piece",
            "n50_targets", "n50_pieces")
DEFAULT = dict(min_span=1, inset=21)


def check(rows, lens, pair_off, pl, margin, min_span, inset):
    """the refusals -> the proper pairs as (target, a, b + lb), the targets' lengths"""
    if not 1 <= min_span <= 2 ** 31 - 1 or not 0 <= inset <= 2 ** 20 or not 0 <= margin <= 2 ** 20:
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
    for r in range(n // 2):
        if not int(pl["state"][r]) & P.UNIQUE:
            continue
        L, t, p = int(lens[2 * r + 1]), int(pl["target"][r]), int(pl["pos"][r])
        if L < 1 or L > 16 * stride:
            raise ValueError("read length")
        if not 0 <= t < len(tlen) or p < 0 or p + L > tlen[t]:
            raise ValueError("a read leaves its target")
    max_insert = len(pl["insert_hist"]) - 1
    proper = []
    if pair_off is not None:
        for r in range(n // 2):
            if pair_off[2 * r + 1] != 1:
                continue
            s1, s2 = int(pl["state"][r]), int(pl["state"][r + 1])
            if not (s1 & P.UNIQUE and s2 & P.UNIQUE) or pl["target"][r] != pl["target"][r + 1] or (s1 & P.MINUS) == (s2 & P.MINUS):
                continue
            rp, rm = (r + 1, r) if s1 & P.MINUS else (r, r + 1)
            a, la, b, lb = int(pl["pos"][rp]), int(lens[2 * rp + 1]), int(pl["pos"][rm]), int(lens[2 * rm + 1])
            if a <= b and a + la <= b + lb and b + lb - a <= max_insert:
                proper.append((int(pl["target"][r]), a, b + lb))
    return proper, tlen


def column_words(seqs):
    """the sequences one behind the other in column space: column g in word g >> 4 at bits 2 * (g & 15), two words of padding"""
    c = np.concatenate([np.asarray(s, np.uint32) for s in seqs] + [np.zeros(0, np.uint32)])
    words = np.zeros((len(c) + 15) // 16 + 2, dtype=np.uint32)
    i = np.arange(len(c), dtype=np.int64)
    np.bitwise_or.at(words, i >> 4, c << ((i & 15) << 1).astype(np.uint32))
    return words


def _result(tlen, seqs, span, runs, counts):
    """span: per column; runs: [(target, s, e, closed)] in target-local columns, in column order"""
    T = len(tlen)
    col_off = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    cuts = [(t, (s + e + 1) // 2, s, e) for t, s, e, closed in runs if closed]
    pieces = []                                                     # (target, start, length)
    for t in range(T):
        at = [0] + [c for tt, c, _, _ in cuts if tt == t] + [int(tlen[t])]
        pieces += [(t, a, b - a) for a, b in zip(at, at[1:])]
    t_cuts = np.zeros(T, np.uint32)
    for t, _, _, _ in cuts:
        t_cuts[t] += 1
    off = [int(col_off[t]) + s for t, s, _ in pieces]
    res = dict(span=np.asarray(span, np.uint32), cut_cols=np.array([col_off[t] + c for t, c, _, _ in cuts], np.uint32),
               cut_first=np.array([col_off[t] + s for t, _, s, _ in cuts], np.uint32), cut_last=np.array([col_off[t] + e for t, _, _, e in cuts], np.uint32),
               t_cuts=t_cuts, piece_off=np.array(off + [int(col_off[-1])], np.uint32), begin=np.array(off, np.uint64), len=np.array([n for _, _, n in pieces], np.int32),
               piece_target=np.array([t for t, _, _ in pieces], np.int32), piece_start=np.array([s for _, s, _ in pieces], np.uint32), words=column_words(seqs))
    assert [len(s) for s in seqs] == [int(x) for x in tlen]
    res["info"] = dict(counts, runs=len(runs), runs_open=len(runs) - len(cuts), cuts=len(cuts), targets_cut=int((t_cuts > 0).sum()), pieces=len(pieces),
                       max_span=int(max(list(span) + [0])), longest_piece=max([n for _, _, n in pieces] + [0]), n50_targets=SC.n50(tlen),
                       n50_pieces=SC.n50([n for _, _, n in pieces]))
    return res


def break_columns(rows, lens, pair_off, pl, seqs, margin, min_span=1, inset=21):
    """every column asks every proper pair of its target; the runs by walking the columns"""
    proper, tlen = check(rows, lens, pair_off, pl, margin, min_span, inset)
    span, runs, n_cand, n_weak = [], [], 0, 0
    for t in range(len(tlen)):
        lo = np.array([a + inset for tt, a, _ in proper if tt == t], np.int64)
        hi = np.array([e - inset for tt, _, e in proper if tt == t], np.int64)
        run = None                                                  # the first column of the run at hand
        for j in range(int(tlen[t])):
            sp = int(np.count_nonzero((lo <= j) & (j < hi)))
            span.append(sp)
            cand = margin <= j < tlen[t] - margin
            weak = cand and sp < min_span
            n_cand += cand
            n_weak += weak
            if weak and run is None:
                run = j
            if run is not None and not weak:                        # the run ended at j - 1; j closes it iff it is a candidate
                runs.append((t, run, j - 1, run - 1 >= margin and cand))
                run = None
        if run is not None:                                         # it ran to the target's end
            runs.append((t, run, int(tlen[t]) - 1, False))
    counts = dict(pairs_proper=len(proper), pairs_spanning=sum(1 for _, a, e in proper if e - a > 2 * inset), candidate_columns=int(n_cand), weak_columns=int(n_weak))
    return _result(tlen, seqs, span, runs, counts)


def break_pairs(rows, lens, pair_off, pl, seqs, margin, min_span=1, inset=21):
    """every pair adds to the slice it spans; the runs from the differences of the weak mask"""
    proper, tlen = check(rows, lens, pair_off, pl, margin, min_span, inset)
    col_off = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    span = np.zeros(int(col_off[-1]), np.int64)
    n_span = 0
    for t, a, e in proper:
        if e - inset > a + inset:
            span[col_off[t] + a + inset:col_off[t] + e - inset] += 1
            n_span += 1
    runs, n_cand, n_weak = [], 0, 0
    for t in range(len(tlen)):
        n = int(tlen[t])
        j = np.arange(n)
        cand = (j >= margin) & (j < n - margin)
        weak = cand & (span[col_off[t]:col_off[t + 1]] < min_span)
        n_cand += int(cand.sum())
        n_weak += int(weak.sum())
        d = np.diff(np.concatenate([[0], weak.astype(np.int8), [0]]))
        for s, e in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1):
            runs.append((t, int(s), int(e), bool(s - 1 >= margin and e + 1 < n - margin)))
    counts = dict(pairs_proper=len(proper), pairs_spanning=n_span, candidate_columns=n_cand, weak_columns=n_weak)
    return _result(tlen, seqs, span, runs, counts)


def pieces_of(res):
    """the pieces as code arrays, in piece order"""
    return [P.codes_of(res["words"], int(res["piece_off"][j]), int(res["len"][j])) for j in range(len(res["len"]))]


def fasta(res):
    """the piece FASTA as bytes: one record per piece with a length"""
    out = []
    for j, s in enumerate(pieces_of(res)):
        if len(s):
            out.append(">contig_id=%d_length=%d_from=%d_start=%d\n%s\n" % (j, len(s), res["piece_target"][j], res["piece_start"][j], "".join("ACGT"[x] for x in s)))
    return "".join(out).encode()


def cuts_tsv(res):
    """one line per cut: contig cut run_first run_last, in target-local columns (the piece behind a cut is the one that starts inside its target)"""
    out = []
    behind = [j for j in range(len(res["len"])) if res["piece_start"][j] > 0]
    assert len(behind) == len(res["cut_cols"])
    for i, j in enumerate(behind):
        base = int(res["piece_off"][j]) - int(res["piece_start"][j])
        out.append("%d\t%d\t%d\t%d\n" % (res["piece_target"][j], int(res["cut_cols"][i]) - base, int(res["cut_first"][i]) - base, int(res["cut_last"][i]) - base))
    return "".join(out).encode()
