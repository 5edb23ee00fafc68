"""Seeded cases of the stitch stage (tests/stitch_checker.py is the definition): the smallest shapes at which the kernels can go wrong.
case(name) -> dict(seqs, twords, tbegin, tlen, entries (a, b, gap, state or None), variants (of the stitch call)); checked(name, i) -> the
checker's result for variant i, computed once.

The targets are made as in tests/merge_cases.py: windows of a random genome, as they are or as their reverse complements; target i begins at a
base with begin & 15 == 3 i mod 16.  An entry names the two ends that were cut apart (x = 2t left, 2t + 1 right) and a gap near -o."""
import functools

import numpy as np

import merge_cases as QC
import place_checker as P
import stitch_checker as ST

_rng, _seq, _sub, _pair, _pair_of, PAIRINGS = QC._rng, QC._seq, QC._sub, QC._pair, QC._pair_of, QC.PAIRINGS
JOIN = 3                                                            # SUPPORTED | JOIN: a bundle the scaffolder joined


def _make(targets, entries, variants, **extra):
    c = QC._make(targets, variants, **extra)
    c["entries"] = ST.entries_of(*entries)
    return c


def _ends(i, pairing):
    """the two ends that _pair(..., pairing) makes overlap, of targets i and i + 1"""
    return 2 * i + (pairing[0] == "R"), 2 * (i + 1) + (pairing[1] == "R")


def _pairs(rng, specs):
    """specs: [(la, lb, o, pairing, sub)] -> targets, a, b, gap = -o"""
    t, a, b, gap = [], [], [], []
    for la, lb, o, pr, sub in specs:
        x, y = _ends(len(t), pr)
        t += _pair(rng, la, lb, o, pr, sub)
        a.append(x), b.append(y), gap.append(-o)
    return t, a, b, gap


def _pairings():
    """o = min_overlap = 16 in all four end pairings; at min_overlap 17 nothing overlaps.  An empty target and one of a single base behind them"""
    rng = _rng(401)
    t, a, b, gap = _pairs(rng, [(100 + 7 * i, 131 - 5 * i, 16, pr, ()) for i, pr in enumerate(PAIRINGS)])
    return _make(t + [_seq(rng, 0), _seq(rng, 1)], (a, b, gap), [dict(), dict(min_overlap=17)])


def _half_length():
    """o = W with n = 2 o is stitched, n = 2 o - 1 is not"""
    rng = _rng(402)
    return _make(*_split(_pairs(rng, [(300, 100, 50, "RL", ()), (300, 99, 50, "RL", ())])), [dict()])


def _split(x):
    return x[0], x[1:]


def _max_overlap():
    """o = max_overlap is stitched, o = max_overlap + 1 is not: the window lies one base off"""
    rng = _rng(403)
    return _make(*_split(_pairs(rng, [(300, 280, 64, "RL", ()), (310, 290, 65, "RR", ())])), [dict(max_overlap=64), dict()])


def _full_window():
    """max_overlap 4096, the largest: windows that fill the wave's piece of LDS.  o = 4096 with a mismatch in its first and its last column, o = 4095
    (every word pair shifted by one base, the last word of the piece partial) and o = 16 at the far end of a window of 4096 (the last word pair
    of the piece).  At the default max_overlap the short one alone is seen"""
    rng = _rng(416)
    return _make(*_split(_pairs(rng, [(8200, 8300, 4096, "RL", [0, 4095]), (8192, 8200, 4095, "LR", ()), (8200, 8192, 16, "RR", ())])),
                 [dict(max_overlap=4096), dict()])


def _partial_word():
    """o in 47 / 48 / 49: the masked last word (its other bits hold whatever lies behind the overlap)"""
    rng = _rng(404)
    return _make(*_split(_pairs(rng, [(200, 210, o, PAIRINGS[i % 4], ()) for i, o in enumerate((47, 48, 49, 17, 31, 33))])), [dict()])


def _funnel():
    """min(W_a, W_b) - o at every residue mod 16: every shift of the word pair"""
    rng = _rng(405)
    return _make(*_split(_pairs(rng, [(300, 2 * (40 + r), 40, PAIRINGS[r % 4], [r] if r % 3 == 0 else ()) for r in range(16)])), [dict()])


def _passes():
    """o = min_overlap + 64 and + 65: a lane's second pass.  The third pair overlaps by 81 without a mismatch and, its overlap ending as it begins but
    for one base, by 20 with one: the best is found a pass later than the worse one.  gap -20 and slack 0 take the short one"""
    rng = _rng(406)
    t, a, b, gap = _pairs(rng, [(300, 310, 80, "RL", ()), (300, 310, 81, "LR", ())])
    v = _seq(rng, 81)
    v[61:81] = _sub(v[0:20], [7])
    x, y = _ends(len(t), "RL")
    t += [np.concatenate([_seq(rng, 200), v]), np.concatenate([v, _seq(rng, 190)])]
    return _make(t, (a + [x], b + [y], gap + [-20]), [dict(), dict(slack=0), dict(slack=61)])


def _mismatches():
    """o = 50 (the last word holds two columns).  A mismatch in the first column, in the last, in both (== max_mismatches passes), in three (+ 1
    fails), none; at max_mismatches 0, 1 and 3"""
    rng = _rng(407)
    return _make(*_split(_pairs(rng, [(220, 230, 50, PAIRINGS[i % 4], sub) for i, sub in enumerate(([0], [49], [0, 49], [0, 20, 49], (), [48, 49], [15, 16, 32]))])),
                 [dict(), dict(max_mismatches=0), dict(max_mismatches=1), dict(max_mismatches=3)])


def _short():
    """an overlap of 20: under the merge stage's min_overlap, stitched with the defaults"""
    rng = _rng(408)
    return _make(*_split(_pairs(rng, [(400, 380, 20, "RL", ())])), [dict()])


def _two_partners():
    """merge_cases' two_partners: the right end of target 0 overlaps the left ends of targets 1 and 2 alike; the entry names target 1"""
    c = QC.case("two_partners")
    return _make(c["seqs"], ([1], [2], [-55]), [dict()])


def _periodic():
    """merge_cases' periodic: a period of 10 over 80 bases at the two ends, o = 80, 70, ..., 20 at the one partner: hits 7.  gap -70: slack 0 and 9 leave
    o = 70 alone, slack 10 (|gap + o| == slack passes) admits 60 and 80 too"""
    c = QC.case("periodic")
    return _make(c["seqs"], ([1], [2], [-70]), [dict(), dict(slack=0), dict(slack=9), dict(slack=10)])


def _gap_extremes():
    """gap = 2^31 - 1, -(2^31 - 1) and -2^31: gap + o in 64 bits; every candidate lies outside the slack"""
    rng = _rng(409)
    t, a, b, gap = _pairs(rng, [(200, 210, 30, pr, ()) for pr in PAIRINGS[:3]])
    return _make(t, (a, b, [2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31]), [dict(), dict(slack=0)])


def _homopolymer():
    """two runs of A, 700 bases each: every o from 16 to 350 is a candidate, hits saturate at 255; gap -100 and slack 0 leave one"""
    return _make([np.zeros(700, np.uint8), np.zeros(700, np.uint8)], ([1], [2], [-100]), [dict(max_overlap=350), dict(), dict(max_overlap=300), dict(slack=0)])


def _unselected():
    """entries that the state does not select are ignored, whatever they hold: an end out of range, two ends of one target, ends that selected
    entries name; bundles that are only supported, and joins dropped for a cycle"""
    rng = _rng(410)
    t, a, b, gap = _pairs(rng, [(150, 160, 25, pr, ()) for pr in PAIRINGS])
    T = len(t)
    a = a[:1] + [2 * T + 5, 0, a[0]] + a[1:] + [b[1]]
    b = b[:1] + [3, 1, b[0]] + b[1:] + [0xFFFFFFFF]
    gap = gap[:1] + [0, 0, -25] + gap[1:] + [7]
    return _make(t, (a, b, gap, [JOIN, 1, 0, 2 | 4, JOIN, 2, 7, 1]), [dict()])


def _path5():
    """merge_cases' path5: five windows of one genome in a row, two of them reverse complements, in mixed id order; overlaps 50, 50, 50, 60"""
    c = QC.case("path5")
    return _make(c["seqs"], ([3, 8, 5, 0], [9, 4, 1, 6], [-48, -50, -53, -60], [JOIN] * 4), [dict()], g=c["g"])


def _ring3():
    """merge_cases' ring3 through a raw list: opened at contig 0, whose left end loses its stitch"""
    c = QC.case("ring3")
    return _make(c["seqs"], ([1, 3, 5], [2, 4, 0], [-50, -50, -50]), [dict()])


def _ring2():
    c = QC.case("ring2")
    return _make(c["seqs"], ([2, 1], [0, 3], [-50, -50]), [dict()])


def _tiny():
    """targets of length 0, 1 and 2 min_overlap - 1 (W below min_overlap) named by entries, beside a pair that is stitched"""
    rng = _rng(411)
    t, a, b, gap = _pairs(rng, [(120, 130, 24, "RL", ())])
    g = _seq(rng, 200)
    t += [_seq(rng, 0), _seq(rng, 1), g[:31], g[15:200]]                      # the last two overlap by 16, and W = 15
    return _make(t, (a + [0, 4, 9], b + [5, 6, 10], gap + [0, 0, -16]), [dict()])


def _t0():
    return _make([], ((), (), ()), [dict()])


def _j0():
    """no entry: the targets come out unchanged, as a target set"""
    rng = _rng(412)
    return _make([_seq(rng, 77), _seq(rng, 0), _seq(rng, 130)], ((), (), ()), [dict()])


def _none_selected():
    rng = _rng(413)
    t, a, b, gap = _pairs(rng, [(150, 160, 25, "RL", ())])
    return _make(t, (a, b, gap, [1]), [dict()])


CASES = {"pairings": _pairings, "half_length": _half_length, "max_overlap": _max_overlap, "full_window": _full_window, "partial_word": _partial_word, "funnel": _funnel, "passes": _passes,
         "mismatches": _mismatches, "short": _short, "two_partners": _two_partners, "periodic": _periodic, "gap_extremes": _gap_extremes, "homopolymer": _homopolymer,
         "unselected": _unselected, "path5": _path5, "ring3": _ring3, "ring2": _ring2, "tiny": _tiny, "t0": _t0, "j0": _j0, "none_selected": _none_selected}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def entries(c):
    """the entries as Engine.stitch_targets takes them: without the state where there is none"""
    return c["entries"][:3] if c["entries"][3] is None else c["entries"]


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return ST.stitch_windows(c["seqs"], c["entries"], **c["variants"][i])


@functools.lru_cache(maxsize=None)
def many(n):
    """n pairs of targets of 60 .. 90 bases and n entries: three of four overlap by 16 .. 30, in turn with a mismatch; every fifth entry is
    unselected.  Not in CASES: the GPU test lowers stitch_max_blocks on it, so that the grids stride and a wave takes further entries"""
    rng = _rng(414)
    t, a, b, gap, state = [], [], [], [], []
    for i in range(n):
        o = 16 + i % 15
        x, y = _ends(len(t), PAIRINGS[i % 4])
        if i % 4 == 3:
            t += [_seq(rng, 60 + i % 31), _seq(rng, 60 + (7 * i) % 31)]
        else:
            t += _pair(rng, 60 + i % 31, 60 + (7 * i) % 31, o, PAIRINGS[i % 4], [i % o] if i % 3 == 0 else ())
        a.append(x), b.append(y), gap.append(-o + i % 5 - 2), state.append(1 if i % 5 == 4 else JOIN)
    return _make(t, (a, b, gap, state), [dict()])


PLANTED_CUTS = ((0, 1200), (1170, 2500), (2475, 4000))                # overlaps of 30 and 25


@functools.lru_cache(maxsize=None)
def planted(dirty=False):
    """scaffold_cases' planted genome with contigs that overlap: G[0:1200] is contig 2, revcomp(G[1170:2500]) contig 0, G[2475:4000] contig 1; 1000
    pairs with outer inserts of 300 .. 400 laid over the genome (dirty: base 500 of every contig is wrong, for a polish to mend) -> the case dict of
    the placement, the genome"""
    import place_cases as PC
    import scaffold_cases as SCQ
    rng = _rng(415)
    g = _seq(rng, 4000)
    w = [g[a:b] for a, b in PLANTED_CUTS]
    tg = [P.revcomp(w[1]), w[2], w[0]]
    if dirty:
        tg = [_sub(t, [500]) for t in tg]
    reads = []
    for _ in range(SCQ.PLANTED_PAIRS):
        ins = int(rng.integers(300, 401))
        a = int(rng.integers(0, 4000 - ins + 1))
        pair = [g[a:a + 100], P.revcomp(g[a + ins - 100:a + ins])]
        reads += pair if rng.integers(0, 2) else pair[::-1]
    c = PC._make(reads, tg, pair_off=np.array([1, 1, 2, 2] * SCQ.PLANTED_PAIRS, dtype=np.uint8))
    return dict(c, seqs=tg), g


def next_round(stitched):
    """the targets that are the stitched contigs"""
    return QC._make(ST.sequences(stitched), [dict()])
