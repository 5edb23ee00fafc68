"""Seeded cases of the grow stage (tests/grow_checker.py is the definition): the smallest shapes at which the kernels can go wrong.
case(name) -> dict(rows, lens, pair_off = None, twords, tbegin, tlen, seqs, params (of the placement), variants (of the grow call));
placed(name) -> the placement checker's result, checked(name, i) -> the grow checker's result for variant i, both computed once.

Every target is a window [s, e) of a random genome g and every read a window of g too: a right overhang of a bases and h more is
g[e - a : e + h], a left one g[s - h : s + a].  A read given as it is lies on the `+` strand at a right end and on the `-` strand at a left end
(the twin's right overhang on the mirrored end)."""
import functools

import numpy as np

import grow_checker as GC
import place_checker as P

K = 21


def _rng(seed):
    return np.random.default_rng(seed)


def _seq(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _sub(c, positions):
    c = np.array(c, dtype=np.uint8, copy=True)
    for p in positions:
        c[p] = (c[p] + 1) & 3
    return c


def _make(reads, targets, variants, shifts=None, gaps=None, **params):
    rows, lens = P.nodes_of(reads)
    twords, tbegin, tlen = P.ragged(targets, shifts if shifts is not None else [3 * i % 16 for i in range(len(targets))], gaps)
    return dict(rows=rows, lens=lens, pair_off=None, twords=twords, tbegin=tbegin, tlen=tlen, seqs=[np.asarray(t, np.uint8) for t in targets], params=params,
                variants=variants)


ONE = dict(min_cover=1)


def _h_extremes():
    # h = 1 and h = L - min_anchor = 37 at both ends; h = 38 leaves 62 anchored bases: no placement
    g = _seq(_rng(101), 700)
    reads = [g[401:501], g[437:537], g[438:538], g[199:299], g[163:263], g[162:262]]
    return dict(_make(reads, [g[200:500]], [ONE]), g=g)


def _a_equals_w():
    # target 0 has 80 bases: shorter than the reads (100) and than Lmax - 1, so W = 80; a = 80 is the whole target, a = 81 does not exist
    g = _seq(_rng(102), 900)
    reads = [g[100:200], g[99:199], P.revcomp(g[80:180]), g[620:720]]
    return dict(_make(reads, [g[100:180], g[300:700]], [ONE]), g=g)


PARTIAL_A = (64, 65, 79, 80, 81)


def _partial_word():
    # a mod 16 = 0, 1, 15, 0, 1 with mm at the bound (one of the two in the last anchored base): an overhanging base that is compared is one too many
    g = _seq(_rng(103), 800)
    reads = [_sub(g[500 - a:600 - a], [30, a - 1]) for a in PARTIAL_A]
    return dict(_make(reads, [g[100:500], g[550:750]], [ONE]), g=g)


def _mm_bound():
    # mm = 2 and 3 with a mismatch in the last anchored base; the first overhanging base differs from the base behind the end in the end array (the
    # first base of the next end: the complement of base 98 of the next target)
    g = _seq(_rng(104), 800)
    A, Cn = g[100:400], g[450:700]
    nb = 3 - int(Cn[98])
    base = g[330:430].copy()                                                  # a = 70, h = 30 at the right end of A
    base[70] = (nb + 1) & 3
    left = g[420:520]                                                        # h = 30, a = 70 at the left end of Cn: the twin's last anchored base is base 30
    reads = [_sub(base, [25, 69]), _sub(base, [25, 45, 69]), _sub(base, [25, 45]), _sub(left, [30, 60]), _sub(left, [30, 60, 80])]
    return dict(_make(reads, [A, Cn], [ONE]), g=g)


def _tiny_targets():
    # targets of 0, min_anchor - 1 and min_anchor bases between longer ones, all abutting in the packed array
    g = _seq(_rng(105), 1500)
    targets = [g[0:300], g[0:0], g[400:462], g[500:563], g[700:1000]]
    reads = [g[500:600], g[400:500], g[463:563], g[930:1030], g[270:370]]
    return dict(_make(reads, targets, [ONE], shifts=[5, 0, 0, 0, 0], gaps=[True, False, False, False, False]), g=g)


def _period3():
    # an end of 90 bases of a period-3 repeat: a read of pure repeat lies there at a = 63, 66, .. 90 with mm 0 -> hits 10, no vote
    rng = _rng(106)
    rep = np.tile(np.array([0, 1, 2], np.uint8), 30)
    g = _seq(rng, 600)
    reads = [np.tile(np.array([0, 1, 2], np.uint8), 34)[:100], g[330:430]]
    return dict(_make(reads, [np.concatenate([_seq(rng, 200), rep]), g[100:400]], [ONE]), g=g)


def _equal_ends():
    # two targets that end in the same 99 bases: a tie across ends (the smaller e is the best, nobody votes); with max_occ = 1 every seed is over
    rng = _rng(107)
    tail, ext = _seq(rng, 99), _seq(rng, 30)
    read = np.concatenate([tail[29:], ext])
    return _make([read, P.revcomp(read)], [np.concatenate([_seq(rng, 200), tail]), np.concatenate([_seq(rng, 150), tail])], [ONE, dict(min_cover=1, max_occ=1)])


def _mid(a, b):
    """one substitution in the middle of each of the seeds a .. b - 1 (k = 21)"""
    return [K * j + 10 for j in range(a, b)]


def _second_chunk():
    # 1400-nt reads, 66 seeds in two chunks of 64: read 1 and its reverse complement are found only through seeds 64 and 65, read 3 through none;
    # read 0 through every seed (the seeds of chunk 1 ask for the usable masks of chunk 0)
    g = _seq(_rng(108), 3200)
    base = g[310:1710]                                                       # a = 1390, h = 10 at the right end of g[100:1700]
    r1 = _sub(base, _mid(0, 64))
    reads = [base, r1, P.revcomp(r1), _sub(base, _mid(0, 66))]
    return dict(_make(reads, [g[100:1700], g[2000:2400]], [dict(min_cover=1, max_mismatches=70), ONE]), g=g)


def _cover():
    # voters with h = 30, 20, 10: cover 3 on columns 0 .. 9, 2 on 10 .. 19; with max_grow = 8 the growth is cut there
    g = _seq(_rng(109), 600)
    reads = [g[330:430], g[320:420], g[310:410]]
    return dict(_make(reads, [g[100:400]], [dict(), dict(min_cover=2), dict(min_cover=1, max_grow=8)]), g=g)


def _percent():
    # five voters: column 5 has 4 of 5 (80 %: passes at min_percent 80), column 8 has 3 of 5
    g = _seq(_rng(110), 600)
    r = g[330:430]
    reads = [r, r, r, _sub(r, [78]), _sub(r, [75, 78])]
    return dict(_make(reads, [g[100:400]], [dict(), dict(min_percent=81), dict(min_percent=60)]), g=g)


def _minus_only():
    g = _seq(_rng(111), 600)
    reads = [P.revcomp(g[330:430]), P.revcomp(g[325:425]), P.revcomp(g[320:420])]
    return dict(_make(reads, [g[100:400]], [dict()]), g=g)


def _left_grow():
    g = _seq(_rng(112), 600)
    reads = [g[70:170], g[75:175], P.revcomp(g[80:180])]
    return dict(_make(reads, [g[100:400]], [dict()]), g=g)


def _both_ends():
    # a target of 70 bases under reads of 80: both ends grow by 10
    g = _seq(_rng(113), 400)
    reads = [g[100 - h:180 - h] for h in (15, 12, 10)] + [g[170 - a:250 - a] for a in (65, 68, 70)]
    return dict(_make(reads, [g[100:170]], [dict()]), g=g)


def _n0():
    return _make([], [_seq(_rng(114), 200)], [dict()])


def _t0():
    return _make([_seq(_rng(115), 100)], [], [dict()])


def _all_placed():
    g = _seq(_rng(116), 500)
    return _make([g[p:p + 100] for p in range(0, 400, 40)], [g], [dict()])


SEAM_LENS = (1, 15, 16, 17, 0, 15, 16, 17, 31, 32, 33)
SEAM_NEW_LENS = [1, 31, 32, 33, 0, 15, 16, 17, 51, 52, 53, 2364, 2300]


def _word_seams():
    """k_gr_ends and k_gr_build at their seams.  Ends of 1, 15, 16, 17, 31, 32 and 33 columns, two of width 0 between them (an empty target), 9182 end
    columns in all (no multiple of 16; 574 words).  Targets 1 .. 3 grow by 8 at both ends, 8 .. 10 by 20 at the right end, target 11 by the 64 of
    max_grow: the new lengths (SEAM_NEW_LENS) hold 1, 15, 16, 17, 31, 32, 33 and a 0, 4965 new columns in all (no multiple of 16; 311 words and
    the two of padding).  k = 8 and min_anchor = 8, so that the short ends anchor a read; the 2200-base read makes W = len for every short target"""
    g, G = _seq(_rng(117), 1300), _seq(_rng(118), 5200)
    targets, reads = [], []
    for i, n in enumerate(SEAM_LENS):
        s = 60 + 100 * i
        e = s + n
        targets.append(g[s:e])
        if i in (1, 2, 3):
            reads += [g[e - 12:e + 8], g[s - 8:s + 12]]
        if i >= 8:
            reads.append(g[e - 20:e + 20])
    targets += [G[100:2400], G[2700:5000]]
    reads.append(G[300:2500])                                                 # a = 2100, h = 100 at the right end of target 11
    return dict(_make(reads, targets, [dict(k=8, min_anchor=8, min_cover=1)]), g=g)


CASES = {"word_seams": _word_seams, "h_extremes": _h_extremes, "a_equals_w": _a_equals_w, "partial_word": _partial_word, "mm_bound": _mm_bound, "tiny_targets": _tiny_targets, "period3": _period3,
         "equal_ends": _equal_ends, "second_chunk": _second_chunk, "cover": _cover, "percent": _percent, "minus_only": _minus_only, "left_grow": _left_grow,
         "both_ends": _both_ends, "n0": _n0, "t0": _t0, "all_placed": _all_placed}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


def place_args(c):
    return c["rows"], c["lens"], c["pair_off"], c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def placed(name):
    c = case(name)
    return P.place(*place_args(c), **c["params"])


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return GC.grow_index(c["rows"], c["lens"], placed(name), c["seqs"], **c["variants"][i])


@functools.lru_cache(maxsize=None)
def many_reads(n):
    """n reads of 64 .. 75 nt on four targets behind eight 1400-nt reads that hang over the end of a fifth (66 seeds: the usable masks of two
    chunks stay in the scratch of the waves that take a short read next).  Of the short reads three in four hang over an end, the others lie
    inside a target or nowhere.  Not in CASES: the GPU test sizes n by the device, so that a wave of k_gr_place takes more than one candidate"""
    assert n >= 8
    rng = _rng(117)
    g = _seq(rng, 6000)
    bounds = [(100, 800), (1000, 1333), (1500, 2700), (2900, 2965), (3200, 4800)]
    reads = []
    for i in range(n):
        if i < 8:
            reads.append(g[4800 - 1390 + i:4800 + 10 + i])
        else:
            s, e = bounds[i % 4]
            L = int(rng.integers(64, 76))
            a = int(rng.integers(60, L))
            if i % 4 == 3:
                r = g[105 + i % 600:105 + i % 600 + L] if i % 8 == 3 else _seq(rng, L)
            elif (i // 4) & 1:
                r = g[e - a:e - a + L]
            else:
                r = g[s - (L - a):s + a]
            if i % 5 == 0:
                r = _sub(r, [int(rng.integers(0, L))])
            reads.append(P.revcomp(r) if i % 3 == 0 else r)
    return dict(_make(reads, [g[s:e] for s, e in bounds], [dict()], shifts=[3, 0, 9, 14, 6]), g=g)


# ---- the planted genome ----------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_BOUNDS = 7, ((50, 1200), (1320, 2950))


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED, n_reads=1200, genome=3000):
    """a random genome, two contigs with a gap of 120 between them and 50 bases missing at the genome's ends, 100-nt reads at 40x with 1 %
    substitutions, half of them given as the reverse complement -> the case, the genome, per read (start, error-free)"""
    rng = _rng(seed)
    g = _seq(rng, genome)
    reads, meta = [], []
    for _ in range(n_reads):
        a = int(rng.integers(0, genome - 100 + 1))
        r = g[a:a + 100].copy()
        err = rng.random(100) < 0.01
        r[err] = (r[err] + rng.integers(1, 4, size=int(err.sum()))) & 3
        meta.append((a, not err.any()))
        reads.append(P.revcomp(r) if rng.random() < 0.5 else r.astype(np.uint8))
    c = _make(reads, [g[s:e] for s, e in PLANTED_BOUNDS], [dict()])
    return c, g, meta


def next_round(c, grown):
    """the case whose targets are the grown ones"""
    seqs = GC.sequences(grown)
    twords, tbegin, tlen = P.ragged(seqs, [3 * i % 16 for i in range(len(seqs))])
    return dict(c, twords=twords, tbegin=tbegin, tlen=tlen, seqs=seqs)
