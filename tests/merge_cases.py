"""Seeded cases of the merge stage (tests/merge_checker.py is the definition): the smallest shapes at which the kernels can go wrong.
case(name) -> dict(seqs, twords, tbegin, tlen, variants (of the merge call)); checked(name, i) -> the checker's result for variant i, computed
once.

Every target is a window of a random genome, as it is or as its reverse complement: two windows g[a0:a1] and g[a1 - o:b1] overlap by o at the
right end of the first and the left end of the second; a reverse complement turns a right end into a left one.  Target i begins at a base with
begin & 15 == 3 i mod 16."""
import functools

import numpy as np

import merge_checker as MC
import place_checker as P


def _rng(seed):
    return np.random.default_rng(seed)


def _seq(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _sub(c, positions):
    c = np.array(c, dtype=np.uint8, copy=True)
    for p in positions:
        c[p] = (c[p] + 1) & 3
    return c


def _make(targets, variants, **extra):
    targets = [np.asarray(t, np.uint8) for t in targets]
    twords, tbegin, tlen = P.ragged(targets, [3 * i % 16 for i in range(len(targets))])
    return dict(extra, seqs=targets, twords=twords, tbegin=tbegin, tlen=tlen, variants=variants)


def _pair_of(g, la, o, pairing="RL", sub=()):
    """the windows g[:la] and g[la - o:], which overlap by o: the right (R) or left (L) end of the first, the left or right end of the second;
    sub: overlap columns (0 = the first overlapped base of the second window) substituted in the second"""
    a, b = g[:la], _sub(g[la - o:], sub)
    return (P.revcomp(a) if pairing[0] == "L" else a), (P.revcomp(b) if pairing[1] == "R" else b)


def _pair(rng, la, lb, o, pairing="RL", sub=()):
    """two such targets of la and lb bases from a genome of their own"""
    return _pair_of(_seq(rng, la + lb - o), la, o, pairing, sub)


PAIRINGS = ("RL", "RR", "LL", "LR")


def _pairings():
    """o = min_overlap in all four end pairings, an empty target and one of a single base between them; at min_overlap 43 the same targets
    overlap by min_overlap - 1"""
    rng = _rng(301)
    t = []
    for i, pr in enumerate(PAIRINGS):
        t += _pair(rng, 100 + 7 * i, 131 - 5 * i, 42, pr)
    t.insert(2, _seq(rng, 0))
    t.insert(5, _seq(rng, 1))
    return _make(t, [dict(), dict(min_overlap=43)])


def _half_length():
    """n = 2 o joins, n = 2 o - 1 does not"""
    rng = _rng(302)
    return _make(list(_pair(rng, 300, 100, 50)) + list(_pair(rng, 300, 99, 50)), [dict()])


def _max_overlap():
    """o = max_overlap joins, o = max_overlap + 1 does not: the window of max_overlap bases lies one base off"""
    rng = _rng(303)
    return _make(list(_pair(rng, 300, 280, 64)) + list(_pair(rng, 310, 290, 65, "RR")), [dict(max_overlap=64)])


PARTIAL_O = (48, 49, 47)


def _partial_word():
    """o mod 16 in 0, 1, 15.  One mismatch (the bound) in the first or in the last overlapped base joins: it lies in seed 0 of one of the two ends,
    which finds the overlap through seed 1 only; two (first and last) do not.  The base just outside the overlap differs"""
    rng = _rng(304)
    t = []
    for i, o in enumerate(PARTIAL_O):
        while True:
            g = _seq(rng, 410 - o)
            if g[199 - o] != g[200]:                                # the bases that would be compared at o + 1
                break
        t += _pair_of(g, 200, o, PAIRINGS[i], sub=[0] if i != 1 else [o - 1])
        t += _pair(rng, 200, 210, o, PAIRINGS[i], sub=[0, o - 1])
    return _make(t, [dict()])


def _seeds64():
    """k = 8 and max_overlap = 512: an end of 64 seeds; the overlap of 512 bases has a mismatch in seed 0 of the second target's end (allowed, or not at max_mismatches 0)"""
    rng = _rng(305)
    return _make(_pair(rng, 1100, 1030, 512, "RL", sub=[3]), [dict(k=8, min_overlap=100, max_overlap=512), dict(k=8, min_overlap=100, max_overlap=512, max_mismatches=0)])


def _one_sided():
    """o = 50 with a mismatch in column 25: the right end of target 0 has seed 1 (columns 8 .. 28) broken and seed 0 (columns 29 .. 49) a second time
    in the index, at the left end of target 2; the left end of target 1 sees the overlap through its seed 0 (columns 0 .. 20).  At max_occ 1 the
    overlap exists at one end only: no join.  At the default it joins"""
    rng = _rng(306)
    g = _seq(rng, 450)
    a, b = g[:250], _sub(g[200:], [25])
    c = _seq(rng, 300)
    c[17:38] = g[229:250]
    return _make([a, b, c], [dict(max_occ=1), dict()])


def _two_partners():
    """the right end of target 0 overlaps the left ends of targets 1 and 2, which begin alike: ambiguous, no join; each of the two chooses it"""
    rng = _rng(307)
    g = _seq(rng, 500)
    return _make([g[:300], g[240:500], np.concatenate([g[240:330], _seq(rng, 150)])], [dict()])


def _periodic():
    """a period of 10 over 80 bases at the two ends: o = 80, 70, 60, 50 at one partner"""
    rng = _rng(308)
    u = np.tile(_seq(rng, 10), 8)
    while True:
        a, b = np.concatenate([_seq(rng, 150), u]), np.concatenate([u, _seq(rng, 140)])
        if a[149] != u[9] and b[80] != u[0]:                       # the period ends there
            return _make([a, b], [dict()])


def _mismatch_column():
    """an overlap of 50 with one mismatch: the merged base of that column is the earlier contig's"""
    rng = _rng(309)
    return _make(_pair(rng, 220, 230, 50, "RL", sub=[10]), [dict()], at=220 - 50 + 10)


def _path5():
    """five windows of one genome in a row, two of them reverse complements, in mixed id order; the middle one has o_left + o_right = n"""
    rng = _rng(310)
    g = _seq(rng, 1000)
    w = [g[0:300], g[250:500], g[450:550], g[500:800], g[740:1000]]
    return _make([P.revcomp(w[3]), w[0], w[2], w[4], P.revcomp(w[1])], [dict()], g=g)


def _ring3():
    """three windows around a circular genome of 600 bases: opened at contig 0, whose left end loses its join"""
    rng = _rng(311)
    g = _seq(rng, 600)
    gg = np.concatenate([g, g])
    return _make([gg[0:250], gg[200:450], gg[400:650]], [dict()], g=g)


def _ring2():
    rng = _rng(312)
    g = _seq(rng, 400)
    gg = np.concatenate([g, g])
    return _make([gg[0:250], P.revcomp(gg[200:450])], [dict()], g=g)


def _self_overlap():
    """the two ends of target 0 overlap each other by 60: a ring of one is no overlap"""
    rng = _rng(313)
    u = _seq(rng, 60)
    return _make([np.concatenate([u, _seq(rng, 200), u]), _seq(rng, 150)], [dict()])


def _t0():
    return _make([], [dict()])


def _all_empty():
    return _make([np.zeros(0, np.uint8)] * 3, [dict()])


def _one():
    return _make([_seq(_rng(314), 333)], [dict()])


def _short():
    """every target shorter than 2 min_overlap, two of them overlapping by 42"""
    rng = _rng(315)
    g = _seq(rng, 130)
    return _make([g[:83], g[41:101], _seq(rng, 20), _seq(rng, 1), _seq(rng, 0)], [dict()])


def _word_seams():
    """k_mg_build at its seams: merged contigs of 1, 15, 16, 17, 31, 32 and 33 bases (targets that join nothing) around two joined pairs, one of
    them minus-oriented; 9045 columns in all (no multiple of 16: the last word is partial, the two behind it are padding; 568 words with them: with
    merge_max_blocks 1 every lane takes several).  The empty target is in no merged contig: the stage has no empty item"""
    rng = _rng(317)
    t = [_seq(rng, n) for n in (1, 15, 16)] + [_seq(rng, 0), _seq(rng, 17)] + list(_pair(rng, 2300, 2200, 50)) + [_seq(rng, n) for n in (31, 32)]
    t += list(_pair(rng, 2250, 2250, 50, "LR")) + [_seq(rng, 33)]
    return _make(t, [dict()])


CASES = {"word_seams": _word_seams, "pairings": _pairings, "half_length": _half_length, "max_overlap": _max_overlap, "partial_word": _partial_word, "seeds64": _seeds64, "one_sided": _one_sided,
         "two_partners": _two_partners, "periodic": _periodic, "mismatch_column": _mismatch_column, "path5": _path5, "ring3": _ring3, "ring2": _ring2,
         "self_overlap": _self_overlap, "t0": _t0, "all_empty": _all_empty, "one": _one, "short": _short}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return MC.merge_index(c["seqs"], **c["variants"][i])


@functools.lru_cache(maxsize=None)
def many_ends(n):
    """n targets of 90 .. 99 bases, every 64th pair of neighbours overlapping by 45, the others unrelated.  Not in CASES: the GPU test sizes n by the
    device, so that a wave of k_mg_overlap takes a second end"""
    rng = _rng(316)
    t = []
    while len(t) < n:
        i = len(t)
        if i % 64 == 62 and i + 1 < n:
            t += _pair(rng, 90 + i % 10, 90 + (i + 1) % 10, 45, PAIRINGS[(i // 64) % 4])
        else:
            t.append(_seq(rng, 90 + i % 10))
    return _make(t, [dict()])


def next_round(merged):
    """the case whose targets are the merged contigs"""
    return _make(MC.sequences(merged), [dict()])
