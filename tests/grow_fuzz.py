"""Seeded families of cases for the grow stage (tests/test_grow_fuzz_cpu.py, tests/test_gpu_grow_fuzz.py), in the form of tests/grow_cases.py and
through its _make: target i begins at a base with begin & 15 == 3 i mod 16 and the targets abut.  Where the cases there were each made for one
outcome, a family is made for a kind of input: a thousand targets of every length around the word, the seed and min_anchor under a few reads
per end (`many_targets`), reads that hang over by up to 237 bases (`long_overhangs`), one-letter, periodic and shared ends (`repeats`), ends with
1 to 200 voters whose columns sit exactly on the bounds of the decision (`votes`), and the bounds of k, min_anchor, W, the mismatches and
max_grow (`edges`).  Every generator is deterministic: SEEDS names the seed of each family, and first_difference() names the first array and
index at which two results differ.

A family keeps what it planted next to the case (`made`): tests/test_grow_fuzz_cpu.py asserts from it and from the checker's result that the
family holds what it is for.  As in grow_cases every target is a window [s, e) of a random genome g and a read a window of g too: a right
overhang of a bases and h more is g[e - a : e + h], a left one g[s - h : s + a]."""
import functools

import numpy as np

import grow_checker as GC
import place_checker as P
import polish_checker as Q
from grow_cases import _make, _seq, _sub, next_round, place_args  # noqa: F401  (next_round, place_args: for the users of this module)

SEEDS = {"many_targets": 501, "many_targets_small": 511, "long_overhangs": 502, "long_overhangs_small": 512, "repeats": 503, "votes": 504, "edges": 505}
TARGET_LENGTHS = (0, 1, 15, 16, 17, 62, 63, 64, 80, 99, 100, 101, 130, 200, 257)
LONG_TARGET, LONG_READ, LONG_READS, LONG_H0 = 1600, 1400, 8, 62        # the last target and the 66-seed reads over its right end: h = 62 .. 69


def _window(g, s, e, side, a, h):
    """the read that lies on the last (side 1) or the first (side 0) a bases of the target g[s:e] and h bases beyond"""
    return g[e - a:e + h] if side else g[s - h:s + a]


def _many_targets_of(seed, T, n_unmatched, n_inside, n_bound):
    rng = np.random.default_rng(seed)
    g = _seq(rng, 400 * T + 3000)
    targets, reads, spans, at = [], [], [], 300
    for t in range(T):
        n = LONG_TARGET if t == T - 1 else int(rng.choice(TARGET_LENGTHS))
        s, e = at, at + n
        flip = int(rng.random() < .5)
        targets.append(P.revcomp(g[s:e]) if flip else g[s:e])
        spans.append((s, e, flip))
        at = e + 300
        if 63 <= n < LONG_TARGET:
            for side in (0, 1):
                for _ in range(int(rng.integers(0, 6))):
                    L = int(rng.integers(64, 101))
                    a = int(rng.integers(63, min(L - 1, n) + 1))
                    r = _window(g, s, e, side, a, L - a)
                    if rng.random() < .3:
                        r = _sub(r, [int(rng.integers(0, L))])
                    reads.append(("over", P.revcomp(r) if rng.random() < .5 else r))
    s, e, _ = spans[-1]
    for i in range(LONG_READS):                                      # 66 seeds each: the usable masks of two chunks
        reads.append(("long", _window(g, s, e, 1, LONG_READ - LONG_H0 - i, LONG_H0 + i)))
    for i in range(n_inside):                                        # inside the long target: placed, no candidates
        p = s + int(rng.integers(0, LONG_TARGET - 100))
        r = g[p:p + 100] if i % 3 else _sub(g[p:p + 100], [int(rng.integers(0, 100))])
        reads.append(("inside", P.revcomp(r) if i % 2 else r))
    for _ in range(n_unmatched):                                     # random bases: candidates that lie nowhere
        reads.append(("unmatched", _seq(rng, int(rng.integers(64, 101)))))
    long_enough = [t for t in range(T - 1) if spans[t][1] - spans[t][0] >= 63]
    for i in range(n_bound):                                         # min_anchor + 1 = 64 bases: a = 63, h = 1; 63 bases: no candidate
        for L in (63, 64):
            s, e, _ = spans[long_enough[int(rng.integers(0, len(long_enough)))]]
            reads.append(("n%d" % L, _window(g, s, e, i % 2, L - 1, 1)))
    order = rng.permutation(len(reads))
    kinds = [reads[i][0] for i in order]
    return dict(_make([reads[i][1] for i in order], targets, [dict(min_cover=1), dict(), dict(min_cover=2, max_grow=5)]), g=g,
                made=dict(kinds=kinds, spans=spans))


def _many_targets():
    """1 000 targets of TARGET_LENGTHS (windows of one genome, half of them reverse complemented) and a last one of LONG_TARGET bases.  Every end of
    a target of 63 bases or more lies under 0 to 5 reads of 64 to 100 nt with 63 or more anchored bases, 30 % of them with one substitution, half
    given as the reverse complement.  In the same shuffled order: LONG_READS reads of LONG_READ nt over the right end of the last target (h = 62
    to 69: with them the growth reaches max_grow 64), reads inside it (placed), reads of random bases, and reads of 63 and 64 nt at a = L - 1.
    made: kinds (per read) and spans ((s, e, reverse complemented) per target)"""
    return _many_targets_of(SEEDS["many_targets"], 1000, 260, 40, 30)


def _many_targets_small():
    """the same generator at 40 targets: what the quadratic statement can take"""
    return _many_targets_of(SEEDS["many_targets_small"], 40, 6, 4, 3)


def _long_overhangs_of(seed, T):
    rng = np.random.default_rng(seed)
    g = _seq(rng, 1200 * T + 1000)
    targets, reads, made, at = [], [], [], 500
    for t in range(T):
        n = int(rng.integers(100, 400))
        s, e = at, at + n
        targets.append(g[s:e])
        at = e + 700
        for side in (0, 1):
            for _ in range(int(rng.integers(2, 7))):
                L = int(rng.integers(150, 301))
                a = int(rng.integers(63, min(L - 1, n) + 1))
                r = _window(g, s, e, side, a, L - a)
                subs = [int(x) for x in rng.integers(0, L, size=2)] if rng.random() < .4 else []
                made.append((2 * t + side, L - a, subs))
                r = _sub(r, subs)
                reads.append(P.revcomp(r) if rng.random() < .5 else r)
    return dict(_make(reads, targets, [dict(min_cover=1, max_grow=200), dict(min_cover=2, max_grow=65), dict(min_cover=1, max_grow=4096)]), g=g, made=made)


def _long_overhangs():
    """40 targets of 100 to 399 bases, each end under 2 to 6 reads of 150 to 300 nt with 63 or more anchored bases: overhangs of up to 237, three
    lane passes of k_gr_vote, ends walked beyond 64 columns, max_grow no multiple of 64.  Four reads in ten carry two substitutions.
    made: (end, h, the substituted positions) per read"""
    return _long_overhangs_of(SEEDS["long_overhangs"], 40)


def _long_overhangs_small():
    """the same generator at 9 targets: what the quadratic statement can take"""
    return _long_overhangs_of(SEEDS["long_overhangs_small"], 9)


ONE_LETTER, SHARED = 10, 64


def _repeats():
    """Ends that repeat.
    one_letter: ONE_LETTER targets that end in 90 A behind ten bases without an A, under a read of 100 A and one of 64 A.  With max_occ 65535 the
        long read lies at every a from 63 to 90 of every such end: more than 255 placements at mm 0 (hits 255, hits_saturated), the short one at
        a = 63 of each (hits ONE_LETTER); at the default max_occ the seeds are over it and nothing overhangs.
    period2, period3: SHARED targets each whose last 99 bases are the same repeat of GT / of ACG.  A read of 67 nt of the period-2 repeat lies at
        a = 64 and 66 of each end (hits 2 SHARED), one of 70 nt of the period-3 repeat at a = 63, 66, 69 (hits 3 SHARED); reads of 100 nt of
        either saturate.  The tie goes to the smallest e and, there, the smallest h; nobody votes.
    period10: one target that ends in nine copies of a unit of 10 bases; a read of eight copies and 20 other bases lies at a = 70 and a = 80 of
        that end: two overhangs of one end tie, the smaller h is reported, no vote.
    voters: two plain targets with three voters at one end each: they vote whatever the others do.
    made: the id of the first target and of the first read of each part"""
    rng = np.random.default_rng(SEEDS["repeats"])
    t, reads, made = [], [], {}
    made["one_letter"] = (len(t), len(reads))
    for _ in range(ONE_LETTER):
        t.append(np.concatenate([_seq(rng, 140), 1 + _seq(rng, 10) % 3, np.zeros(90, np.uint8)]).astype(np.uint8))
    reads += [np.zeros(100, np.uint8), np.zeros(64, np.uint8)]
    for name, unit, short in (("period2", (2, 3), 67), ("period3", (0, 1, 2), 70)):
        made[name] = (len(t), len(reads))
        p = len(unit)
        tail = np.tile(np.array(unit, np.uint8), 99 // p + 1)[-99:]                  # the repeat ends with the unit's last base
        for _ in range(SHARED):
            body = _seq(rng, int(rng.integers(120, 180)))
            body[-1] = (tail[p - 1] + 1) & 3                                         # the period ends there
            t.append(np.concatenate([body, tail]))
        rep = lambda n: np.tile(np.array(unit, np.uint8), n // p + 2)[:n]
        s, l = rep(short), rep(100)
        reads += [s, P.revcomp(s), l, P.revcomp(l)]
    made["period10"] = (len(t), len(reads))
    unit = np.array([0, 2, 1, 3, 3, 0, 1, 1, 2, 0], np.uint8)
    body = _seq(rng, 150)
    body[-1] = (unit[-1] + 1) & 3
    t.append(np.concatenate([body, np.tile(unit, 9)]))
    z = _seq(rng, 20)
    z[:3] = (unit[:3] + 1) & 3                                                       # a = 90 is three mismatches away
    r = np.concatenate([np.tile(unit, 8), z])
    reads += [r, P.revcomp(r)]
    made["voters"] = (len(t), len(reads))
    g = _seq(rng, 1200)
    t += [g[100:400], g[600:900]]
    reads += [g[330:430], g[325:425], P.revcomp(g[320:420]), g[570:670], P.revcomp(g[575:675]), g[580:680]]
    made["n"] = (len(t), len(reads))
    return dict(_make(reads, t, [dict(min_cover=1, max_occ=65535), dict(min_cover=1), dict(max_occ=65535)]), made=made)


# per end of `votes`: the voters' overhangs (one number: all of them) and {column: dissenting voters}
VOTE_H, VOTE_A = 16, 64
VOTE_ENDS = ((1, (16,), {}),
             (2, (16, 16), {5: 1}),                                                  # two bases tied
             (3, (16, 12, 8), {}),                                                   # the cover falls to 2 at column 8, to 1 at 12
             (5, (16,) * 5, {4: 1, 9: 2}),                                           # 4 of 5: 80 % exactly; 3 of 5
             (20, (16,) * 20, {3: 4, 7: 5, 11: 10}),                                 # 16 of 20: 80 % exactly; 15 of 20: one fewer; 10 : 10
             (64, (16,) * 64, {2: 1, 10: 32}),                                       # a single dissent; 32 : 32
             (65, (16,) * 65, {6: 13, 9: 14}),                                       # 52 of 65: 80 % exactly; 51 of 65
             (200, (16,) * 100 + (14,) * 100, {2: 40, 5: 98, 8: 41, 11: 99, 13: 1}))  # 160 and 159 of 200: 80 %; 102 and 101: 51 %; the cover halves at 14
VOTE_VARIANTS = [dict(min_percent=p, min_cover=c) for c in (1, 3) for p in (51, 80, 100)]


def _votes():
    """one target of 300 bases per entry of VOTE_ENDS, its right (even entries) or left (odd) end under that many reads of 80 nt or less with 64
    anchored bases; at column i of the growth the first `dissent[i]` voters carry another base (all the same one).  All reads in one shuffled
    order, every second one given as the reverse complement.  made: per entry (end, [(cover, top) per column])"""
    rng = np.random.default_rng(SEEDS["votes"])
    g = _seq(rng, 800 * len(VOTE_ENDS) + 800)
    targets, reads, made = [], [], []
    for t, (n, hs, dissent) in enumerate(VOTE_ENDS):
        s = 400 + 800 * t
        e, side = s + 300, 1 - t % 2
        targets.append(g[s:e])
        assert n == len(hs) and all(d <= sum(h > i for h in hs) for i, d in dissent.items())
        for v, h in enumerate(hs):
            r = _window(g, s, e, side, VOTE_A, h)
            subs = [i for i, d in dissent.items() if v < d and i < h]
            r = _sub(r, [VOTE_A + i if side else h - 1 - i for i in subs])
            reads.append(P.revcomp(r) if len(reads) % 2 else r)
        cols = []
        for i in range(max(hs)):
            cover = sum(h > i for h in hs)
            d = sum(1 for v, h in enumerate(hs) if h > i and v < dissent.get(i, 0))
            cols.append((cover, max(cover - d, d)))
        made.append((2 * t + side, cols))
    order = rng.permutation(len(reads))
    return dict(_make([reads[i] for i in order], targets, VOTE_VARIANTS), g=g, made=made, order=order)


EDGE_W = tuple(range(63, 96))                                        # the targets whose whole length is the anchored part


def _edges():
    """The bounds of the parameters, each on targets of its own (windows of one genome, 300 apart).
    whole: per n of EDGE_W a target of n bases under a read of n + 4 at one end (they alternate): a = W = n.
    bound: at the right end of a target of 200 bases reads of L = min_anchor + 1 for min_anchor 63, 31 and 8 (a = L - 1, h = 1) and one base
        shorter (no candidates there), and reads of 40 nt with a = 8 and a = 31 (a = k = min_anchor in the variants with k 8 and 31).
    mm: at the right end of a target of 250 bases reads with 0, 1, 2 and 3 substitutions in the anchored part, one of them in its last base, and
        a first overhanging base that differs from the column behind the end in the end array (the complement of base W - 1 of the next target).
    grow1: three voters at both ends of one target (max_grow 1 cuts every growth to one column).
    made: part -> (the first target, the first read)"""
    rng = np.random.default_rng(SEEDS["edges"])
    g = _seq(rng, 30000)
    targets, reads, made, at = [], [], {}, 300

    def target(n):
        nonlocal at
        s, e = at, at + n
        targets.append(g[s:e])
        at = e + 300
        return s, e

    made["whole"] = (len(targets), len(reads))
    for i, n in enumerate(EDGE_W):
        s, e = target(n)
        r = _window(g, s, e, i % 2, n, 4)
        reads.append(P.revcomp(r) if i % 3 == 0 else r)
    made["bound"] = (len(targets), len(reads))
    s, e = target(200)
    for m in (63, 31, 8):
        reads += [_window(g, s, e, 1, m, 1), _window(g, s, e, 1, m - 1, 1)]
    reads += [_window(g, s, e, 1, 8, 32), P.revcomp(_window(g, s, e, 1, 31, 9))]
    made["mm"] = (len(targets), len(reads))
    s, e = target(250)
    nxt = g[at:at + 150]                                             # the next target: its left end follows this right end in the end array
    base = _window(g, s, e, 1, 70, 30).copy()
    base[70] = ((3 - int(nxt[98])) + 1) & 3
    reads += [base, _sub(base, [69]), _sub(base, [25, 69]), _sub(base, [25, 45, 69]), P.revcomp(_sub(base, [25, 69]))]
    made["grow1"] = (len(targets), len(reads))
    s, e = target(150)
    assert (targets[-1] == nxt).all()
    reads += [_window(g, s, e, 1, 70 + i, 30 - i) for i in (0, 5, 10)] + [P.revcomp(_window(g, s, e, 0, 65 + i, 35 - i)) for i in (0, 5, 10)]
    made["n"] = (len(targets), len(reads))
    one = dict(min_cover=1)
    return dict(_make(reads, targets, [one, dict(one, k=8, min_anchor=8), dict(one, k=31, min_anchor=31), dict(one, max_mismatches=0), dict(one, max_grow=1)]), g=g, made=made)


CASES = {"many_targets": _many_targets, "many_targets_small": _many_targets_small, "long_overhangs": _long_overhangs, "long_overhangs_small": _long_overhangs_small,
         "repeats": _repeats, "votes": _votes, "edges": _edges}
GPU_FAMILIES = ("many_targets", "long_overhangs", "repeats", "votes", "edges")      # (the *_small cases are the quadratic statement's draws)
# the case the quadratic statement runs on
BRUTE = {"many_targets": "many_targets_small", "long_overhangs": "long_overhangs_small", "repeats": "repeats", "votes": "votes", "edges": "edges"}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def placed(name):
    c = case(name)
    return P.place(*place_args(c), **c["params"])


@functools.lru_cache(maxsize=None)
def _checked(name, i):
    c = case(name)
    return GC.grow_index(c["rows"], c["lens"], placed(name), c["seqs"], **c["variants"][i])


def checked(name, i=0):
    return _checked(name, i)                                         # (one cache entry whether i is given or not)


@functools.lru_cache(maxsize=None)
def fasta(name, i=0):
    """the checker's grown FASTA of variant i, rendered once"""
    return GC.fasta(checked(name, i))


@functools.lru_cache(maxsize=None)
def polished(name):
    """the polished sequences of the family's placement (tests/polish_checker.py)"""
    c = case(name)
    return Q.sequences(Q.polish_scatter(c["rows"], c["lens"], placed(name), c["twords"], c["tbegin"], c["tlen"]))


@functools.lru_cache(maxsize=None)
def checked_polished(name, i=0):
    c = case(name)
    return GC.grow_index(c["rows"], c["lens"], placed(name), polished(name), **c["variants"][i])


@functools.lru_cache(maxsize=None)
def second_round(name, i):
    """(the case whose targets are the grown ones of variant i, the placement checker's result on it, the grow checker's at the same variant)"""
    c = case(name)
    c2 = next_round(c, checked(name, i))
    pl2 = P.place(*place_args(c2), **c2["params"])
    return c2, pl2, GC.grow_index(c2["rows"], c2["lens"], pl2, c2["seqs"], **c["variants"][i])


def every(names=None):
    return [(n, i) for n in sorted(names or CASES) for i in range(len(case(n)["variants"]))]


def first_difference(got, want):
    """(array, index, got, want) of the first entry of the first array of the checker's that differs, then the first counter, or None"""
    for k in GC.ARRAYS:
        if got[k].shape != want[k].shape:
            return k, "shape", got[k].shape, want[k].shape
        d = np.nonzero(got[k] != want[k])[0]
        if len(d):
            return k, int(d[0]), got[k][d[0]], want[k][d[0]]
    for k in GC.COUNTERS:
        if got["info"][k] != want["info"][k]:
            return "info", k, got["info"][k], want["info"][k]
    return None
