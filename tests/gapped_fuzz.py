"""Seeded families of cases for the gapped placement (tests/test_gapped_fuzz_cpu.py, tests/test_gpu_gapped_fuzz.py), in the form of
tests/gapped_cases.py.  Where the cases there were each made for one outcome, a family is made for a kind of input: low-complexity sequence
(nearly every cell of a table a tie), tandem repeats, duplicated segments (ties and near ties between loci, strands and targets), reads of two
chunks of seeds, and the edges of targets, seeds and the band.  Every generator is deterministic: SEEDS names the seed of each family, and
first_difference() names the first read at which two results differ."""
import functools

import numpy as np

import gapped_checker as GC
import place_checker as P
from gapped_cases import edit, make, other, rand, targets  # noqa: F401  (targets: for the users of this module)

SEEDS = {"two_letter": 101, "three_letter": 102, "two_letter_k12": 103, "tandem": 104, "duplicates": 105, "long_reads": 106, "edges": 107, "pool": 108}
FULL_LIMIT = 200                                                     # gapped_full runs on the reads of `long_reads` up to this length only


def sub(at, b):
    """a substitution by base b as edits for edit(): the base inserted, the old one dropped (edit()'s own 'S' leaves the alphabet)"""
    return [("I", at, [int(b)]), ("D", at, 1)]


def mutate(rng, w, n_edits, alphabet, apart=4, kinds=(0, 1, 2)):
    """a copy of w with n_edits edits at least `apart` bases apart: a substitution, or an insertion or deletion of 1 to 2 bases, new bases
    from the alphabet (kinds: what to draw from, 0 a substitution, 1 an insertion, 2 a deletion)"""
    at, edits = [], []
    for _ in range(200):
        if len(at) == n_edits:
            break
        x = int(rng.integers(2, len(w) - 4))
        if all(abs(x - y) >= apart + 2 for y in at):
            at.append(x)
    for x in at:
        kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == 0:
            edits += sub(x, [b for b in alphabet if b != w[x]][int(rng.integers(0, len(alphabet) - 1))])
        elif kind == 1:
            edits.append(("I", x, [alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=int(rng.integers(1, 3)))]))
        else:
            edits.append(("D", x, int(rng.integers(1, 3))))
    return edit(w, edits)


def _letters(name, alphabet, columns, k, cut):
    """a genome over `alphabet` cut into two targets; 39 reads of 40 to 130 nt from both strands with 0 to 4 edits (the exact ones are placed by
    the Hamming pass) and one read that lies nowhere"""
    rng = np.random.default_rng(SEEDS[name])
    al = np.array(alphabet, dtype=np.uint8)
    g = al[rng.integers(0, len(al), size=columns)]
    seqs = [g[:cut], g[cut:]]
    reads = []
    for _ in range(39):
        s = seqs[int(rng.integers(0, 2))]
        W = int(rng.integers(48, 123))
        a = int(rng.integers(0, len(s) - W))
        r = mutate(rng, s[a:a + W], int(rng.integers(0, 5)), alphabet)
        reads.append(P.revcomp(r) if rng.integers(0, 2) else r)
    reads.append(al[rng.integers(0, len(al), size=90)])
    return make(reads, seqs, [dict(k=k, max_edits=2, max_occ=64), dict(k=k, max_edits=6, max_occ=64)])


def _two_letter():
    """{A, T}, 600 columns, k = 8: every seed has many occurrences, so a wave's two halves hold unrelated candidates, nearly all of which leave
    their table early, and nearly every cell is a tie between diagonal, up and left"""
    return _letters("two_letter", (0, 3), 600, 8, 250)


def _three_letter():
    """{A, C, T}, 3 000 columns, k = 8 (the minus strand reads {A, G, T})"""
    return _letters("three_letter", (0, 1, 3), 3000, 8, 1300)


def _two_letter_k12():
    """{A, T}, 3 000 columns, k = 12"""
    return _letters("two_letter_k12", (0, 3), 3000, 12, 1300)


TANDEM_PERIODS = (1, 2, 3, 7, 11, 12, 13)
TANDEM_UNITS = {1: [3], 2: [1, 2]}                                   # T; CG (its own reverse complement); the other periods: seeded
# (unit, x): A, C, AC, AG, TA -- no two of them or their reverse complements share a k-mer; TA is its own reverse complement
PURE = (([0], 3), ([1], 4), ([0, 1], 3), ([0, 2], 4), ([3, 0], 3))
PURE_LEN = 90                                                        # longer than the 80 columns of a tandem target's repeat: a pure read lies in its own target only


def _tandem():
    """k = 12, E = 3.  Per period p: 60 random columns, 80 of a period-p repeat, 60 random; nine reads of about 100 nt across it: three start
    points, each with one deleted base, one inserted base (both inside the repeat) and reverse complemented with a deletion and a substitution.
    Then four targets that are nothing but a repeat of period 1 or 2, PURE_LEN + x columns, with the read of PURE_LEN repeat bases: it lies at
    every multiple of the period up to x at d = 0, which is UNIQUE for x = E and not for x = E + 1 (p <= best.p + E); the read of TA lies at the
    same loci on both strands (+ wins, not UNIQUE).  The Hamming pass runs with max_occ 1 here so that it leaves those exact reads alone.  The
    pure reads are the last but one len(PURE) reads, in the order of PURE; the last read lies nowhere."""
    rng = np.random.default_rng(SEEDS["tandem"])
    seqs, reads = [], []
    for p in TANDEM_PERIODS:
        unit = TANDEM_UNITS.get(p)
        while unit is None or any((np.roll(unit, s) == unit).all() for s in range(1, p)):
            unit = rng.integers(0, 4, size=p)
        t = np.concatenate([rng.integers(0, 4, size=60), np.tile(unit, 80 // p + 1)[:80], rng.integers(0, 4, size=60)]).astype(np.uint8)
        seqs.append(t)
        for a, at in ((20, 60), (50, 50), (80, 40)):
            reads.append(edit(t[a:a + 101], [("D", at, 1)]))
            reads.append(edit(t[a:a + 99], [("I", at, [int(t[a + at])])]))
            reads.append(P.revcomp(edit(t[a:a + 101], [("D", at + 5, 1), ("S", at + 20)])))
    for unit, x in PURE:
        seqs.append(np.tile(unit, PURE_LEN + x)[:PURE_LEN + x].astype(np.uint8))
        reads.append(np.tile(unit, PURE_LEN)[:PURE_LEN].astype(np.uint8))
    reads.append(rng.integers(0, 4, size=100).astype(np.uint8))
    return make(reads, seqs, [dict(k=12, max_edits=3, max_occ=256)], place=dict(max_occ=1))


def _duplicates():
    """Three segments of 150 columns.  A: exact and with base 70 substituted, both in target 0.  B: exact in target 1, with base 80 deleted in
    target 2.  C: exact in target 3, reverse complemented in target 0 (the lower target: the strand decides before the target).  Reads of 100 nt
    from the exact copies, both strands: an indel on the changed base ties the two copies at equal d (not UNIQUE), an indel elsewhere leaves the
    changed copy a rival at d + 1 (UNIQUE), every read of C has equal d on both strands (+ wins, not UNIQUE).  The read of B with base 80 deleted
    is exact on target 2: the Hamming pass takes it.  The last read lies nowhere."""
    rng = np.random.default_rng(SEEDS["duplicates"])
    r = lambda n: rng.integers(0, 4, size=n).astype(np.uint8)
    A, B, C = r(150), r(150), r(150)
    seqs = [np.concatenate([r(40), A, r(30), edit(A, [("S", 70)]), r(25), P.revcomp(C), r(40)]), np.concatenate([r(30), B, r(30)]),
            np.concatenate([r(35), edit(B, [("D", 80, 1)]), r(30)]), np.concatenate([r(20), C, r(45)])]
    reads = []
    for s, changed in ((A, 70), (B, 80), (C, 75)):
        for a in (10, 30):
            w = s[a:a + 101]
            reads.append(edit(w, [("D", changed - a, 1)]))                      # the changed base itself dropped
            reads.append(edit(w, [("D", 75 - a + 3, 1)]))
            reads.append(edit(w[:99], [("I", 75 - a - 4, other(w[75 - a - 4]))]))
            reads.append(P.revcomp(edit(w, [("D", 60 - a, 1)])))
            reads.append(P.revcomp(edit(w[:99], [("I", changed - a, other(w[changed - a]))])))
        reads.append(edit(s[25:125], [("S", changed - 25)]))                     # against B's other copy: an inserted base, at equal d
    reads.append(r(100))
    return make(reads, seqs, [dict(), dict(max_edits=2)])


LONG_MADE = (8, 9, 10)                                               # reads of `long_reads`: three substitutions; chunk 0 broken; chunk 0 over max_occ


def _long_reads():
    """{A, C, T}, 2 600 columns of which 700 .. 1 300 repeat one 8-mer, k = 8, E = 6, max_occ 16, rows of blocks_of(1025) words.  Six reads of 600
    to 1 024 nt with up to 5 edits and two of 150 nt (gapped_full runs on these two alone).  Three made reads of 1 024 nt (LONG_MADE): one with
    three substitutions in seeds below 64, so every seed of chunk 1 is a duplicate through a usable seed of chunk 0; one with every seed below 64
    broken by a substitution (not placed); one whose first 512 bases lie in the repeat, every seed below 64 over max_occ, and which has a deleted
    base behind them: it is placed through chunk 1 alone, within E = 6."""
    rng = np.random.default_rng(SEEDS["long_reads"])
    al = np.array([0, 1, 3], dtype=np.uint8)
    g = al[rng.integers(0, 3, size=2600)]
    unit = np.array([0, 1, 3, 3, 1, 0, 0, 3], dtype=np.uint8)
    g[700:1300] = np.tile(unit, 75)
    reads = []
    for n in (600, 700, 800, 900, 1000, 1024, 150, 150):
        W = n - 8 if n > 1000 or n == 150 else n
        a = int(rng.integers(0, 2600 - W))
        r = mutate(rng, g[a:a + W], int(rng.integers(1, 6)), (0, 1, 3))[:1024]
        reads.append(P.revcomp(r) if rng.integers(0, 2) else r)
    w = g[1400:1400 + 1024]
    reads.append(edit(w, sub(43, 1 if w[43] != 1 else 0) + sub(250, 1 if w[250] != 1 else 0) + sub(500, 1 if w[500] != 1 else 0)))
    reads.append(edit(w, [x for j in range(64) for x in sub(8 * j + 3, 1 if w[8 * j + 3] != 1 else 0)]))
    reads.append(edit(g[780:780 + 1025], [("D", 800, 1)]))
    return make(reads, [g], [dict(k=8, max_edits=6, max_occ=16)], stride=P.blocks_of(1025))


def _edges():
    """k = 8, E = 15 and 3, max_occ 1 and 2.  Target 0: 300 random columns with one 8-mer planted twice and another three times.  Targets 1 .. 4:
    k, k + 1, k + 3 and k + 15 columns.  Reads: on the tiny targets with the seed at q = 0 and at q = len - k, bases hanging over either end;
    over either end of target 0 by x = 0, 1, 2, 3, 14, 15 bases with an indel within E of that end; an indel run of E = 3 and 15 bases directly behind a seed and directly before one; reads whose only exact seed is the 8-mer that occurs twice and the one that occurs three times"""
    rng = np.random.default_rng(SEEDS["edges"])
    r = lambda n: rng.integers(0, 4, size=n).astype(np.uint8)
    g = r(300)
    m2, m3 = r(8), r(8)
    for at in (60, 200):
        g[at:at + 8] = m2
    for at in (90, 150, 250):
        g[at:at + 8] = m3
    tiny = [r(8), r(9), r(11), r(23)]
    t1, t2, t3, t4 = tiny
    reads = [np.concatenate([t1, other(t1[-1])]), np.concatenate([r(8), t1]), t2.copy(), np.concatenate([t2[1:], r(3)]), np.concatenate([r(8), t2[:8], r(2)]),
             edit(t3, [("D", 8, 1)]), np.concatenate([other(t3[0]), t3[:7], t3[3:]]), edit(t4, [("D", 8, 3)]), edit(t4, [("D", 8, 15)]),
             np.concatenate([r(16), t4[15:], r(1)]), edit(t4, [("I", 8, r(3))])]
    for x in (0, 1, 2, 3, 14, 15):
        for near in (2, 12):                                          # the indel within 3 and within 15 bases of the end
            w = g[300 - 64 + x:]
            reads.append(np.concatenate([edit(w, [("D", len(w) - near, 1)]), r(x)]))
            w = g[:64 - x]
            reads.append(np.concatenate([r(x), edit(w, [("I", near, other(w[near]))])]))
    for E, f in ((3, 8), (15, 32)):                                  # f exact bases on either side of the run: enough that the run is the cheapest script
        m = f + (-(f + E)) % 8                                       # m + E is a multiple of k: the bases behind the run begin a seed
        for a in (20, 120):
            reads.append(np.concatenate([g[a:a + f], g[a + f + E:a + 2 * f + E]]))                # the run behind seed f / k - 1 and before seed f / k
            reads.append(np.concatenate([g[a:a + f], r(E), g[a + f:a + 2 * f]]))                 # behind seed f / k - 1, no seed after it
            reads.append(np.concatenate([g[a + 24 - m:a + 24], r(E), g[a + 24:a + 24 + f]]))     # before seed (m + E) / k
            reads.append(P.revcomp(np.concatenate([g[a + 40:a + 40 + f], g[a + 40 + f + E:a + 40 + 2 * f + E]])))
    for at in (60, 90):                                              # only the planted 8-mer stays exact
        reads.append(edit(g[at - 8:at + 16], [("S", 3), ("S", 20)]))
        reads.append(edit(g[at - 8:at + 17], [("S", 3), ("D", 18, 1)]))
    reads.append(r(64))
    return make(reads, [g] + tiny, [dict(k=8, max_edits=15, max_occ=2), dict(k=8, max_edits=3, max_occ=1), dict(k=8, max_edits=3, max_occ=2),
                                    dict(k=8, max_edits=15, max_occ=1)])


POOL = 255                                                           # odd and coprime to 7


@functools.lru_cache(maxsize=None)
def _pool_reads():
    rng = np.random.default_rng(SEEDS["pool"])
    g = rng.integers(0, 4, size=2000).astype(np.uint8)
    pool = []
    for i in range(POOL):
        n = 0 if i % 40 == 39 else (int(rng.integers(7, 10)) if i % 10 == 3 else int(rng.integers(1, 4)))
        W = int(rng.integers(60, 125)) if n > 3 else int(rng.integers(38, 143))
        a = int(rng.integers(0, 2000 - W))
        keep = 21 if W < 64 else 0                                   # a short read keeps its one or two seeds' worth of exact bases at the front
        r = np.concatenate([g[a:a + keep], mutate(rng, g[a + keep:a + W], n, (0, 1, 2, 3), kinds=(0, 1, 2, 1, 2))])
        pool.append(P.revcomp(r) if rng.integers(0, 2) else r)
    return g, pool


def _pool():
    """255 different reads of 30 to 150 nt from both strands of a 2 kb target: 1 to 3 edits (deletions, insertions, substitutions); about one in
    ten with 7 to 9 edits, more than E = 6; six exact ones, which the Hamming pass places"""
    g, pool = _pool_reads()
    return make(pool, [g])


@functools.lru_cache(maxsize=None)
def many_different_reads(n):
    """n reads drawn from the pool as pool[(7 i) mod 255]: reads i and i + 16 384 differ, so a wave of k_gp_trace that takes a second read takes a
    different one, of another length and script, and unplaced reads lie between placed ones"""
    g, pool = _pool_reads()
    return make([pool[(7 * i) % POOL] for i in range(n)], [g])


CASES = {"two_letter": _two_letter, "three_letter": _three_letter, "two_letter_k12": _two_letter_k12, "tandem": _tandem, "duplicates": _duplicates,
         "long_reads": _long_reads, "edges": _edges, "pool": _pool}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def placed(name):
    """the Hamming placement the gapped pass starts from (tests/place_checker.py)"""
    c = case(name)
    return P.place(c["rows"], c["lens"], None, *targets(c), **c["place"])


@functools.lru_cache(maxsize=None)
def _checked(name, i):
    c = case(name)
    return GC.gapped_banded(c["rows"], c["lens"], placed(name), *targets(c), **c["variants"][i])


def checked(name, i=0):
    return _checked(name, i)                                         # (one cache entry whether i is given or not)


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


def first_difference(got, want):
    """(array, index) of the first entry of the first array of the checker's that differs (for the per-read arrays the index is the read), or None"""
    for k in GC.ARRAYS:
        if got[k].shape != want[k].shape:
            return k, "shape", got[k].shape, want[k].shape
        d = np.nonzero(got[k] != want[k])[0]
        if len(d):
            return k, int(d[0]), got[k][d[0]], want[k][d[0]]
    return None


@functools.lru_cache(maxsize=None)
def shortened(name, limit=FULL_LIMIT):
    """the case with every read longer than `limit` taken out (a removed read, len -1), for the statement that fills full tables"""
    c = case(name)
    reads = [r if len(r) <= limit else None for r in c["reads"]]
    return make(reads, c["seqs"], c["variants"], c["place"], stride=c["rows"].shape[1])
