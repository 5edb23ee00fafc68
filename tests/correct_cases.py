"""Inputs of the read error correction's tests (tests/test_correct_cpu.py, tests/test_gpu_correct.py): seeded, a few hundred to 2000 reads each.

case(name) -> dict(rows, lens, params=dict(k, solid_min, min_run), truth=list of the error-free forward reads (or None), want=list of the forward
reads the definition must give (hand-stated; or None)); the checker's answer is computed once per case and shared (checked(name))."""
import numpy as np

import correct_checker as K

_cache, _checked = {}, {}


def random_set(seed, genome_len, lo, hi, coverage, rate, stride=None):
    """reads of lo .. hi nt from both strands of an iid genome, every base substituted with probability `rate`"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome_len).astype(np.uint8)
    n = int(coverage * genome_len / ((lo + hi) / 2))
    reads, truth = [], []
    for _ in range(n):
        length = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, genome_len - length + 1))
        t = g[at:at + length].copy()
        if rng.integers(0, 2):
            t = K.revcomp(t)
        r = t.copy()
        hit = rng.random(length) < rate
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        reads.append(r.astype(np.uint8))
        truth.append(t)
    rows, lens = K.nodes_of(reads, stride)
    return dict(rows=rows, lens=lens, truth=truth, want=None, genome=g)


def every_position(k=21):
    """one 70-nt locus under 12 clean reads at staggered offsets, and 70 copies of the locus read with one substitution at p = 0 .. 69"""
    rng = np.random.default_rng(701)
    g = rng.integers(0, 4, 110).astype(np.uint8)
    clean = [g[o:o + 70].copy() for o in (0, 2, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40)]
    locus = g[20:90].copy()
    reads = list(clean)
    for p in range(70):
        r = locus.copy()
        r[p] = (r[p] + 1 + p % 3) & 3
        reads.append(r)
    rows, lens = K.nodes_of(reads)
    return dict(rows=rows, lens=lens, truth=clean + [locus] * 70, want=clean + [locus] * 70)


def two_errors(k=21):
    """100-nt reads with two substitutions d = 1 .. k + 2 apart in the interior: untouched for d <= k, both fixed for d >= k + 1"""
    rng = np.random.default_rng(702)
    clean = rng.integers(0, 4, 100).astype(np.uint8)
    reads, want = [clean.copy() for _ in range(5)], [clean.copy() for _ in range(5)]
    for d in range(1, k + 3):
        p1, p2 = 25 + d, 25 + 2 * d                        # every position once per role; the roles differ in the wrong base
        r = clean.copy()
        r[p1] = (r[p1] + 1) & 3
        r[p2] = (r[p2] + 2) & 3
        reads.append(r)
        want.append(r.copy() if d <= k else clean.copy())
    rows, lens = K.nodes_of(reads)
    return dict(rows=rows, lens=lens, truth=[clean] * len(reads), want=want)


def ambiguity(k=21):
    """two copies of a (2k + 1)-nt segment that differ in the middle base, each in its own context and well covered; reads of the first copy with
    a third base there (ambiguous); and a locus whose reads disagree in one base with no version solid (no candidate)"""
    rng = np.random.default_rng(703)
    left, right = rng.integers(0, 4, k).astype(np.uint8), rng.integers(0, 4, k).astype(np.uint8)
    ctx = [rng.integers(0, 4, 30).astype(np.uint8) for _ in range(4)]
    copy_a = np.concatenate([ctx[0], left, [0], right, ctx[1]]).astype(np.uint8)
    copy_b = np.concatenate([ctx[2], left, [1], right, ctx[3]]).astype(np.uint8)
    reads = [copy_a.copy() for _ in range(6)] + [copy_b.copy() for _ in range(6)]
    third = copy_a.copy()
    third[30 + k] = 2
    reads += [third.copy() for _ in range(2)]
    n_ambiguous = 2
    lone = rng.integers(0, 4, 80).astype(np.uint8)
    for base, copies in ((0, 2), (1, 2), (3, 1)):
        for _ in range(copies):
            r = lone.copy()
            r[40] = base
            reads.append(r)
    rows, lens = K.nodes_of(reads)
    return dict(rows=rows, lens=lens, truth=None, want=[r.copy() for r in reads], n_ambiguous=n_ambiguous, n_no_candidate=5)


def shapes(k=21):
    """one read of 5000 nt with five substitutions among clean 60-nt reads; reads with len < k, == k, == k + 1; removed pairs"""
    rng = np.random.default_rng(704)
    g = rng.integers(0, 4, 5000).astype(np.uint8)
    reads = [g[o:o + 60].copy() for o in range(0, 5000 - 60 + 1, 5)]
    want = [r.copy() for r in reads]
    long_read = g.copy()
    for p in (130, 1000, 1064, 3333, 4900):
        long_read[p] = (long_read[p] + 2) & 3
    reads.append(long_read); want.append(g.copy())
    short = rng.integers(0, 4, 10).astype(np.uint8)
    reads.append(short); want.append(short.copy())                                  # len < k
    reads.append(g[200:200 + k].copy()); want.append(g[200:200 + k].copy())         # len == k, clean
    bad_k = g[300:300 + k].copy(); bad_k[7] ^= 1
    reads.append(bad_k); want.append(bad_k.copy())                                  # len == k, its one k-mer weak: the whole read, skipped
    reads.append(g[400:400 + k + 1].copy()); want.append(g[400:400 + k + 1].copy())
    bad_k1 = g[500:500 + k + 1].copy(); bad_k1[0] ^= 2
    reads.append(bad_k1); want.append(g[500:500 + k + 1].copy())                    # len == k + 1, left-end run [0, 0]
    bad_k1r = g[600:600 + k + 1].copy(); bad_k1r[k] ^= 3
    reads.append(bad_k1r); want.append(g[600:600 + k + 1].copy())                   # ... right-end run [1, 1]
    reads += [None, None]; want += [None, None]
    reads.append(np.zeros(0, dtype=np.uint8)); want.append(np.zeros(0, dtype=np.uint8))   # len 0
    rows, lens = K.nodes_of(reads)
    return dict(rows=rows, lens=lens, truth=None, want=want)


def heavy():
    """one 60-nt read 600 times (its k-mers' bins are above a slice budget of 256), one copy with an error, and a few other reads"""
    rng = np.random.default_rng(705)
    r0 = rng.integers(0, 4, 60).astype(np.uint8)
    reads = [r0.copy() for _ in range(600)]
    bad = r0.copy(); bad[30] = (bad[30] + 1) & 3
    reads.append(bad)
    other = rng.integers(0, 4, 200).astype(np.uint8)
    reads += [other[o:o + 60].copy() for o in range(0, 140, 7)]
    want = [r0.copy() for _ in range(601)] + [r.copy() for r in reads[601:]]
    rows, lens = K.nodes_of(reads)
    return dict(rows=rows, lens=lens, truth=None, want=want)


def all_removed():
    rows, lens = K.nodes_of([None] * 7, stride=4)
    return dict(rows=rows, lens=lens, truth=None, want=[None] * 7)


def empty():
    return dict(rows=np.zeros((0, 4), dtype=np.uint32), lens=np.zeros(0, dtype=np.int32), truth=None, want=[])


# name -> (maker, params).  The seeds of the random sets are those for which the checker changes no error-free read and makes none worse
# (tests/test_correct_cpu.py asserts both).
CASES = {
    "rand_k21": (lambda: random_set(11, 4000, 60, 100, 30, 0.01), dict(k=21, solid_min=3, min_run=1)),
    "rand_k15": (lambda: random_set(12, 4000, 60, 100, 30, 0.01), dict(k=15, solid_min=3, min_run=1)),
    "rand_k31": (lambda: random_set(13, 4000, 64, 100, 30, 0.01), dict(k=31, solid_min=3, min_run=1)),
    "rand_2pct": (lambda: random_set(14, 4000, 60, 100, 30, 0.02), dict(k=21, solid_min=3, min_run=1)),
    "rand_small": (lambda: random_set(15, 3000, 40, 70, 30, 0.005), dict(k=21, solid_min=2, min_run=1)),
    "rand_minrun3": (lambda: random_set(16, 4000, 60, 100, 30, 0.01), dict(k=21, solid_min=3, min_run=3)),
    "wide_stride": (lambda: random_set(17, 1000, 60, 100, 30, 0.01, stride=16), dict(k=21, solid_min=3, min_run=1)),
    "every_position": (every_position, dict(k=21, solid_min=3, min_run=1)),
    "two_errors": (two_errors, dict(k=21, solid_min=3, min_run=1)),
    "ambiguity": (ambiguity, dict(k=21, solid_min=3, min_run=1)),
    "shapes": (shapes, dict(k=21, solid_min=3, min_run=1)),
    "heavy": (heavy, dict(k=21, solid_min=3, min_run=1)),
    "all_removed": (all_removed, dict(k=21, solid_min=3, min_run=1)),
    "empty": (empty, dict(k=21, solid_min=3, min_run=1)),
}
RANDOM = [n for n in CASES if n.startswith("rand_") or n == "wide_stride"]


def case(name):
    if name not in _cache:
        maker, params = CASES[name]
        c = maker()
        c["params"] = params
        c["rows"].setflags(write=False)
        c["lens"].setflags(write=False)
        _cache[name] = c
    return _cache[name]


def checked(name):
    """(rows, info) of the checker on a case: computed once, read only"""
    if name not in _checked:
        c = case(name)
        rows, info = K.correct(c["rows"], c["lens"], **c["params"])
        rows.setflags(write=False)
        _checked[name] = (rows, info)
    return _checked[name]
