"""Seeded families of cases for the merge stage (tests/test_merge_fuzz_cpu.py, tests/test_gpu_merge_fuzz.py), in the form of tests/merge_cases.py
and through its _make: target i begins at a base with begin & 15 == 3 i mod 16.  Where the cases there were each made for one outcome, a family
is made for a kind of input: long chains and rings of windows in shuffled id order and mixed orientation (`chains`), chains whose overlaps carry
a substitution (`chain_mismatches`), low-complexity, periodic and duplicated ends (`repeats`), the bounds of the overlap, the word and the seed
(`edges`), and chains of long windows whose merged FASTA takes several chunks (`long_windows`).  Every generator is deterministic: SEEDS names the
seed of each family, and first_difference() names the first array and index at which two results differ.

A family keeps what it planted next to the targets (`groups`, `made`, ...): tests/test_merge_fuzz_cpu.py asserts from these and from the checker's
result that the family holds what it is for."""
import functools

import numpy as np

import merge_checker as MC
import place_checker as P
from merge_cases import PAIRINGS, _make, _pair, _seq, _sub, next_round, targets  # noqa: F401  (next_round, targets: for the users of this module)

SEEDS = {"chains": 401, "chains_small": 402, "chain_mismatches": 403, "chain_mismatches_small": 407, "repeats": 404, "edges": 405, "long_windows": 406}
CHAIN_LENGTHS = (2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1025)
RING_LENGTHS = (2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 64, 65, 513)
SMALL_CHAINS, SMALL_RINGS = (2, 3, 4, 33), (17,)                     # the reduced draw of `chains` for the quadratic statement: 59 windows


def _windows(rng, m, ring, n_range=(120, 170), o_range=(42, 60), alphabet=4, half=()):
    """m windows along a random genome (ring: around a circular one), window i overlapping window i + 1 by o[i]: ([window], [o]).  Every window is
    at least twice the largest overlap long, so that W = len / 2 holds the overlap, and at least o_left + o_right, so that only neighbours
    overlap.  half: the windows that are o_left + o_right long exactly (both overlaps are half of them)"""
    n = [int(x) for x in rng.integers(*n_range, size=m)]
    o = [int(x) for x in rng.integers(*o_range, size=m if ring else m - 1)]
    for i in half:                                                   # 0 < i < m - 1: n = 2 o, and the overlap on either side is o
        o[i - 1] = o[i] = int(rng.integers(o_range[0], min(o_range[1], n_range[0] // 2 + 1)))
        n[i] = 2 * o[i]
    at = np.concatenate([[0], np.cumsum([n[i] - o[i] for i in range(len(o))])]).astype(np.int64)
    if ring:
        G = int(at[-1])                                              # the circle: every window begins where the one before ends less its overlap
        g = rng.integers(0, alphabet, size=G).astype(np.uint8)
        w = [g[(int(at[i]) + np.arange(n[i])) % G] for i in range(m)]
    else:
        g = rng.integers(0, alphabet, size=int(at[-1]) + n[-1]).astype(np.uint8)
        w = [g[int(at[i]):int(at[i]) + n[i]].copy() for i in range(m)]
    if alphabet == 2:
        w = [3 * x for x in w]                                       # {A, T}
    return w, o


def _shuffled(rng, groups, extra=()):
    """groups: [(kind, [window], [o])].  All windows and the `extra` targets in one shuffled id order, every window reverse complemented with
    probability one half: (targets, [(kind, [id], [flipped], [o])])"""
    n = sum(len(w) for _, w, _ in groups) + len(extra)
    ids = [int(x) for x in rng.permutation(n)]
    t, out, at = [None] * n, [], 0
    for kind, w, o in groups:
        mine, flipped = ids[at:at + len(w)], [int(x) for x in rng.integers(0, 2, size=len(w))]
        at += len(w)
        for i, s, f in zip(mine, w, flipped):
            t[i] = P.revcomp(s) if f else s
        out.append((kind, mine, flipped, o))
    for i, s in zip(ids[at:], extra):
        t[i] = s
    return t, out


def _chains_of(seed, chain_lengths, ring_lengths, **kw):
    rng = np.random.default_rng(seed)
    groups = [("chain", *_windows(rng, m, False, **kw)) for m in chain_lengths] + [("ring", *_windows(rng, m, True, **kw)) for m in ring_lengths]
    n = sum(len(w) for _, w, _ in groups)
    extra = [_seq(rng, i % 2) for i in range(max(4, n // 40))]       # empty and one-base targets between them
    t, groups = _shuffled(rng, groups, extra)
    return t, groups


def _chains():
    """linear chains of CHAIN_LENGTHS and rings of RING_LENGTHS windows of 120 to 169 bases with overlaps of 42 to 59, each from a genome of its
    own, all windows shuffled into one id order and half of them reverse complemented; empty and one-base targets in between.  Variant 1 is the
    first round of the two-round test: at max_overlap 50 the joins of longer overlaps are left to the second round"""
    t, groups = _chains_of(SEEDS["chains"], CHAIN_LENGTHS, RING_LENGTHS)
    return _make(t, [dict(), dict(max_overlap=50)], groups=groups)


def _chains_small():
    """the same generator at chains of SMALL_CHAINS and a ring of SMALL_RINGS: what the quadratic statement can take"""
    t, groups = _chains_of(SEEDS["chains_small"], SMALL_CHAINS, SMALL_RINGS)
    return _make(t, [dict(), dict(max_overlap=50)], groups=groups)


MISMATCH_CHAINS = tuple(range(3, 41))                                # 817 windows: more than three blocks of contigs
SMALL_MISMATCH_CHAINS = (3, 4, 5, 7, 9, 13, 18, 40)                  # the reduced draw for the quadratic statement: 99 windows


def _mismatch_chains_of(seed, lengths):
    rng = np.random.default_rng(seed)
    groups, planted = [], []
    for c, m in enumerate(lengths):
        half = () if m < 5 else (2,) if m < 9 else (2, 5)
        w, o = _windows(rng, m, False, half=half)
        for i in range(m - 1):
            if (i + c) % 2:
                continue
            col = (0, o[i] // 2, o[i] - 1)[int(rng.integers(0, 3))]
            later = int(rng.integers(0, 2))
            if later:
                w[i + 1] = _sub(w[i + 1], [col])
            else:
                w[i] = _sub(w[i], [len(w[i]) - o[i] + col])
            planted.append((c, i, o[i], col, later))
        groups.append(("chain", w, o))
    t, groups = _shuffled(rng, groups, [_seq(rng, 0), _seq(rng, 1)])
    made = [(groups[c][1][i], groups[c][1][i + 1], o, col, later) for c, i, o, col, later in planted]
    return _make(t, [dict(), dict(max_mismatches=0)], groups=groups, made=made, lengths=lengths)


def _chain_mismatches():
    """chains of 3 to 40 windows in which about every second overlap carries exactly one substitution, in the later or in the earlier window, in
    the first, a middle or the last overlap column; in every chain of five or more, windows 2 and (from nine on) 5 are o_left + o_right long
    exactly.  made: [(id of the earlier window, id of the later, o, column, which window is changed)].  Variant 1 (max_mismatches 0) breaks the
    chains at those joins"""
    return _mismatch_chains_of(SEEDS["chain_mismatches"], MISMATCH_CHAINS)


def _chain_mismatches_small():
    """the same generator at SMALL_MISMATCH_CHAINS: what the quadratic statement can take"""
    return _mismatch_chains_of(SEEDS["chain_mismatches_small"], SMALL_MISMATCH_CHAINS)


TANDEM_PERIODS = (2, 3, 5, 7, 10, 13, 21, 30)
AT_ENDS = 6


def _repeats():
    """Ends that repeat.
    two_letter: three chains of four windows of 300 to 399 bases over {A, T}, overlaps of 60 to 99: at k = 8 every seed of such an end has many
        occurrences, nearly all of them at loci that do not verify.
    tandem: per period p of TANDEM_PERIODS a pair of targets, the right end of the first and the left end of the second 96 bases of one period-p
        repeat (the period ends there): an overlap at every multiple of p, one partner, the longest wins.
    duplicates: an end U of 90 bases at the right of target a and at the left of b, c and d -- in b with one substitution, in c and d exact, so
        that a's end chooses c: by mm before b, by y before d; b, c and d each choose a.  A second such group with two substitutions in b (out of
        reach at max_mismatches 1) and exact copies in c and d.  Every U holds one 16-mer R that all of them share: the seeds inside it are over a
        small max_occ, the overlap is found through the others.
    shared: four pairs that overlap by 70 bases with R inside the overlap: R lies in 16 ends, over the max_occ 4 of the last variant, and the pairs join
        through their other seeds.
    at_ends: AT_ENDS targets of 600 random bases and 512 of the repeat AT, three of them reverse complemented: at min_overlap 8, k = 8 and
        max_mismatches 0 every such end has (512 - 8) / 2 + 1 overlaps with each of the five others -- hits saturates at 255.
    made: the id of the first target of each part"""
    rng = np.random.default_rng(SEEDS["repeats"])
    t, made = [], {}
    made["two_letter"] = len(t)
    for _ in range(3):
        w, _o = _windows(rng, 4, False, n_range=(300, 400), o_range=(60, 100), alphabet=2)
        t += [P.revcomp(s) if rng.integers(0, 2) else s for s in w]
    made["tandem"] = len(t)
    for p in TANDEM_PERIODS:
        while True:
            unit = _seq(rng, p)
            if not any((np.roll(unit, s) == unit).all() for s in range(1, p)):
                break
        u = np.tile(unit, 96 // p + 1)[:96]
        while True:
            a, b = np.concatenate([_seq(rng, 150), u]), np.concatenate([u, _seq(rng, 140)])
            if a[149] != unit[p - 1] and b[96] != unit[96 % p]:          # the period ends there
                break
        t += [a, P.revcomp(b)] if p % 2 else [a, b]
    made["duplicates"] = len(t)
    R = _seq(rng, 16)
    for subs in (1, 2):
        U = _seq(rng, 90)
        U[40:56] = R
        a = np.concatenate([_seq(rng, 130), U])
        b = np.concatenate([_sub(U, [20, 70][:subs]), _seq(rng, 120)])
        c = np.concatenate([U, _seq(rng, 125)])
        d = np.concatenate([U, _seq(rng, 135)])
        t += [a, b, P.revcomp(c), d]
    made["shared"] = len(t)
    for i in range(4):                                               # further copies of R: four pairs that overlap by 70, R in the overlap
        g = _seq(rng, 330)
        g[150 + 7 * i:166 + 7 * i] = R
        t += [g[:200], g[130:]] if i % 2 else [P.revcomp(g[130:]), P.revcomp(g[:200])]
    made["at_ends"] = len(t)
    for i in range(AT_ENDS):
        s = np.concatenate([_seq(rng, 600), np.tile(np.array([0, 3], np.uint8), 256)])
        t.append(P.revcomp(s) if i % 2 else s)
    made["n"] = len(t)
    return _make(t, [dict(k=8), dict(k=12), dict(), dict(k=8, max_occ=65535, max_mismatches=0, min_overlap=8, max_overlap=512), dict(k=8, max_occ=4)], made=made)


EDGE_BOUNDS = (42, 41, 512, 513)                                     # min_overlap, min_overlap - 1, max_overlap, max_overlap + 1
EDGE_RESIDUES = tuple(range(43, 64))                                 # o mod 16 over all residues; o mod k in 0, 1, k - 1 for k = 8, 21 and 31
EDGE_MISMATCH_O, EDGE_MISMATCH_COLUMNS = 100, (2, 50, 70, 90, 98)    # the first seed, a middle one, the last whole seed at k = 21 / 31 and at k = 8, the tail
EDGE_TINY = 45


def _edges():
    """pairs of targets from genomes of their own.  bounds: o of EDGE_BOUNDS in the four end pairings (the targets of the two long ones have ends of
    512 bases: 64 seeds at k = 8).  residues: o of EDGE_RESIDUES, the pairing changing.  mismatches: o = 100 with one substitution in column c of
    EDGE_MISMATCH_COLUMNS (column c of one end is column 99 - c of the other: the first seed of one is the tail of the other).  tiny: EDGE_TINY
    targets of 1 to 15 bases side by side, each a merged contig of its own.  pairs: [(part, id of the first target, o, pairing, column)]"""
    rng = np.random.default_rng(SEEDS["edges"])
    t, pairs = [], []
    for o in EDGE_BOUNDS:
        for i, pr in enumerate(PAIRINGS):
            la, lb = (1100 + 16 * i, 1060 + 8 * i) if o > 100 else (100 + 7 * i, 131 - 5 * i)
            pairs.append(("bounds", len(t), o, pr, -1))
            t += _pair(rng, la, lb, o, pr)
    for i in range(EDGE_TINY // 3):
        t.append(_seq(rng, 1 + i % 15))
    for i, o in enumerate(EDGE_RESIDUES):
        pairs.append(("residues", len(t), o, PAIRINGS[i % 4], -1))
        t += _pair(rng, 140 + i, 150 - i, o, PAIRINGS[i % 4])
    for i in range(EDGE_TINY // 3, 2 * (EDGE_TINY // 3)):
        t.append(_seq(rng, 1 + (7 * i) % 15))
    for i, col in enumerate(EDGE_MISMATCH_COLUMNS):
        pairs.append(("mismatches", len(t), EDGE_MISMATCH_O, PAIRINGS[i % 4], col))
        t += _pair(rng, 230 + i, 240 - i, EDGE_MISMATCH_O, PAIRINGS[i % 4], sub=[col])
    for i in range(2 * (EDGE_TINY // 3), EDGE_TINY):
        t.append(_seq(rng, 1 + (4 * i) % 15))
    return _make(t, [dict(k=8), dict(), dict(k=31)], pairs=pairs)


LONG_CHAINS = (5, 120, 9, 64, 33, 100, 17, 80, 2, 110, 48, 90, 70, 60, 101, 75, 40, 115, 95, 66)   # 1 300 windows; the longest merged contig stays below half a chunk


def _long_windows():
    """chains of LONG_CHAINS windows of 1 800 to 2 199 bases, overlaps of 42 to 512: more than 2 * 2^20 columns after the merge, so the merged
    FASTA takes three chunks of 1 MiB or more.  Only the ends are indexed"""
    rng = np.random.default_rng(SEEDS["long_windows"])
    t, groups = _shuffled(rng, [("chain", *_windows(rng, m, False, n_range=(1800, 2200), o_range=(42, 513))) for m in LONG_CHAINS])
    return _make(t, [dict()], groups=groups)


CASES = {"chains": _chains, "chains_small": _chains_small, "chain_mismatches": _chain_mismatches, "chain_mismatches_small": _chain_mismatches_small,
         "repeats": _repeats, "edges": _edges, "long_windows": _long_windows}
GPU_FAMILIES = ("chains", "chain_mismatches", "repeats", "edges", "long_windows")      # (the *_small cases are the quadratic statement's draws)
# the case the quadratic statement runs on
BRUTE = {"chains": "chains_small", "chain_mismatches": "chain_mismatches_small", "repeats": "repeats", "edges": "edges"}


@functools.lru_cache(maxsize=None)
def second_round(name, i):
    """(the case whose targets are the merged contigs of variant i, the checker's result on it at the defaults)"""
    c2 = next_round(checked(name, i))
    return c2, MC.merge_index(c2["seqs"])


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _checked(name, i):
    c = case(name)
    return MC.merge_index(c["seqs"], **c["variants"][i])


def checked(name, i=0):
    return _checked(name, i)                                         # (one cache entry whether i is given or not)


@functools.lru_cache(maxsize=None)
def fasta(name, i=0):
    """the checker's merged FASTA of variant i, rendered once"""
    return MC.fasta(checked(name, i))


def every(names=None):
    return [(n, i) for n in sorted(names or CASES) for i in range(len(case(n)["variants"]))]


def first_difference(got, want):
    """(array, index, got, want) of the first entry of the first array of the checker's that differs, then the first counter, or None"""
    for k in MC.ARRAYS:
        if got[k].shape != want[k].shape:
            return k, "shape", got[k].shape, want[k].shape
        d = np.nonzero(got[k] != want[k])[0]
        if len(d):
            return k, int(d[0]), got[k][d[0]], want[k][d[0]]
    for k in MC.COUNTERS:
        if got["info"][k] != want["info"][k]:
            return "info", k, got["info"][k], want["info"][k]
    return None


def ends_of(seqs, max_overlap):
    """E_x of every end: the last W bases of the target, or the reverse complement of the first W"""
    out = []
    for s in seqs:
        W = min(len(s) >> 1, max_overlap)
        out += [P.revcomp(s[:W]), s[len(s) - W:]]
    return out


def found_at(seqs, x, **params):
    """every (mm, y, o) of end x by the definition, for one end: each y and o, the Hamming distance, then whether a usable seed of P_x lies whole
    and exact in the overlap; and the number of usable (seed, occurrence) pairs of the end"""
    p = dict(MC.DEFAULT, **params)
    k = p["k"]
    E = ends_of(seqs, p["max_overlap"])
    occ = {}
    for e in E:
        for v in P.kmer_values(e, k):
            occ[int(v)] = occ.get(int(v), 0) + 1
    Px = P.revcomp(E[x])
    n = [occ.get(int(v), 0) for v in P.kmer_values(Px, k)[::k]] if len(Px) >= p["min_overlap"] else []
    usable = [1 <= c <= p["max_occ"] for c in n]
    found = []
    for y in range(len(E)):
        if y >> 1 == x >> 1 or not usable:
            continue
        for o in range(p["min_overlap"], min(len(Px), len(E[y])) + 1):
            diff = Px[:o] != E[y][len(E[y]) - o:]
            if int(diff.sum()) <= p["max_mismatches"] and any(usable[j] and not diff[j * k:j * k + k].any() for j in range(o // k)):
                found.append((int(diff.sum()), y, o))
    return found, sum(c for c, u in zip(n, usable) if u), n
