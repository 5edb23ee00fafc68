"""Seeded cases of the scaffolds (tests/scaffold_checker.py is the definition), built on the placement's checker: the smallest shapes at which
the kernels can go wrong.  The targets are random, so every read has one placement; the reads are cut from the targets without an error at
planted reaches, so the links are known.  case(name) -> dict(rows, lens, pair_off, twords, tbegin, tlen, params (of the placement), seqs (the
targets as code arrays), variants (a list of scaffold parameters, `insert` among them)); placed(name) -> the checker's placement;
checked(name, i) -> the scaffold checker's result for variant i, computed once."""
import functools

import numpy as np

import place_cases as PC
import place_checker as P
import scaffold_checker as SC

_rng, _seq = PC._rng, PC._seq
READ = 25                                                          # one seed of 21 and four bases
DEFAULT = dict(insert=300, **SC.DEFAULT)
L, R = 0, 1                                                        # the ends of a target: x = 2t + e


def mate(targets, x, d, n=READ):
    """the read of n bases that lies on target x >> 1, points out of end x & 1 and reaches d bases to it"""
    t = targets[x >> 1]
    assert n <= d <= len(t), (x, d, len(t))
    return t[len(t) - d:len(t) - d + n] if x & 1 else P.revcomp(t[d - n:d])


def _make(targets, links, shifts=None, gaps=None, variants=(), paired=True, extra=(), **params):
    """links: (end, reach, end, reach) per pair, the first two of the mate with the smaller index"""
    reads = []
    for x1, d1, x2, d2 in links:
        reads += [mate(targets, x1, d1), mate(targets, x2, d2)]
    pair_off = np.array([1, 1, 2, 2] * len(links) + [0, 0] * len(extra), dtype=np.uint8) if paired else None
    c = PC._make(reads + list(extra), targets, shifts=shifts, gaps=gaps, pair_off=pair_off, **params)
    return dict(c, seqs=[np.asarray(t, np.uint8) for t in targets], links=list(links), variants=[dict(DEFAULT, **v) for v in (variants or ({},))])


def bundle(rng, targets, x, y, n, lo=READ, hi=None):
    """n links between the ends x and y with reaches lo .. hi (at most the target's length), the judging mate on x or y in turn"""
    out = []
    for i in range(n):
        dx = int(rng.integers(lo, min(hi or 10 ** 9, len(targets[x >> 1])) + 1))
        dy = int(rng.integers(lo, min(hi or 10 ** 9, len(targets[y >> 1])) + 1))
        out.append((x, dx, y, dy) if i & 1 else (y, dy, x, dx))
    return out


def _two():
    rng = _rng(201)
    tg = [_seq(rng, 200), _seq(rng, 180)]
    return _make(tg, bundle(rng, tg, 2 * 0 + R, 2 * 1 + L, 5, hi=120), variants=({}, dict(min_links=6), dict(min_links=1)))


ORIENT_CHAIN = [(0, 0), (1, 0), (2, 1), (3, 0), (4, 1), (5, 1)]      # (contig, orient): R-L, R-R, L-L, R-R, L-R


def chain_links(rng, targets, chain, n, hi=None):
    links = []
    for (c, o), (d, q) in zip(chain, chain[1:]):
        links += bundle(rng, targets, 2 * c + (o ^ 1), 2 * d + q, n, hi=hi)
    return links


def _orient():
    rng = _rng(202)
    tg = [_seq(rng, n) for n in (150, 90, 121, 64, 200, 77)]
    return _make(tg, chain_links(rng, tg, ORIENT_CHAIN, 6, hi=60), variants=({}, dict(insert=100)))


def _ambiguous():
    rng = _rng(203)
    tg = [_seq(rng, 160) for _ in range(6)]
    links = bundle(rng, tg, 2 * 0 + R, 2 * 1 + L, 10, hi=100) + bundle(rng, tg, 2 * 0 + R, 2 * 2 + L, 5, hi=100) + \
        bundle(rng, tg, 2 * 3 + R, 2 * 4 + L, 10, hi=100) + bundle(rng, tg, 2 * 3 + R, 2 * 5 + L, 4, hi=100)
    return _make(tg, links, variants=(dict(min_links=3), dict(min_links=3, max_second_percent=40), dict(min_links=3, max_second_percent=51), dict(min_links=5)))


def _tie():
    rng = _rng(204)
    tg = [_seq(rng, 140) for _ in range(6)]
    links = bundle(rng, tg, 2 * 0 + R, 2 * 2 + L, 6, hi=90) + bundle(rng, tg, 2 * 0 + R, 2 * 1 + R, 6, hi=90) + \
        bundle(rng, tg, 2 * 3 + R, 2 * 4 + L, 6, hi=90) + bundle(rng, tg, 2 * 3 + R, 2 * 5 + L, 5, hi=90)
    return _make(tg, links, variants=(dict(max_second_percent=100), dict(max_second_percent=100, min_links=6), dict(max_second_percent=100, min_links=7), {}))


def _mutual():
    rng = _rng(205)
    tg = [_seq(rng, 150) for _ in range(3)]
    return _make(tg, bundle(rng, tg, 2 * 0 + R, 2 * 1 + L, 5, hi=100) + bundle(rng, tg, 2 * 2 + R, 2 * 1 + L, 12, hi=100))


def _ring3():
    rng = _rng(206)
    tg = [_seq(rng, 130) for _ in range(5)]
    links = bundle(rng, tg, 2 * 1 + R, 2 * 4 + L, 6, hi=80) + bundle(rng, tg, 2 * 4 + R, 2 * 3 + R, 7, hi=80) + bundle(rng, tg, 2 * 3 + L, 2 * 1 + L, 8, hi=80) + \
        bundle(rng, tg, 2 * 0 + R, 2 * 2 + L, 5, hi=80)
    return _make(tg, links)


def _ring2():
    rng = _rng(207)
    tg = [_seq(rng, 170), _seq(rng, 110), _seq(rng, 140)]
    return _make(tg, bundle(rng, tg, 2 * 2 + R, 2 * 1 + L, 6, hi=50) + bundle(rng, tg, 2 * 2 + L, 2 * 1 + R, 9, hi=50))


def _too_far():
    rng = _rng(208)
    tg = [_seq(rng, 400), _seq(rng, 400), _seq(rng, 400)]
    links = [(1, 150, 2, 150 - i) for i in range(5)] + [(2, 151, 1, 150)] * 2 + [(3, 200, 4, 101), (4, 100, 3, 200), (3, 199, 4, 100), (3, 30, 4, 30)]
    return _make(tg, links, variants=(dict(max_insert=300, min_links=3), dict(max_insert=301, min_links=3), dict(max_insert=299, min_links=3)))


def _neg_gap():
    rng = _rng(209)
    tg = [_seq(rng, 200) for _ in range(3)]
    links = [(1, 70 + i, 2, 80) for i in range(5)] + [(3, 45 + i, 4, 50 - i) for i in range(5)] + [(3, 46, 4, 50)]
    return _make(tg, links, variants=(dict(insert=100), dict(insert=100, min_gap=1), dict(insert=100, min_gap=60), dict(insert=0)))


LONG_N = 300


@functools.lru_cache(maxsize=None)
def long_chain_truth():
    """the chain of the case long_chain as (contig, orient) from its smaller terminal"""
    rng = _rng(210)
    ids = rng.permutation(LONG_N)
    chain = [(int(c), int(rng.integers(0, 2))) for c in ids]
    if chain[0][0] > chain[-1][0]:
        chain = [(c, o ^ 1) for c, o in chain[::-1]]
    return chain


def _long_chain():
    rng = _rng(211)
    tg = [_seq(rng, 30 + (37 * i + 11) % 100) for i in range(LONG_N)]
    return _make(tg, chain_links(rng, tg, long_chain_truth(), 5), shifts=[7 * i % 16 for i in range(LONG_N)], gaps=[i % 3 != 1 for i in range(LONG_N)],
                 variants=(dict(insert=120),))


def _big_bundle():
    rng = _rng(212)
    tg = [_seq(rng, 1500), _seq(rng, 1400)] + [_seq(rng, 60) for _ in range(24)]
    links = bundle(rng, tg, 2 * 0 + R, 2 * 1 + L, 3000, hi=480)
    singles = [(2 * (2 + i) + R, 30 + i, 2 * (3 + i) + L, 31) for i in range(0, 24, 2)] + [(2 * 0 + L, 40 + i, 2 * (2 + i) + L, 33) for i in range(12)]
    order = rng.permutation(len(links) + len(singles))
    both = links + singles
    return _make(tg, [both[i] for i in order], variants=(dict(insert=600), dict(insert=600, min_links=1)))


SEAM_LENS = (40, 0, 33, 0, 0, 61, 17, 129, 0, 25, 50, 0, 31, 1, 26)
SEAM_CHAIN = [(0, 1), (9, 0), (2, 0), (14, 1), (5, 0), (12, 1)]      # gaps of 1 .. 7 between contigs of 25 .. 61 bases


def _seams():
    rng = _rng(213)
    tg = [_seq(rng, n) for n in SEAM_LENS]
    links = chain_links(rng, tg, SEAM_CHAIN, 5, hi=25) + bundle(rng, tg, 2 * 7 + R, 2 * 10 + R, 5, hi=40)
    return _make(tg, links, shifts=[5 * i % 16 for i in range(len(tg))], gaps=[i % 4 != 1 for i in range(len(tg))],
                 variants=(dict(insert=53, min_gap=1), dict(insert=57, min_gap=7), dict(insert=50, min_gap=3)))


def _no_pairs():
    rng = _rng(214)
    tg = [_seq(rng, 150), _seq(rng, 0), _seq(rng, 150)]
    return _make(tg, bundle(rng, tg, 2 * 0 + R, 2 * 2 + L, 6), paired=False)


def _one_target():
    rng = _rng(215)
    t = _seq(rng, 600)
    tg = [t, _seq(rng, 100)]
    reads = []
    for a in range(0, 300, 30):
        reads += [t[a:a + READ], P.revcomp(t[a + 275:a + 300])]
    c = PC._make(reads, tg, pair_off=np.array([1, 1, 2, 2] * 10, dtype=np.uint8))
    return dict(c, seqs=tg, links=[], variants=[dict(DEFAULT)])


def _empty(reads, targets):
    def make():
        rng = _rng(216)
        tg = [_seq(rng, n) for n in targets]
        rd = [_seq(rng, 30) for _ in range(reads)]
        c = PC._make(rd, tg, pair_off=np.array([1, 1, 2, 2] * (reads // 2), dtype=np.uint8) if reads else None)
        return dict(c, seqs=tg, links=[], variants=[dict(DEFAULT)])
    return make


CASES = {"two": _two, "orient": _orient, "ambiguous": _ambiguous, "tie": _tie, "mutual": _mutual, "ring3": _ring3, "ring2": _ring2, "too_far": _too_far,
         "neg_gap": _neg_gap, "long_chain": _long_chain, "big_bundle": _big_bundle, "seams": _seams, "no_pairs": _no_pairs, "one_target": _one_target,
         "n0": _empty(0, (100, 0, 50)), "t0": _empty(4, ())}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def placed(name):
    c = case(name)
    return P.place(*PC.args(c), **c["params"])


def scaffold_args(c, pl):
    return c["rows"], c["lens"], c["pair_off"], pl


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return SC.scaffold_dicts(*scaffold_args(c, placed(name)), **c["variants"][i])


def every():
    """(name, variant index) of all cases"""
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


# ---- the planted genome: three contigs of a 4000-base genome, 1000 pairs with outer inserts of 300 .. 400 -------------------------------
PLANTED_SEED, PLANTED_PAIRS, PLANTED_ERR = 301, 1000, 0.01
PLANTED_TRUTH = [(1, 1), (0, 0), (2, 1)]                              # G[0:1200] is contig 2, revcomp(G[1260:2500]) contig 0, G[2580:4000] contig 1


@functools.lru_cache(maxsize=None)
def planted_genome(noisy=False):
    """-> the case dict (insert: the placement's median is the caller's to take) and the genome; noisy: 1 % substitutions in the reads"""
    rng = _rng(PLANTED_SEED)
    g = _seq(rng, 4000)
    tg = [P.revcomp(g[1260:2500]), g[2580:4000], g[0:1200]]
    reads = []
    for _ in range(PLANTED_PAIRS):
        ins = int(rng.integers(300, 401))
        a = int(rng.integers(0, 4000 - ins + 1))
        pair = [g[a:a + 100], P.revcomp(g[a + ins - 100:a + ins])]
        reads += pair if rng.integers(0, 2) else pair[::-1]
    if noisy:
        out = []
        for r in reads:
            r = r.copy()
            e = rng.random(len(r)) < PLANTED_ERR
            r[e] = (r[e] + rng.integers(1, 4, size=int(e.sum()))) & 3
            out.append(r)
        reads = out
    c = PC._make(reads, tg, pair_off=np.array([1, 1, 2, 2] * PLANTED_PAIRS, dtype=np.uint8))
    return dict(c, seqs=tg, links=[], variants=[dict(DEFAULT)]), g


# ---- more than 2 MB of scaffold records: the FASTA in several chunks --------------------------------------------------------------------
CHUNK_N, CHUNK_CHAINS = 36, ([(20, 0), (33, 1), (25, 0)], [(22, 1), (35, 0), (30, 1), (27, 1)])


@functools.lru_cache(maxsize=None)
def chunks():
    """36 targets of about 60 kb, joined only among the late ones (two chains with `-` contigs and gaps): with 1 MB chunks the joined scaffolds
    fall in the second chunk and later.  The placement checker is not run over 2 MB of targets: the reads are cut from random targets at
    known places, so the placement is written down (and the test compares the device's with it)
    -> the case dict, that placement in the checker's form"""
    rng = _rng(401)
    tg = [_seq(rng, 60000 + 7 * i) for i in range(CHUNK_N)]
    links = []
    for chain in CHUNK_CHAINS:
        links += chain_links(rng, tg, chain, 5, hi=200)
    c = _make(tg, links, shifts=[5 * i % 16 for i in range(CHUNK_N)], variants=(dict(insert=450),))
    ends = [(x, d) for x1, d1, x2, d2 in links for x, d in ((x1, d1), (x2, d2))]
    tlen = np.array([len(t) for t in tg], dtype=np.int64)
    pl = dict(target=np.array([x >> 1 for x, _ in ends], np.int32), pos=np.array([tlen[x >> 1] - d if x & 1 else d - READ for x, d in ends], np.int32),
              state=np.array([P.PLACED | P.UNIQUE | (0 if x & 1 else P.MINUS) for x, _ in ends], np.uint8),
              col_off=np.concatenate([[0], np.cumsum(tlen)]).astype(np.uint32))
    return c, pl
