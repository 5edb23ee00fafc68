"""Seeded cases of the read placement (tests/place_checker.py is the definition): the smallest shapes at which the kernels can go wrong.
case(name) -> dict(rows, lens, pair_off | None, twords, tbegin, tlen, params); checked(name) -> the checker's result, computed once."""
import functools

import numpy as np

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


def _make(reads, targets, shifts=None, gaps=None, pair_off=None, stride=None, **params):
    rows, lens = P.nodes_of(reads, stride)
    twords, tbegin, tlen = P.ragged(targets, shifts if shifts is not None else [3 * i % 16 for i in range(len(targets))], gaps)
    if pair_off is not None:
        pair_off = np.asarray(pair_off, dtype=np.uint8)
        assert len(pair_off) == len(lens)
    return dict(rows=rows, lens=lens, pair_off=pair_off, twords=twords, tbegin=tbegin, tlen=tlen, params=params)


def _exact():
    rng = _rng(1)
    t = _seq(rng, 600)
    reads = [t[p:p + 100] for p in range(0, 501, 50)] + [P.revcomp(t[p:p + 100]) for p in range(0, 501, 50)]
    return _make(reads, [t])


def _bound():
    rng = _rng(2)
    t = _seq(rng, 500)
    r = t[200:300]                       # seeds 0-20, 21-41, 42-62, 63-83; 84 .. 99 lie in no seed
    reads = [_sub(r, [30, 85, 90, 95]), _sub(r, [30, 85, 88, 90, 95]), P.revcomp(_sub(r, [30, 85, 90, 95])), P.revcomp(_sub(r, [30, 85, 88, 90, 95])),
             _sub(r, [84, 99]), r]
    return _make(reads, [t])


def _last_seed_only():
    rng = _rng(3)
    t = _seq(rng, 400)
    r = t[120:220]
    return _make([_sub(r, [5, 25, 50]), P.revcomp(_sub(r, [5, 25, 50])), _sub(r, [20, 41, 62])], [t])


def _every_seed_hit():
    rng = _rng(4)
    t = _seq(rng, 400)
    r = t[100:200]                       # S = 4 <= max_mismatches = 4
    return _make([_sub(r, [0, 21, 42, 63]), _sub(r, [10, 30, 50, 83]), P.revcomp(_sub(r, [10, 30, 50, 83])), _sub(r, [10, 30, 50])], [t])


def _ends():
    rng = _rng(5)
    a, b, c = _seq(rng, 300), _seq(rng, 300), _seq(rng, 203)
    x = _seq(rng, 1)
    reads = [a[:100], a[200:], b[:100], b[200:], c[:100], c[103:], P.revcomp(a[:100]), P.revcomp(b[200:]),
             np.concatenate([x, a[:99]]), np.concatenate([a[201:], x]), np.concatenate([x, b[:99]]), np.concatenate([c[104:], x]),
             np.concatenate([a[250:], b[:50]]), P.revcomp(np.concatenate([a[250:], b[:50]])), np.concatenate([b[240:], c[:60]])]
    # b lies directly behind a, c directly behind b: a begins at base 16 + 5, so the seams are at bases 321 and 621 (5 and 13 mod 16)
    return _make(reads, [a, b, c], shifts=[5, 0, 0], gaps=[True, False, False])


def _unaligned():
    rng = _rng(6)
    targets = [_seq(rng, n) for n in (260, 301, 333, 256, 417)] + [_seq(rng, 10), _seq(rng, 1500)]
    reads = []
    for i, L in enumerate((31, 32, 33, 63, 64, 65, 150, 151)):
        for j, t in enumerate(targets[:5]):
            p = int(rng.integers(0, len(t) - L + 1))
            r = _sub(t[p:p + L], rng.integers(0, L, size=(i + j) % 3))
            reads.append(P.revcomp(r) if (i + j) & 1 else r)
    big = targets[6][211:1311]           # 1100 nt: 69 words, 52 seeds
    reads += [_sub(big, [0, 600, 1099]), P.revcomp(big), None, np.zeros(0, np.uint8), targets[0][:K - 1], targets[5]]
    return _make(reads, targets, shifts=[0, 1, 15, 0, 1, 7, 9], gaps=[True, True, True, True, True, True, True])


def _repeat():
    rng = _rng(7)
    seg, unit, x, y = _seq(rng, 300), _seq(rng, 60), _seq(rng, 42), _seq(rng, 42)
    xf, yf = [_seq(rng, 21) for _ in range(4)], [_seq(rng, 21) for _ in range(5)]
    t0 = np.concatenate([_seq(rng, 150), seg, _seq(rng, 100), unit, unit, unit, _seq(rng, 80)])
    t1 = np.concatenate([_seq(rng, 90), seg, _seq(rng, 120)] + [np.concatenate([x, f, _seq(rng, 30)]) for f in xf] + [np.concatenate([y, f, _seq(rng, 30)]) for f in yf])
    reads = [seg[100:200], P.revcomp(seg[50:190]), unit, np.concatenate([unit, unit]), np.concatenate([x, xf[1]]), np.concatenate([y, yf[2]]), y, x,
             P.revcomp(np.concatenate([y, yf[4]])), t0[100:200], _sub(seg[20:150], [64])]
    return _make(reads, [t0, t1], max_occ=4)


def _palindrome():
    rng = _rng(8)
    h = _seq(rng, 50)
    pal = np.concatenate([h, P.revcomp(h)])
    assert (P.revcomp(pal) == pal).all()
    t = np.concatenate([_seq(rng, 77), pal, _seq(rng, 90)])
    return _make([pal, t[60:160]], [t])


def _saturate():
    # 301 `+` placements of the poly-A read (its reverse complement, poly-T, has none); the poly-C read has none on either strand
    return _make([np.zeros(100, np.uint8), np.full(100, 1, np.uint8)], [np.zeros(400, np.uint8)], max_occ=1000)


def _pairs():
    rng = _rng(9)
    seg = _seq(rng, 300)
    t0 = np.concatenate([_seq(rng, 2000), seg, _seq(rng, 700)])
    t1 = np.concatenate([_seq(rng, 500), seg, _seq(rng, 200)])
    fw = lambda t, a, n=100: t[a:a + n]
    rc = lambda t, a, n=100: P.revcomp(t[a:a + n])
    pairs = []
    for i, ins in enumerate((200, 230, 251, 251, 300, 333, 380, 399)):          # proper, either mate first, lengths 100 / 90
        a = 50 + 150 * i
        m1, m2 = fw(t0, a), rc(t0, a + ins - 90, 90)
        pairs.append((m1, m2) if i & 1 else (m2, m1))
    pairs += [(rc(t0, 100), fw(t0, 300)),                                        # - left of +
              (fw(t0, 100), fw(t0, 300)), (rc(t0, 100), rc(t0, 300)),            # same strand
              (fw(t0, 400), rc(t1, 100)),                                        # split over two targets
              (fw(t0, 500), _seq(rng, 100)),                                     # an unplaced mate
              (fw(t0, 600), rc(seg, 100)),                                       # a MULTI mate
              (fw(t0, 1000), rc(t0, 1300)), (fw(t0, 1000), rc(t0, 1301)),        # insert 400 = max_insert, 401
              (fw(t0, 1200, 150), rc(t0, 1220, 100))]                            # the - read ends inside the + read: a + la > b + lb
    reads, po = [], []
    for m1, m2 in pairs:
        reads += [m1, m2]
        po += [1, 1, 2, 2]
    reads.append(fw(t0, 50))                                                     # an unpaired read behind the pairs
    po += [0, 0]
    return _make(reads, [t0, t1], pair_off=po, max_insert=400)


def _rand(n_reads=1500):
    rng = _rng(10)
    g = _seq(rng, 5000)
    g[2400:2800] = g[200:600]
    targets = [g[:1700], g[1700:3400], g[3400:]]
    reads, po = [], []
    for _ in range(n_reads // 2):
        ins = int(rng.integers(200, 501))
        a = int(rng.integers(0, len(g) - ins + 1))
        l1, l2 = int(rng.integers(100, 151)), int(rng.integers(100, 151))
        m1, m2 = g[a:a + l1].copy(), P.revcomp(g[a + ins - l2:a + ins])
        for m in (m1, m2):
            e = rng.random(len(m)) < 0.01
            m[e] = (m[e] + rng.integers(1, 4, size=int(e.sum()))) & 3
        if rng.random() < 0.5:
            m1, m2 = m2, m1
        reads += [m1.astype(np.uint8), m2.astype(np.uint8)]
        po += [1, 1, 2, 2]
    return _make(reads, targets, shifts=[11, 6, 14], pair_off=po)


def _empty_targets():
    rng = _rng(11)
    return _make([_seq(rng, 100), _seq(rng, 50)], [], pair_off=[1, 1, 2, 2])


def _empty_reads():
    rng = _rng(12)
    return _make([], [_seq(rng, 200), _seq(rng, 90)])


def _empty_short():
    rng = _rng(13)
    t = [_seq(rng, 20), _seq(rng, 5), _seq(rng, 0), _seq(rng, 19)]
    return _make([np.concatenate(t), t[0]], t, shifts=[0, 0, 0, 0], gaps=[True, False, False, False])


def _mid(a, b):
    """one substitution in the middle of each of the seeds a .. b - 1 (k = 21)"""
    return [K * j + 10 for j in range(a, b)]


def _many_seeds_parts():
    rng = _rng(14)
    X, W = _seq(rng, 2800), _seq(rng, 2800)
    W[:1344] = 0                         # seeds 0 .. 63 of W are the poly-A 21-mer: 1324 occurrences, over max_occ
    t0 = np.concatenate([_seq(rng, 137), X, _seq(rng, 211)])
    t1 = np.concatenate([_seq(rng, 55), _sub(X, [1500, 2000, 2500]), _seq(rng, 19)])
    t2 = np.concatenate([_seq(rng, 80), W, _seq(rng, 90)])
    return X, W, [t0, t1, t2]


def _many_seeds():
    # 133 seeds: three chunks of 64 in k_pl_place.  Read 1 is found only from chunk 1, read 2 only from chunk 2 (its last five seeds), read 4 from
    # no seed; read 5 through chunk 1 while all of chunk 0 matches and is over max_occ; reads 7 .. 10 (65, 64, 64, 65 seeds) lie on t0 and t1 at
    # equal mm through one seed each: exactly two placements
    X, W, targets = _many_seeds_parts()
    r2, r7 = _sub(X, _mid(0, 128)), _sub(X[100:1465], _mid(0, 64))
    reads = [X, _sub(X, _mid(0, 64)), r2, P.revcomp(r2), _sub(X, _mid(0, 133)), W, P.revcomp(W), r7, _sub(X[100:1464], _mid(0, 63)),
             _sub(X[100:1444], _mid(1, 64)), P.revcomp(r7), _sub(targets[1][55:2855], _mid(0, 64))]
    return _make(reads, targets, shifts=[3, 9, 14], max_mismatches=140, max_occ=8)


def _mm_limit():
    # the uint8 mm and the mm << 33 of the key at their limit: 254 substitutions (none in seed 0) are placed, 255 are not
    X, _, targets = _many_seeds_parts()
    at = [K + 10 * i for i in range(255)]
    return _make([_sub(X, at[:254]), _sub(X, at), P.revcomp(_sub(X, at[:254]))], targets[:1], shifts=[3], max_mismatches=254, max_occ=8)


TINY_LENS = [0, 21, 22, 37, 0, 0, 64, 65, 16, 100, 5, 48, 0, 20, 129, 1, 63, 0, 33]


def _tiny_targets():
    # 150 targets, 39 of them empty: several seams inside one word of k_pl_gather, one wave of k_pl_uncovered, and equal offsets in item_of
    rng = _rng(15)
    targets = [_seq(rng, TINY_LENS[i % 19]) for i in range(150)]
    reads = []
    for i, t in enumerate(targets):
        if len(t) >= K and i % 3 != 2:
            reads.append(P.revcomp(t) if i & 1 else t)
        if len(t) >= 40 and i % 2 == 0:
            reads.append(t[-25:])
        if len(t) >= 60 and i % 4 == 1:
            reads.append(_sub(t[3:40], [30]))
    return _make(reads, targets, shifts=[5 * i % 16 for i in range(150)], gaps=[i % 4 != 1 for i in range(150)])


SEAM_LENS = [1, 15, 16, 17, 0, 31, 32, 33, 4100]


def _word_seams():
    # k_pl_gather at its seams: targets that end 1 base before, at and 1 base behind a word boundary, an empty one between them, 4245 columns in all
    # (no multiple of 16: the last word is partial; 266 words: more than one block of 256 lanes).  k = 8, so that every target of 15 bases or more is
    # the whole of a read in one orientation or the other, and the long one is read across every boundary of 256 columns
    rng = _rng(19)
    targets = [_seq(rng, n) for n in SEAM_LENS]
    reads = [P.revcomp(t) if i & 1 else t for i, t in enumerate(targets[:-1]) if len(t) >= 15]
    reads += [targets[-1][p - 20:p + 20] for p in range(256, 4100, 256)] + [targets[-1][:30], P.revcomp(targets[-1][-30:])]
    return _make(reads, targets, shifts=[7 * i % 16 for i in range(len(targets))], gaps=[i % 2 == 0 for i in range(len(targets))], k=8)


CASES = {"word_seams": _word_seams, "exact": _exact, "bound": _bound, "last_seed_only": _last_seed_only, "every_seed_hit": _every_seed_hit, "ends": _ends, "unaligned": _unaligned,
         "repeat": _repeat, "palindrome": _palindrome, "saturate": _saturate, "pairs": _pairs, "rand": _rand, "empty_targets": _empty_targets,
         "empty_reads": _empty_reads, "empty_short": _empty_short, "many_seeds": _many_seeds, "mm_limit": _mm_limit, "tiny_targets": _tiny_targets}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def rand_cut():
    """the first 200 reads of `rand`"""
    c = dict(case("rand"))
    c.update(rows=c["rows"][:400], lens=c["lens"][:400], pair_off=c["pair_off"][:400])
    return c


@functools.lru_cache(maxsize=None)
def many_reads(n):
    """n short reads (21 .. 48 nt) on four targets, one of them empty, behind eight 1400-nt reads (67 seeds: the usable masks of two chunks stay
    in the scratch of the waves that take a short read next); consecutive reads are mates.  Not in CASES: the GPU test sizes n by the device,
    so that a wave of k_pl_place takes more than one read"""
    assert n % 2 == 0 and n >= 8
    rng = _rng(16)
    targets = [_seq(rng, 700), _seq(rng, 0), _seq(rng, 333), _seq(rng, 1200), _seq(rng, 1600)]
    reads = []
    for i in range(n):
        if i < 8:
            p = int(rng.integers(0, 201))
            r = targets[4][p:p + 1400]
        else:
            t = targets[(0, 2, 3)[i % 3]]
            L = int(rng.integers(21, 49))
            p = int(rng.integers(0, len(t) - L + 1))
            r = t[p:p + L]
            if i % 5 == 0:
                r = _sub(r, [int(rng.integers(0, L))])
            if i % 7 == 0:
                r = _seq(rng, L)
        reads.append(P.revcomp(r) if i & 1 else r)
    return _make(reads, targets, shifts=[3, 0, 9, 14, 6], pair_off=[1, 1, 2, 2] * (n // 2))


HEADER_LENS = [21, 40, 64, 99, 100, 333, 1000, 1200, 50, 75, 150, 480, 999, 1001]
HEADER_ENDS = {1000: "_reads=11_depth=1.05", 40: "_reads=120_depth=120.00", 1200: "_reads=1000_depth=", 333: "_reads=11_depth=10.30", 1001: "_reads=1_depth=0.04",
               99: "_reads=1_depth=0.33", 21: "_reads=1_depth=1.00", 480: "_reads=3_depth=0.56",
               999: "_reads=0_depth=0.00", 150: "_reads=0_depth=0.00", 100: "_reads=0_depth=0.00", 75: "_reads=0_depth=0.00", 64: "_reads=0_depth=0.00", 50: "_reads=0_depth=0.00"}


def header_nodes():
    """one random read of every length in HEADER_LENS: without edges each becomes a contig of its own, numbered by descending length"""
    rng = _rng(17)
    return P.nodes_of([_seq(rng, n) for n in HEADER_LENS])


def header_reads(contigs):
    """reads for the depth headers of contigs with the lengths of HEADER_LENS (code arrays, any order): every width of id, length, reads and
    depth the device formats, HEADER_ENDS by length"""
    rng = _rng(18)
    by = {len(c): c for c in contigs}
    assert sorted(by) == sorted(HEADER_LENS)
    c = by[1000]
    reads = [c[p:p + 100] for p in range(0, 1000, 100)] + [c[475:525]]          # 1050 bases: 1.05, the leading zero of dd
    reads += [by[40]] * 120                                                       # 120.00: q >= 100
    for _ in range(1000):                                                         # four-digit reads
        L = int(rng.integers(21, 61))
        a = int(rng.integers(0, 1200 - L + 1))
        reads.append(by[1200][a:a + L])
    reads += [by[333]] * 10 + [by[333][200:300]]                                  # 3430 bases: 10.30
    reads += [by[1001][900:950], by[99][50:83], by[21]]                           # 0.04, 0.33, 1.00
    reads += [P.revcomp(by[480][a:a + 90]) for a in (0, 100, 390)]                # the minus strand only: 270 bases, 0.56
    return reads                                                                  # 999, 150, 100, 75, 64, 50: no read


def args(c):
    return c["rows"], c["lens"], c["pair_off"], c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def checked(name, flags=0):
    c = case(name)
    return P.place(*args(c), flags=flags, **c["params"])
