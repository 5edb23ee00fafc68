"""Seeded cases of the break stage (tests/break_checker.py is the definition), built on the placement's checker: the smallest shapes at which
the kernels can go wrong.  The targets are random, so every read has one placement; the pairs are cut from the targets without an error
around known fragments, so the spans are known.  case(name) -> dict(rows, lens, pair_off, twords, tbegin, tlen, params (of the placement),
seqs (the targets as code arrays), variants (a list of break parameters, `margin` among them)); placed(name) -> the checker's placement;
checked(name, i) -> the break checker's result for variant i, computed once."""
import functools

import numpy as np

import break_checker as BC
import place_cases as PC
import place_checker as P

_rng, _seq = PC._rng, PC._seq
READ = 25                                                          # one seed of 21 and four bases
DEFAULT = dict(margin=30, min_span=1, inset=0)


def _make(targets, frags, shifts=None, gaps=None, variants=(), paired=True, extra=(), **params):
    """frags: (target, a, e) per pair: the `+` read is t[a : a + 25], the `-` read the reverse complement of t[e - 25 : e]; with inset 0 the
    pair spans columns a .. e - 1.  The judging mate is the `-` read in every second pair.  extra: (first read, second read, paired) to go behind them"""
    reads, po = [], []
    for i, (t, a, e) in enumerate(frags):
        assert 0 <= a and a + READ <= e <= len(targets[t]) and e - a <= 1000, (t, a, e)
        pair = [targets[t][a:a + READ], P.revcomp(targets[t][e - READ:e])]
        reads += pair[::-1] if i & 1 else pair
        po += [1, 1, 2, 2]
    for r1, r2, is_pair in extra:
        reads += [r1, r2]
        po += [1, 1, 2, 2] if is_pair else [0, 0, 0, 0]
    c = PC._make(reads, targets, shifts=shifts, gaps=gaps, pair_off=np.array(po, dtype=np.uint8) if paired else None, **params)
    return dict(c, seqs=[np.asarray(t, np.uint8) for t in targets], frags=list(frags), variants=[dict(DEFAULT, **v) for v in (variants or ({},))])


def cover(t, lo, hi, step=8, n=100):
    """fragments of n columns of target t, every `step` columns, that together span lo .. hi - 1"""
    return [(t, a, a + n) for a in range(lo, hi - n, step)] + [(t, hi - n, hi)]


def _one_cut():
    """pairs over the left and over the right of column 296 and none across, but for three short fragments of 40 columns"""
    rng = _rng(601)
    tg = [_seq(rng, 600)]
    frags = cover(0, 0, 292) + cover(0, 300, 600) + [(0, 276, 316)] * 3
    return _make(tg, frags, variants=(dict(margin=50, inset=20), dict(margin=50, inset=20, min_span=2), dict(margin=50, inset=0), dict(margin=50, inset=19)))


def _threshold():
    """span 3 left of column 200 and right of 209, span 2 on 200 .. 209"""
    rng = _rng(602)
    tg = [_seq(rng, 400)]
    frags = [(0, 0, 200)] * 3 + [(0, 210, 400)] * 3 + [(0, 150, 260)] * 2
    return _make(tg, frags, variants=(dict(min_span=3), dict(min_span=2), dict(min_span=1), dict(min_span=6), dict(min_span=5)))


def _inset():
    """inset 15: a fragment of 30 columns spans nothing, one of 31 exactly column 150"""
    rng = _rng(603)
    tg = [_seq(rng, 300), _seq(rng, 300)]
    frags = [(0, 0, 140), (0, 160, 300), (0, 135, 165), (1, 0, 140), (1, 160, 300), (1, 135, 166)]
    return _make(tg, frags, variants=(dict(margin=20, inset=15), dict(margin=20, inset=16), dict(margin=20, inset=12)))


# (first column, length) of the runs of the case midpoint: among their first and their last columns are columns = 63 and 0 mod 64 and = 255 and
# 0 mod 256 (starts 63, 127, 192, 255, 512, 703, 896, 1279; ends 63, 128, 383, 575, 767, 1024)
MID_RUNS = ((63, 1), (127, 2), (192, 3), (255, 4), (321, 63), (512, 64), (703, 65), (896, 129), (1279, 300))
MID_LEN = 1700


def _midpoint():
    rng = _rng(604)
    tg = [_seq(rng, MID_LEN)]
    frags, at = [], 0
    for s, n in MID_RUNS:
        frags.append((0, at, s))
        at = s + n
    frags.append((0, at, MID_LEN))
    return _make(tg, frags, shifts=[0], variants=({}, dict(margin=0), dict(margin=64)))


OPEN_LENS = (200, 300, 300, 300, 60, 61, 63)                         # margin 30: the last three are 2 * margin, 2 * margin + 1, 2 * margin + 3


def _open():
    """no pair on target 0; the run of target 1 reaches the first candidate, that of target 2 the last; the uncovered columns of target 3 lie in
    the margin; target 4 has no candidate, target 5 one; target 6 is the shortest that can be cut: its column 31 alone is not spanned"""
    rng = _rng(605)
    tg = [_seq(rng, n) for n in OPEN_LENS]
    frags = [(1, 100, 300), (2, 0, 200), (3, 25, 300), (6, 0, 31), (6, 32, 63)]
    return _make(tg, frags, variants=({}, dict(margin=0), dict(margin=31)))


SEAM_LENS = (140, 0, 133, 0, 0, 161, 17, 129, 0, 125, 150, 0, 131, 1, 126)


def _seams():
    """empty targets between the targets, targets that abut; every target of 120 columns or more lacks its middle ten columns and, every second
    one, its first or last thirty"""
    rng = _rng(606)
    tg = [_seq(rng, n) for n in SEAM_LENS]
    frags = []
    for t, n in enumerate(SEAM_LENS):
        if n < 120:
            continue
        mid = n // 2
        frags += [(t, 30 if t % 4 == 2 else 0, mid - 5), (t, mid + 5, n - 30 if t % 4 == 0 else n)]
    return _make(tg, frags, shifts=[5 * i % 16 for i in range(len(tg))], gaps=[i % 4 != 1 and i != 10 for i in range(len(tg))],
                 variants=(dict(margin=10), dict(margin=0), dict(margin=31)))


MANY_SMALL, MANY_CUTS, MANY_SEG = 20, 300, 66


def _many_cuts():
    """20 small targets with 0 .. 2 cuts, one target of 301 segments with two unspanned columns between them, 20 more small targets"""
    rng = _rng(607)
    small = lambda: _seq(rng, 150)
    tg = [small() for _ in range(MANY_SMALL)] + [_seq(rng, (MANY_CUTS + 1) * MANY_SEG)] + [small() for _ in range(MANY_SMALL)]
    frags = []
    for t in range(len(tg)):
        if t == MANY_SMALL:
            frags += [(t, MANY_SEG * i + 2, MANY_SEG * (i + 1)) for i in range(MANY_CUTS + 1)]
        else:
            frags += [[(t, 0, 150)], [(t, 0, 70), (t, 80, 150)], [(t, 0, 45), (t, 50, 100), (t, 105, 150)]][t % 3]
    order = rng.permutation(len(frags))
    return _make(tg, [frags[i] for i in order], shifts=[7 * i % 16 for i in range(len(tg))])


def _not_proper():
    """columns 180 .. 219 of target 0 are spanned by no proper pair, but an improper pair, a split pair, a read with two placements and unpaired
    reads lie over them"""
    rng = _rng(608)
    a = _seq(rng, 400)
    b = _seq(rng, 100)
    c = np.concatenate([_seq(rng, 40), a[185:215], _seq(rng, 30)])
    tg = [a, b, c]
    extra = [(a[170:195], a[200:225], True),                               # both on the `+` strand: improper
             (a[175:200], P.revcomp(b[40:65]), True),                      # the mate on another target: split
             (a[187:212], P.revcomp(a[300:325]), True),                    # two placements (target 2 holds a copy): not unique
             (a[190:215], P.revcomp(a[178:203]), False), (P.revcomp(a[183:208]), a[195:220], False)]   # unpaired
    return _make(tg, cover(0, 0, 180) + cover(0, 220, 400), extra=extra)


def _pile_up():
    """3000 fragments over the same 200 columns beside columns of span 1, and ten columns that nothing spans"""
    rng = _rng(609)
    tg = [_seq(rng, 500)]
    frags = [(0, 100, 300)] * 3000 + [(0, 0, 110), (0, 310, 500)]
    order = rng.permutation(len(frags))
    return _make(tg, [frags[i] for i in order])


def _no_pairs():
    rng = _rng(610)
    tg = [_seq(rng, 300), _seq(rng, 0), _seq(rng, 150)]
    return _make(tg, [(0, 0, 140), (0, 160, 300), (2, 0, 150)], paired=False)


def _empty(reads, targets):
    def make():
        rng = _rng(611)
        tg = [_seq(rng, n) for n in targets]
        rd = [_seq(rng, 30) for _ in range(reads)]
        c = PC._make(rd, tg, pair_off=np.array([1, 1, 2, 2] * (reads // 2), dtype=np.uint8) if reads else None)
        return dict(c, seqs=tg, frags=[], variants=[dict(DEFAULT)])
    return make


CASES = {"one_cut": _one_cut, "threshold": _threshold, "inset": _inset, "midpoint": _midpoint, "open": _open, "seams": _seams, "many_cuts": _many_cuts,
         "not_proper": _not_proper, "pile_up": _pile_up, "no_pairs": _no_pairs, "n0": _empty(0, (100, 0, 50)), "t0": _empty(4, ()), "all_empty": _empty(4, (0, 0, 0))}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def placed(name):
    c = case(name)
    return P.place(*PC.args(c), **c["params"])


def break_args(c, pl, seqs=None):
    return c["rows"], c["lens"], c["pair_off"], pl, c["seqs"] if seqs is None else seqs


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return BC.break_pairs(*break_args(c, placed(name)), **c["variants"][i])


def every():
    """(name, variant index) of all cases"""
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


# ---- the planted chimera: two contigs of a 4000-base genome, the second one joined wrongly at its column 1300 ----------------------------
CHIMERA_SEED, CHIMERA_PAIRS, CHIMERA_JUNCTION = 501, 1000, 1300


@functools.lru_cache(maxsize=None)
def chimera(noisy=False):
    """-> the case dict and the genome: targets [revcomp(g[1300:2700]), g[0:1300] + g[2700:4000]], 1000 pairs with outer inserts of
    300 .. 400 and reads of 100, drawn as scaffold_cases.planted_genome draws them; noisy: 1 % substitutions in the reads"""
    rng = _rng(CHIMERA_SEED)
    g = _seq(rng, 4000)
    tg = [P.revcomp(g[1300:2700]), np.concatenate([g[0:1300], g[2700:4000]])]
    reads = []
    for _ in range(CHIMERA_PAIRS):
        ins = int(rng.integers(300, 401))
        a = int(rng.integers(0, 4000 - ins + 1))
        pair = [g[a:a + 100], P.revcomp(g[a + ins - 100:a + ins])]
        reads += pair if rng.integers(0, 2) else pair[::-1]
    if noisy:
        out = []
        for r in reads:
            r = r.copy()
            e = rng.random(len(r)) < 0.01
            r[e] = (r[e] + rng.integers(1, 4, size=int(e.sum()))) & 3
            out.append(r)
        reads = out
    c = PC._make(reads, tg, pair_off=np.array([1, 1, 2, 2] * CHIMERA_PAIRS, dtype=np.uint8))
    return dict(c, seqs=tg, frags=[], variants=[dict(min_span=1, inset=21)]), g


def pieces_case(c, res):
    """the reads of case c with the pieces of the break result `res` as targets: what the second placement takes"""
    seqs = BC.pieces_of(res)
    tw, tb, tl = P.ragged(seqs, [0] * len(seqs))
    return dict(c, twords=tw, tbegin=tb, tlen=tl, seqs=seqs)
