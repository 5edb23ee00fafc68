"""Seeded cases of the polish (tests/polish_checker.py is the definition), built on the placement's cases and checker: the smallest shapes at
which the kernels can go wrong.  case(name) -> the placement case's dict plus `variants`, a list of polish parameters (min_cover,
min_percent, multi); placed(name, multi) -> the checker's placement (depth mode = the polish's voters); checked(name, i) -> the polish
checker's result for variant i, computed once."""
import functools

import numpy as np

import place_cases as PC
import place_checker as P
import polish_checker as Q

_rng, _seq, _sub, _make = PC._rng, PC._seq, PC._sub, PC._make
DEFAULT = dict(min_cover=3, min_percent=60, multi=False)


def _with(c, *variants, **extra):
    return dict(c, variants=[dict(DEFAULT, **v) for v in (variants or ({},))], **extra)


PLANTED_LENS, PLANTED_SHIFTS = (1203, 640, 77, 0, 130), (3, 0, 15, 7, 9)


def planted_columns(n):
    """where a target of n bases differs from its truth: column 2 and every 41st from 10 on"""
    return sorted({p for p in [2] + list(range(10, n, 41)) if p < n})


def _planted():
    rng = _rng(101)
    truths = [_seq(rng, n) for n in PLANTED_LENS]
    targets = [_sub(t, planted_columns(len(t))) for t in truths]
    reads = []
    for t in truths:
        reads += [t[p:p + 100] for p in range(0, len(t) - 100 + 1, 5)]
    reads += [truths[2][p:p + 30] for p in range(0, 77 - 30 + 1, 3)]
    reads = [P.revcomp(r) if i & 1 else r for i, r in enumerate(reads)]
    return _with(_make(reads, targets, shifts=list(PLANTED_SHIFTS), gaps=[True] * 5), truths=truths)


def _vote_target(rng, votes):
    """a 120-base target and one 60-base read per entry of `votes` over its bases 20 .. 79; a read's base at column 70 (its base 50, in none of
    its two seeds) is cur + the entry (mod 4): the counts of that column are chosen, every other column is unanimous"""
    t = _seq(rng, 120)
    reads = []
    for d in votes:
        r = t[20:80].copy()
        r[50] = (r[50] + d) & 3
        reads.append(r)
    return t, reads


# per target: the votes at its column 70 as offsets from cur
TIES = [[0, 0, 1, 1],            # 2 - 2 with cur among the tied: no change
        [1, 1, 2, 2],            # 2 - 2 without it at cover 4: the smaller code wins at 50 %, ambiguous at 60 %
        [3, 3, 1, 1],            # the same, listed the other way round: the order of the voters is nothing
        [1, 1],                  # cover 2 < min_cover: nothing, not even ambiguous
        [1, 1, 1],               # cover 3 = min_cover: changes
        [1, 1, 1, 0, 0],         # 3 of 5 = 60 %: changes
        [1, 1, 1, 1, 0, 0, 0],   # 4 of 7 < 60 %: ambiguous
        [2, 2, 2, 1, 1, 1, 0]]   # a three-way look: cur loses, the two others tie at 3 of 7


def _ties():
    rng = _rng(102)
    targets, reads = [], []
    for votes in TIES:
        t, rs = _vote_target(rng, votes)
        targets.append(t)
        reads += [P.revcomp(r) if i & 1 else r for i, r in enumerate(rs)]
    return _with(_make(reads, targets), {}, dict(min_percent=50), dict(min_cover=2), dict(min_cover=4, min_percent=43), dict(min_percent=100), dict(min_cover=1, min_percent=1))


def _deep():
    """300 voters over columns 100 .. 139 of target 0 (past the 255 of the bit-sliced counters: words 6 .. 8 go the wide way) next to columns of
    cover 1; targets 1 and 2 carry exactly 255 and 256 voters: the last narrow and the first wide cover"""
    rng = _rng(103)
    t0, t1, t2 = _seq(rng, 400), _seq(rng, 90), _seq(rng, 90)
    reads = [t0[50:150], t0[130:230]]
    for i in range(300):
        r = t0[100:140].copy()           # one seed (bases 0 .. 20); the votes below lie behind it
        if i < 200:
            r[30] = (r[30] + 1) & 3      # column 130: 200 of 302 against cur -> changes (66 %)
        if i < 151:
            r[25] = (r[25] + 2) & 3      # column 125: 151 of 301 -> the most votes, 50.1 %: ambiguous
        if i >= 160:
            r[35] = (r[35] + 3) & 3      # column 135: 140 of 302: cur keeps the most votes
        reads.append(r)
    for t, n in ((t1, 255), (t2, 256)):
        for i in range(n):
            r = t[20:70].copy()
            if 3 * i < 2 * n:
                r[40] = (r[40] + 1) & 3  # column 60: two thirds against cur -> changes
            reads.append(P.revcomp(r) if i & 1 else r)
    return _with(_make(reads, [t0, t1, t2], shifts=[5, 0, 11]))


def _long_among_short():
    """one 2800-nt read among 100-nt reads: the backward walk of every word is bounded by the longest voter, and most of what it passes ended long
    before the word"""
    rng = _rng(104)
    truth = _seq(rng, 3300)
    planted = list(range(37, 3300, 97))
    target = _sub(truth, planted)
    reads = [truth[p:p + 100] for p in range(0, 3201, 25)]
    reads = [P.revcomp(r) if i % 3 == 1 else r for i, r in enumerate(reads)]
    reads.insert(40, truth[150:2950])
    return _with(_make(reads, [target], shifts=[13], max_mismatches=40), {}, dict(min_cover=5, min_percent=90), truths=[truth])


def _seam_targets(rng, tail):
    truths = [_seq(rng, PC.TINY_LENS[i % 19]) for i in range(60)] + [_seq(rng, tail)]
    targets, reads = [], []
    for i, t in enumerate(truths):
        n = len(t)
        at = ([n - 1] if n >= 22 else []) + ([0] if n >= 43 else [])         # a seed of the truth stays whole: 21 .. 41 where base 0 is hit
        targets.append(_sub(t, at))
        if n >= 21:
            reads += [P.revcomp(t) if (i + j) & 1 else t for j in range(2 + i % 3)]
    return truths, targets, reads


def _seams(tail):
    def make():
        truths, targets, reads = _seam_targets(_rng(105), tail)
        return _with(_make(reads, targets, shifts=[5 * i % 16 for i in range(len(targets))], gaps=[i % 4 != 1 for i in range(len(targets))]),
                     {}, dict(min_cover=2), truths=truths)
    return make


def _minus_only():
    rng = _rng(106)
    truth = _seq(rng, 700)
    target = _sub(truth, [5, 100, 333, 334, 335, 650, 699])
    reads = [P.revcomp(truth[p:p + 90]) for p in range(0, 611, 10)]
    return _with(_make(reads, [target], shifts=[9]), truths=[truth])


def _multi():
    """a 150-base segment twice in the target, both copies with the same substitution: the reads of the segment lie on both at mm 1, MULTI, best
    placement the first copy.  With ALGA_POLISH_MULTI the first copy changes back and the second does not; without it neither"""
    rng = _rng(107)
    seg = _seq(rng, 150)
    bad = _sub(seg, [75])
    truth = np.concatenate([_seq(rng, 120), seg, _seq(rng, 200), seg, _seq(rng, 90)])
    target = truth.copy()
    target[120:270], target[470:620] = bad, bad
    target = _sub(target, [60, 350])                                             # outside the repeat: unique reads vote there either way
    reads = [seg[p:p + 100] for p in (0, 10, 20, 30, 50)] + [truth[p:p + 100] for p in (0, 10, 15, 300, 310, 320, 330)]
    reads = [P.revcomp(r) if i & 1 else r for i, r in enumerate(reads)]
    return _with(_make(reads, [target], shifts=[2]), {}, dict(multi=True), truths=[truth])


def _nobody_unplaced():
    rng = _rng(108)
    return _with(_make([_seq(rng, 100), _seq(rng, 60), None], [_seq(rng, 333), _seq(rng, 0), _seq(rng, 17)]), {}, dict(multi=True, min_cover=1))


CASES = {"planted": _planted, "ties": _ties, "deep": _deep, "long_among_short": _long_among_short, "seams": _seams(22), "seams16": _seams(37),
         "minus_only": _minus_only, "multi": _multi, "nobody_unplaced": _nobody_unplaced,
         "nobody_n0": lambda: _with(PC.case("empty_reads"), {}, dict(multi=True)), "nobody_t0": lambda: _with(PC.case("empty_targets"), {}, dict(multi=True))}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def place_flags(variant):
    """the placement's depth mode that counts what this variant lets vote"""
    return P.DEPTH_MULTI if variant["multi"] else 0


def polish_flags(variant, counts=False):
    return (Q.MULTI if variant["multi"] else 0) | (Q.COUNTS if counts else 0)


@functools.lru_cache(maxsize=None)
def placed(name, multi=False):
    c = case(name)
    return P.place(*PC.args(c), flags=P.DEPTH_MULTI if multi else 0, **c["params"])


def polish_args(c, pl):
    return c["rows"], c["lens"], pl, c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    v = c["variants"][i]
    return Q.polish_scatter(*polish_args(c, placed(name, v["multi"])), min_cover=v["min_cover"], min_percent=v["min_percent"], flags=polish_flags(v))


def every():
    """(name, variant index) of all cases"""
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


CHAIN_SEED, CHAIN_ERR = 31, 0.01


@functools.lru_cache(maxsize=None)
def chain_reads():
    """the `chain` recipe of the placement's GPU test (6 kb with a 400-nt repeat, 2400 reads of 100 nt) with 1 % substitutions in the reads
    -> (words, lens, genome)"""
    import graph_cases as GC
    r = GC.replicon_reads(circular=[], linear=[6000], n=2400, length=GC.READ_LEN, seed=CHAIN_SEED, copy=(1000, 4000, 400))
    rng = _rng(CHAIN_SEED + 1000)
    reads = []
    for k in range(len(r.lens) // 2):
        c = P.codes_of(r.words[2 * k + 1], 0, int(r.lens[2 * k + 1])).copy()
        e = rng.random(len(c)) < CHAIN_ERR
        c[e] = (c[e] + rng.integers(1, 4, size=int(e.sum()))) & 3
        reads.append(c.astype(np.uint8))
    words, lens = P.nodes_of(reads, r.words.shape[1])
    return words, lens, r.genomes[0]


def final_targets(uh, ch, fh):
    """(words, begin, len) of the targets of a final result from the host copies of the unitigs, the consensus and the final set"""
    order = fh["order"].astype(np.int64)
    live = fh["verdict"][order] == 2                                             # ALGA_FINAL_ACCEPTED
    begin = 16 * np.asarray(uh["word_off"]).astype(np.int64)[order] + np.where(live, fh["begin"][order], 0)
    return ch["words"], begin, np.where(live, fh["len"][order], 0).astype(np.int32)


def distance_to(genome, seq):
    """the smallest Hamming distance of `seq` to a window of the genome, on either strand"""
    if len(seq) == 0 or len(seq) > len(genome):
        return 0 if len(seq) == 0 else len(seq)
    best = len(seq)
    for g in (genome, P.revcomp(genome)):
        best = min(best, int((np.lib.stride_tricks.sliding_window_view(g, len(seq)) != seq).sum(axis=1).min()))
    return best
