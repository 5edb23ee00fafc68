"""The cases of the gapped placement (tests/test_gapped_cpu.py, tests/test_gpu_gapped.py): the smallest shapes at which the kernels can go wrong.
A case is the node set, the ragged targets, the parameters of the Hamming placement that runs first (max_mismatches 0 unless said: only exact
reads are placed, every edited read is left to the gapped pass) and the variants of the gapped parameters."""
import functools

import numpy as np

import gapped_checker as GC
import place_checker as P


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)


def edit(seq, edits):
    """a copy of seq with edits applied, given in positions of seq: ('D', at, n) drops n bases from at on, ('I', at, bases) inserts before at,
    ('S', at) substitutes the base at"""
    out, at = [], 0
    for e in sorted(edits, key=lambda x: x[1]):
        out.append(seq[at:e[1]])
        at = e[1]
        if e[0] == "D":
            at += e[2]
        elif e[0] == "I":
            out.append(np.asarray(e[2], dtype=np.uint8))
        else:
            out.append(np.array([(int(seq[at]) + 1) & 3], dtype=np.uint8))
            at += 1
    out.append(seq[at:])
    return np.concatenate(out).astype(np.uint8)


def other(b):
    return [(int(b) + 2) & 3]


def make(reads, seqs, variants=None, place=None, gaps=None, stride=None):
    rows, lens = P.nodes_of(reads, stride)
    tw, tb, tl = P.ragged(seqs, [(3 * i) % 16 for i in range(len(seqs))], gaps)
    return dict(rows=rows, lens=lens, twords=tw, tbegin=tb, tlen=tl, seqs=seqs, reads=reads, place=dict(dict(k=21, max_mismatches=0), **(place or {})),
                variants=variants or [dict()])


def _indel_positions():
    """150-nt reads, k = 21 (7 seeds, 3 bases behind the last): one deleted and one inserted base inside seed 0, inside the last seed, on a seed
    boundary, in the last L mod k bases, and on the base next to the anchoring seed on either side (the other seeds broken by substitutions)"""
    g = rand(11, 400)
    reads = []
    for at in (10, 135, 42, 147):
        w = g[100:251]                                               # 151 bases, one deleted: 150
        reads.append(edit(w, [("D", at, 1)]))
        w = g[100:249]
        reads.append(edit(w, [("I", at, other(w[at]))]))
    # only seed 3 (63 .. 83) stays exact: the indel on the base before it (62) and behind it (84)
    subs = [("S", 5), ("S", 30), ("S", 50), ("S", 110), ("S", 130)]
    for at in (62, 84):
        reads.append(edit(g[100:251], subs + [("D", at + (at > 63), 1)]))
        reads.append(edit(g[100:249], subs + [("I", at, other(g[100 + at]))]))
    return make(reads, [g], [dict(), dict(max_edits=8)])


def _homopolymer():
    """a 1-base indel inside a run of six A: the canonical script decides the column; the same reads reverse complemented"""
    g = rand(12, 300)
    g[140:146] = 0
    g[139], g[146] = 1, 2
    reads = [edit(g[80:221], [("D", 62, 1)]), edit(g[80:219], [("I", 62, [0])])]
    reads += [P.revcomp(r) for r in reads]
    return make(reads, [g])


def _edit_bound():
    """exactly E edits placed and E + 1 not; one indel run of length E (the band's edge) and of E + 1; E = 1, 3 and 15 (31 diagonals)"""
    g = rand(13, 500)
    reads = []
    for E in (1, 3, 15):
        for n in (E, E + 1):
            reads.append(edit(g[50:200], [("S", 40 + 5 * i) for i in range(n)]))
            reads.append(edit(g[50:200 + n], [("D", 70, n)]))
            reads.append(edit(g[50:200 - n], [("I", 70, rand(n, n))]))
    return make(reads, [g], [dict(max_edits=1), dict(max_edits=3), dict(max_edits=15)])


def _cigar_runs():
    """alternating indels and matches: a script of 2 E + 1 runs at E = 3 (and the same read at E = 2: not placed)"""
    g = rand(14, 400)
    w = g[100:250]
    reads = [edit(w, [("D", 30, 1), ("I", 60, other(w[60])), ("D", 100, 1)]), edit(w, [("I", 25, other(w[25])), ("D", 75, 1), ("I", 125, other(w[125]))])]
    return make(reads, [g], [dict(max_edits=3), dict(max_edits=2)])


def _overhang():
    """reads hanging over the first and the last column of a target by 1, by E = 3 and by E + 1 bases; a target shorter than the read"""
    g = rand(15, 300)
    reads = []
    for x in (1, 3, 4):
        reads.append(np.concatenate([rand(100 + x, x), g[:100 - x]]))
        reads.append(np.concatenate([g[300 - 100 + x:], rand(200 + x, x)]))
    short = rand(16, 98)
    reads.append(np.concatenate([other(short[0]), short, other(short[-1])]).astype(np.uint8))
    return make(reads, [g, short], [dict(max_edits=3)])


def _seams():
    """two abutting targets (the seam inside one packed word) and a read of their concatenation with a deleted base: it must not be laid across
    the seam; empty targets in between; the same read is placed where the concatenation is one target"""
    a, b = rand(19, 200), rand(20, 200)
    ab = np.concatenate([a, b])
    reads = [edit(ab[150:251], [("D", 20, 1)]), edit(ab[194:295], [("D", 60, 1)]), edit(ab[120:221], [("I", 30, other(ab[150]))])]
    empty = np.zeros(0, np.uint8)
    return make(reads, [a, b, empty, empty, ab[5:395]], gaps=[True, False, False, False, True], variants=[dict(), dict(max_edits=2)])


def _uniqueness():
    """two loci at equal d: not UNIQUE; one locus seen on two neighbouring diagonals (seeds on both sides of a deletion): UNIQUE; a read equal to
    its own reverse complement: both strands at one locus, not UNIQUE"""
    g = rand(21, 300)
    two = np.concatenate([g[:150], rand(22, 40), g[:150], rand(23, 40)])
    half = rand(24, 50)
    pal = np.concatenate([half, P.revcomp(half)])
    t2 = np.concatenate([rand(25, 60), pal[:49], pal[50:], rand(26, 60)])      # the palindrome with its middle base deleted
    reads = [edit(g[20:141], [("D", 60, 1)]), edit(g[150:271], [("D", 60, 1)]), pal]
    return make(reads, [two, g[150:], t2])


def _read_lengths():
    """64, 65, 128 and 129 nt; ALGA_GAPPED_MAX_READ placed, one more counted in skipped_long; k = 8 on a 1024-nt read (128 seeds, two chunks)"""
    g = rand(27, 1300)
    reads = [edit(g[100:100 + n + 1], [("D", n // 2, 1)]) for n in (64, 65, 128, 129)]
    reads += [edit(g[50:50 + 1025], [("D", 500, 1)]), edit(g[50:50 + 1026], [("D", 500, 1)])]
    return make(reads, [g], [dict(), dict(k=8, max_occ=8)], stride=P.blocks_of(1025))


def _participation():
    """a read the Hamming pass placed with 2 mismatches although a gapped placement with 1 edit exists elsewhere: untouched; a read shorter than k;
    a read whose every seed is over max_occ; a read with no exact seed at all; an exact read (placed)"""
    g = rand(28, 400)
    rep = np.tile(rand(29, 21), 8)                                   # every 21-mer of it occurs 8 times in the target below
    w = g[50:150]
    first = edit(w, [("S", 10), ("S", 90)])
    t_del = edit(first, [("D", 40, 1)])                              # in a second target: that read with one base deleted
    reads = [first, g[200:215], rep[:100], edit(g[200:300], [("S", 5 + 10 * i) for i in range(10)]), g[250:350]]
    return make(reads, [g, np.concatenate([rand(30, 30), t_del, rand(31, 30)]), np.concatenate([rep, rand(32, 10), rep])], [dict(max_occ=7), dict()],
                place=dict(max_mismatches=2, max_occ=7))


def _empty_pass():
    """every read is placed by the Hamming pass, or there is none: all arrays at their defaults, cover == pl.cover"""
    g = rand(33, 300)
    return make([g[10:110], P.revcomp(g[150:250]), None], [g])


def _no_reads():
    return make([], [rand(34, 100)])


def _no_targets():
    """reads and no target: every read is tried, the index is empty"""
    return make([rand(35, 100), rand(36, 50)], [])


def _short_targets():
    """every target is shorter than k (an empty one among them): columns, and no indexed position"""
    return make([rand(37, 100), rand(38, 50)], [rand(39, 10), np.zeros(0, np.uint8), rand(40, 20)], gaps=[True, False, False])


CASES = {"indel_positions": _indel_positions, "homopolymer": _homopolymer, "edit_bound": _edit_bound, "cigar_runs": _cigar_runs, "overhang": _overhang, "seams": _seams,
         "uniqueness": _uniqueness, "read_lengths": _read_lengths, "participation": _participation, "empty_pass": _empty_pass, "no_reads": _no_reads,
         "no_targets": _no_targets, "short_targets": _short_targets}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def placed(name):
    """the Hamming placement the gapped pass starts from (tests/place_checker.py)"""
    c = case(name)
    return P.place(c["rows"], c["lens"], None, *targets(c), **c["place"])


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return GC.gapped_banded(c["rows"], c["lens"], placed(name), *targets(c), **c["variants"][i])


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


@functools.lru_cache(maxsize=None)
def planted(seed=41):
    """a 6 kb random genome as one target, 30x reads of 100 nt from both strands, each with one planted 1-base indel at a random column
    -> (case, the true first column of every read, its strand)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=6000, dtype=np.uint8)
    reads, start, minus = [], [], []
    for _ in range(6000 * 30 // 100):
        a, at = int(rng.integers(0, 6000 - 101)), int(rng.integers(1, 99))
        if rng.integers(0, 2):
            w = edit(g[a:a + 101], [("D", at, 1)])
        else:
            w = edit(g[a:a + 99], [("I", at, other(g[a + at]))])
        m = int(rng.integers(0, 2))
        reads.append(P.revcomp(w) if m else w)
        start.append(a)
        minus.append(m)
    return make(reads, [g]), np.array(start), np.array(minus)


@functools.lru_cache(maxsize=None)
def many_reads(n):
    """n reads of 64 nt with one deleted base, drawn from 40 different ones, on a 2 kb target: more than one grid of k_gp_score holds"""
    g = rand(42, 2000)
    pool = [edit(g[a:a + 65], [("D", 30, 1)]) for a in range(0, 1900, 48)]
    return make([pool[(7 * i) % len(pool)] for i in range(n)], [g])
