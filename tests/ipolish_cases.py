"""The cases of the polish with the gapped reads (tests/test_ipolish_cpu.py, tests/test_gpu_ipolish.py): the smallest shapes at which the kernels
can go wrong.  A case is the node set, the ragged targets, the parameters of the Hamming placement (max_mismatches 0: only exact reads are H
voters, every other read is left to the gapped pass) and of the gapped pass, and the variants of this stage's parameters.  The placement and
the gapped placement come from tests/place_checker.py and tests/gapped_checker.py.

A case is built from a TRUTH (what the reads are drawn from) and a target that differs from it: `edit(truth, [...])` in the positions of the
truth -- a 'D' there takes bases out of the target (the reads then insert them), an 'I' puts bases into the target (the reads delete them)."""
import functools

import numpy as np

import gapped_cases as QC
import gapped_checker as GC
import ipolish_checker as IC
import place_checker as P

rand, edit, other = QC.rand, QC.edit, QC.other


def make(reads, seqs, variants=None, gapped=None, gaps=None, stride=None):
    c = QC.make(reads, seqs, variants, None, gaps, stride)
    c["gapped"] = gapped or {}
    return c


def windows(src, starts, length=100, both=True):
    """reads of `length` from src at the given starts, every second one reverse complemented"""
    out = []
    for i, a in enumerate(starts):
        w = np.asarray(src[a:a + length], dtype=np.uint8)
        out.append(P.revcomp(w) if both and i & 1 else w)
    return out


def plain(seed, n):
    """a random sequence without two equal neighbours: an indel planted in it has one place only"""
    g = rand(seed, n)
    for i in range(1, n):
        if g[i] == g[i - 1]:
            g[i] = (int(g[i]) + 1 + (i + 1 < n and (int(g[i]) + 1) & 3 == g[i + 1])) & 3
    return g


def _normalise():
    """a homopolymer of six with one base too few and one with one base too many, voted by reads whose gap lies inside seed 0 (traced through
    the left part: the gap at the run's LAST base) and further in (at its first): they pool at the run's first column; ACACACAC against a
    target with ACACAC (the inserted string rotates, CA against AC); a second event three columns into a run, behind a gap (the shift stops at
    m); reads that begin inside the run (a shift that would pass the script's first column)"""
    g = plain(101, 900)
    g[200:206], g[199], g[206] = 0, 1, 2                             # AAAAAA, the target gets five
    g[400:406], g[399], g[406] = 3, 0, 1                             # TTTTTT, the target gets seven
    g[600:608], g[599], g[608] = [0, 1] * 4, 2, 2                    # ACACACAC, the target gets ACACAC
    g[752:758], g[751], g[758] = 2, 1, 3                             # GGGGGG three columns behind a deleted column: m = 3 for its gap
    t = edit(g, [("D", 203, 1), ("I", 403, [3]), ("D", 604, 2), ("I", 748, other(g[748])), ("D", 755, 1)])
    starts = []
    for at in (200, 400, 600, 750):
        starts += [at - 12, at - 8, at - 3, at + 1, at + 2, at - 60, at - 45, at - 70, at - 30, at - 88, at - 95]
    return make(windows(g, starts), [t], [dict(), dict(min_cover=1)])


def _ties():
    """one site per mix of votes on a column the target has too many of (`-`), holds (cur) or holds wrong (another base): `-` against cur tied;
    `-` against a base tied with cur not among them (the smallest base wins, `-` comes last); cover at min_cover and one below; 3 of 5 at 59,
    60 and 61 per cent; a three-way vote"""
    g = plain(102, 1400)
    sites = [150 + 170 * i for i in range(7)]
    extra = [[next(b for b in range(4) if b != g[s - 1] and b != g[s])] for s in sites]      # the column the target has too many: unlike both neighbours, it has one place
    t = edit(g, [("I", s, x) for s, x in zip(sites, extra)])
    col = [s + i for i, s in enumerate(sites)]                       # the extra column of site i in the target
    mix = [(2, 2, 0), (2, 0, 2), (3, 0, 0), (2, 0, 0), (3, 2, 0), (2, 1, 2), (1, 1, 2)]      # (`-`, cur, another base)
    reads = []
    for i, (nd, ncur, ny) in enumerate(mix):
        y = t.copy()
        y[col[i]] = (int(t[col[i]]) + 1) & 3
        for j in range(nd):
            reads += windows(g, [sites[i] - 35 - 7 * j])
        for j in range(ncur):
            reads += windows(t, [col[i] - 40 - 7 * j])
        for j in range(ny):
            reads += windows(y, [col[i] - 45 - 7 * j])
    c = make(reads, [t], [dict(), dict(min_percent=50), dict(min_percent=59), dict(min_percent=61), dict(min_cover=2, min_percent=40), dict(min_cover=1, min_percent=1)])
    c["cols"] = col
    return c


def _no_equal_neighbours(codes, n):
    out = []
    for b in codes:
        if not out or out[-1] != b:
            out.append(int(b))
    return out[:n]


def _insert_vote():
    """slots the target lacks bases at: two strings at one slot; a tie between two strings (the smaller n, then the smaller string); span at the
    bound and one below; max_ins + 1 bases (counted, no vote, the slot ambiguous); max_ins 1 and 13; reads hanging over the target's ends (edge
    I runs vote nothing)"""
    g = plain(103, 1700)
    sites = [150 + 170 * i for i in range(8)]
    # the 13 bases are a run of T between stretches without T: unit costs split a longer insertion wherever a base matches by chance
    free = lambda seed, n: _no_equal_neighbours(rand(seed, 8 * n) % 3, n)
    g[sites[7] - 20:sites[7]], g[sites[7]:sites[7] + 13], g[sites[7] + 13:sites[7] + 33] = free(1, 20), 3, free(2, 20)
    t = edit(g, [("D", s, 1) for s in sites[:6]] + [("D", sites[6], 7), ("D", sites[7], 13)])
    reads = []

    def with_string(i, bases, n, shift=0):
        """n reads over site i that carry `bases` where the target lacks g[site]"""
        src = np.concatenate([g[:sites[i]], np.asarray(bases, dtype=np.uint8), g[sites[i] + 1:]])
        return windows(src, [sites[i] - 30 - 7 * (j + shift) for j in range(n)])
    a = int(g[sites[0]])
    reads += with_string(0, [a], 3) + with_string(0, [(a + 1) & 3 if (a + 1) & 3 != g[sites[0] - 1] else (a + 2) & 3], 2, 3)      # 3 of one string, 2 of another
    b = int(g[sites[1]])
    reads += with_string(1, [b], 2) + with_string(1, [b, (b + 1) & 3], 2, 2)                                                   # n = 1 against n = 2, tied
    d = int(g[sites[2]])
    reads += with_string(2, [d], 2) + with_string(2, [d ^ 1 if (d ^ 1) != g[sites[2] - 1] and (d ^ 1) != g[sites[2] + 1] else d ^ 2], 2, 2)      # two strings of one base, tied
    reads += with_string(3, [int(g[sites[3]])], 3)                   # span == min_cover
    reads += with_string(4, [int(g[sites[4]])], 2)                   # one below
    reads += with_string(5, [int(g[sites[5]]), (int(g[sites[5]]) + 2) & 3], 3)      # two bases: too long at max_ins 1
    reads += windows(g, [sites[6] - 40 - 5 * j for j in range(3)])   # 7 bases
    reads += windows(g, [sites[7] - 40 - 5 * j for j in range(3)])   # 13 bases
    reads += [np.concatenate([rand(300 + x, x), t[:100 - x]]) for x in (1, 2)] * 2 + [np.concatenate([t[len(t) - 100 + x:], rand(310 + x, x)]) for x in (1, 3)]
    c = make(reads, [t], [dict(), dict(min_percent=50), dict(max_ins=1), dict(max_ins=13), dict(max_ins=7, min_cover=2)], gapped=dict(max_edits=15))
    return c


def _adjacent():
    """three deleted columns in a row; a deleted column three columns from an inserted slot (nearer, the canonical script says substitutions);
    a substitution and a deletion in one word; a slot at a word boundary (g & 15 == 0); a second target of 16 * 16 columns
    whose col_off moves and whose tail an insertion pushes across a word"""
    g = plain(104, 320)
    h = plain(105, 257)
    t = edit(g, [("I", 60, [int(g[60]) ^ 1, int(g[60]) ^ 2, int(g[60]) ^ 1]), ("I", 120, other(g[120])), ("D", 123, 1), ("S", 196), ("I", 201, other(g[201]))])
    # the first target has 324 columns, the second 256 = 16 * 16: its missing base is the slot before its column 172, column 496 = 16 * 31 of all
    u = edit(h, [("D", 172, 1)])
    reads = windows(g, list(range(0, 221, 9))) + windows(h, list(range(0, 158, 9)))
    return make(reads, [t, u], [dict(), dict(min_cover=2)])


def _beside():
    """a deleted column directly beside an inserted slot.  No single script holds that (unit costs: a D run next to an I run costs 2 where a
    substitution costs 1), but column and slot are decided independently, so two read populations give it: four reads of a truth that lacks
    the target's column g (`-` at g, 4 of 7) and three of a truth with one base more behind column g (cur at g; an insertion at slot g + 1,
    3 of the 7 that span it).  At 40 per cent both pass: column g leaves and carries no insertion, column g + 1 stays and carries one"""
    t = plain(130, 400)
    g = 200
    x = next(b for b in range(4) if b != t[g] and b != t[g + 1])
    lacks = np.concatenate([t[:g], t[g + 1:]])
    more = np.concatenate([t[:g + 1], [x], t[g + 1:]]).astype(np.uint8)
    reads = windows(lacks, [g - 30 - 9 * j for j in range(4)]) + windows(more, [g - 34 - 9 * j for j in range(3)])
    c = make(reads, [t], [dict(min_percent=40), dict(), dict(min_percent=40, min_cover=8)])
    c["g"] = g
    return c


def _carries():
    """a deleted column that itself carries an insertion: five reads of a truth that lacks the target's column g (`-` at g, 5 of 8) and three
    of a truth with one base more BEFORE column g (an insertion at slot g, 3 of the 8 that span it).  At 35 per cent both pass: the old column
    g has width 1, all of it the inserted base"""
    t = plain(131, 400)
    g = 208                                                           # 208 = 16 * 13: the column is the first of its word
    x = next(b for b in range(4) if b != t[g - 1] and b != t[g])
    lacks = np.concatenate([t[:g], t[g + 1:]])
    more = np.concatenate([t[:g], [x], t[g:]]).astype(np.uint8)
    reads = windows(lacks, [g - 30 - 7 * j for j in range(5)]) + windows(more, [g - 34 - 9 * j for j in range(3)])
    c = make(reads, [t], [dict(min_percent=35), dict()])
    c["g"] = g
    return c


def _seams():
    """61 targets of 0 .. 129 bases at offsets 3 i mod 16, 16 of them empty; the targets of at least 70 bases have a column too many in their first
    word, a base too few in their last, or both; reads of 50 nt (two seeds: one stays whole); the following targets' col_off moves by the net change"""
    truths, seqs, reads = [], [], []
    for i in range(61):
        n = 0 if i % 4 == 0 else (17 * i) % 130
        g = plain(400 + i, n)
        truths.append(g)
        if n < 70:
            seqs.append(g)
            continue
        ev = [("I", 15, other(g[15]))] if i % 3 else []
        ev += [("D", n - 13, 1)] if i % 2 else []
        seqs.append(edit(g, ev))
        reads += windows(g, list(range(0, n - 49, 2)), 50)
    c = make(reads, seqs, [dict(), dict(min_cover=2)])
    c["truths"] = truths
    return c


def _deep():
    """more than 255 voters on a column and more than 255 `-` votes on one; stretches with exactly 255 and exactly 256 voters"""
    g = plain(106, 700)
    t = edit(g, [("I", 150, other(g[150]))])
    reads = [g[100:200]] * 300 + [t[300:400]] * 255 + [t[450:550]] * 256 + [P.revcomp(t[590:690])] * 3
    return make(reads, [t], [dict()])


def _no_gapped():
    """every read is exact or has substitutions only and the gapped pass places none (max_edits 1, reads with two): the stage is the polish"""
    g = plain(107, 600)
    t = edit(g, [("S", 100), ("S", 300), ("S", 301), ("S", 480)])
    reads = windows(t, list(range(0, 500, 11))) + [edit(g[a:a + 100], [("S", 10), ("S", 90)]) for a in (120, 140, 333)]
    return make(reads, [t], [dict(), dict(min_cover=1)], gapped=dict(max_edits=1))


def _no_voters():
    return make([rand(108, 100), rand(109, 60)], [plain(110, 300), np.zeros(0, np.uint8), plain(111, 37)], gaps=[True, False, False])


def _no_reads():
    return make([], [plain(112, 100)])


def _no_targets():
    return make([rand(113, 100), rand(114, 50)], [])


WORD_SEAM_LENS = [1, 15, 16, 0, 17, 31, 32, 33]


def _word_seams():
    """k_ip_words at its seams.  Targets of 1, 15, 16, 17, 31, 32 and 33 columns and an empty one keep their length (no read of 50 nt lies on them: a
    target this short has no voter) behind, between and in front of three targets of 120 columns that each lose a column (a deleted column between
    kept ones: an empty item of the walk) and gain bases at a slot, with net changes of +1, -1 and +2: every short target starts at another offset
    in its word than before.  A last target of 4200 columns without a voter: more than 256 new words, so that with ipolish_max_blocks 1 every lane
    takes two; the new total is no multiple of 16"""
    seqs, reads = [], []
    short = [plain(450 + i, n) for i, n in enumerate(WORD_SEAM_LENS)]
    for j, ev in enumerate(([("I", 15, None), ("D", 100, 2)], [("I", 15, None), ("I", 70, None), ("D", 100, 1)], [("I", 40, None), ("D", 80, 3)])):
        g = plain(460 + j, 120)
        seqs += short[3 * j:3 * j + 3]
        seqs.append(edit(g, [(e[0], e[1], other(g[e[1]])) if e[0] == "I" else e for e in ev]))
        reads += windows(g, list(range(0, 71, 2)), 50)
    seqs.append(plain(470, 4200))
    return make(reads, seqs, [dict(), dict(min_cover=2)])


CASES = {"word_seams": _word_seams, "normalise": _normalise, "ties": _ties, "insert_vote": _insert_vote, "adjacent": _adjacent, "seams": _seams, "deep": _deep, "beside": _beside, "carries": _carries, "no_gapped": _no_gapped,
         "no_voters": _no_voters, "no_reads": _no_reads, "no_targets": _no_targets}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def place_of(c):
    pl = P.place(c["rows"], c["lens"], None, *targets(c), **c["place"])
    return pl, GC.gapped_banded(c["rows"], c["lens"], pl, *targets(c), **c["gapped"])


@functools.lru_cache(maxsize=None)
def placed(name):
    """(the Hamming placement, the gapped placement) the stage starts from"""
    return place_of(case(name))


@functools.lru_cache(maxsize=None)
def checked(name, i=0, counts=False):
    c = case(name)
    pl, gp = placed(name)
    return IC.ipolish_scatter(c["rows"], c["lens"], pl, gp, *targets(c), flags=IC.COUNTS if counts else 0, **c["variants"][i])


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


# ---- the planted set -------------------------------------------------------------------------------------------------------------------------
def planted_case(seed):
    """a 6 kb random genome; the target is the genome with 12 planted errors at least 150 columns apart and from the ends: 1- and 3-base
    deletions, 1- and 2-base insertions, one of each inside a homopolymer of six and inside ACACAC, two substitutions; 30x error-free reads of
    100 nt from both strands -> (case, genome)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=6000, dtype=np.uint8)
    at = [300 + 450 * i + int(rng.integers(0, 250)) for i in range(12)]
    g[at[4]:at[4] + 6] = 0
    g[at[5]:at[5] + 6] = 3
    g[at[6]:at[6] + 6] = [0, 1] * 3
    g[at[7]:at[7] + 6] = [0, 1] * 3
    ins = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    ev = [("D", at[0], 1), ("D", at[1], 3), ("I", at[2], ins(1)), ("I", at[3], ins(2)), ("D", at[4] + 2, 1), ("I", at[5] + 2, [3]), ("D", at[6] + 2, 2), ("I", at[7] + 2, [0, 1]),
          ("S", at[8]), ("S", at[9]), ("D", at[10], 1), ("I", at[11], ins(1))]
    t = edit(g, ev)
    starts = rng.integers(0, 6000 - 100, size=6000 * 30 // 100)
    reads = [P.revcomp(g[a:a + 100]) if rng.integers(0, 2) else g[a:a + 100].copy() for a in starts]
    return make(reads, [t]), g


PLANTED_SEEDS = (7, 8, 9, 10, 11, 12)


@functools.lru_cache(maxsize=None)
def planted():
    """the first seed at which the checker alone, with the default parameters, gives back the genome -> (seed, case, genome, pl, gp, result)"""
    for seed in PLANTED_SEEDS:
        c, g = planted_case(seed)
        pl, gp = place_of(c)
        res = IC.ipolish_scatter(c["rows"], c["lens"], pl, gp, *targets(c))
        seq = IC.sequences(res)[0]
        ok = len(seq) == len(g) and (seq == g).all()
        print("planted: seed %d %s" % (seed, "taken" if ok else "not taken (the checker does not give back the genome)"))
        if ok:
            return seed, c, g, pl, gp, res
    raise AssertionError("no seed of %r meets the condition" % (PLANTED_SEEDS,))


# ---- the large planted set: expectations known from how it is planted, no checker walk ------------------------------------------------------
MANY_T, MANY_LEN, MANY_K = 220, 10000, 48       # 2.2 M columns and 220 * 199 * 48 = 2 101 440 reads: both above 8192 blocks of 256 threads


def pack_rows(codes):
    """[n, L] codes -> [n, blocks_of(L)] words"""
    n, L = codes.shape
    stride = P.blocks_of(L)
    c = np.zeros((n, 16 * stride), dtype=np.uint32)
    c[:, :L] = codes
    return (c.reshape(n, stride, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def many(n_targets=MANY_T, tlen=MANY_LEN, copies=MANY_K, seed=140):
    """n_targets truths of tlen bases.  Every truth base at a position = 7 mod 40 is substituted in the target, except around positions 2525 and
    7525: there the target has a column too many (a base unlike both neighbours) resp. lacks a base (the truth's base there is made unlike both
    neighbours), so every event has one place only.  Reads: the windows of 100 at every 50th base of every truth, alternately reverse
    complemented, each `copies` times (read r is window r mod W): at most 3 mismatches, the Hamming pass (max_mismatches 3) places them, the
    indel reads (gap at offset 25 or 75: no Hamming placement within 3) go to the gapped pass.  Every column is covered by two windows, the
    first and last 50 of a target by one; no event lies at a window's edge.  So everything is known from the planting: the new targets are the
    truths, and every event's column, bases, votes and cover.
    -> dict(rows, lens, targets, truths, place, K, events [(target, old pos, kind, len, old, new, votes, cover)] in order, t_subs, t_ins, t_dels)"""
    rng = np.random.default_rng(seed)
    truths = rng.integers(0, 4, size=(n_targets, tlen), dtype=np.uint8)
    def unlike(a, b):                                                 # a base unlike two given ones
        out = (a + 1) & 3
        out = np.where((out == a) | (out == b), (a + 2) & 3, out)
        out = np.where((out == a) | (out == b), (a + 3) & 3, out)
        return out.astype(np.uint8)
    q_more, q_less = 2525, 7525
    truths[:, q_less] = unlike(truths[:, q_less - 1], truths[:, q_less + 1])
    extra = unlike(truths[:, q_more - 1], truths[:, q_more])                                  # the column the target has before truth position q_more
    subs = np.array([q for q in range(7, tlen, 40) if min(abs(q - q_more), abs(q - q_less)) > 45])
    seqs, events = [], []
    cover = lambda q: copies * (1 if q < 50 or q >= tlen - 50 else 2)
    for t in range(n_targets):
        g = truths[t]
        s = g.copy()
        s[subs] = (s[subs] + 1 + (t & 1)) & 3
        tgt = np.concatenate([s[:q_more], [extra[t]], s[q_more:q_less], s[q_less + 1:]]).astype(np.uint8)
        seqs.append(tgt)
        ev = [(int(q) + (q > q_more), 0, 1, "ACGT"[s[q]], "ACGT"[g[q]], cover(q), cover(q)) for q in subs if q < q_less]
        ev.append((q_more, 2, 1, "ACGT"[extra[t]], "-", 2 * copies, 2 * copies))
        ev.append((q_less + 1, 1, 1, "-", "ACGT"[g[q_less]], 2 * copies, 2 * copies))       # the slot before the target's column q_less + 1
        ev += [(int(q), 0, 1, "ACGT"[s[q]], "ACGT"[g[q]], cover(q), cover(q)) for q in subs if q > q_less]
        events += [(t,) + e for e in sorted(ev)]
    starts = np.arange(0, tlen - 99, 50)
    win = np.lib.stride_tricks.sliding_window_view(truths, 100, axis=1)[:, starts, :].reshape(-1, 100)      # [T * W, 100]
    minus = (np.arange(len(win)) & 1) == 1
    fwd = np.where(minus[:, None], 3 - win[:, ::-1], win).astype(np.uint8)
    W = len(fwd)
    pool = np.empty((2 * W, P.blocks_of(100)), dtype=np.uint32)
    pool[1::2] = pack_rows(fwd)
    pool[0::2] = pack_rows((3 - fwd[:, ::-1]).astype(np.uint8))
    rows = np.tile(pool, (copies, 1))
    lens = np.full(2 * W * copies, 100, dtype=np.int32)
    tw, tb, tl = P.ragged(seqs, [(3 * i) % 16 for i in range(n_targets)])
    return dict(rows=rows, lens=lens, targets=(tw, tb, tl), truths=truths, place=dict(k=21, max_mismatches=3), K=copies, events=events,
                t_subs=len(subs), n_reads=W * copies)


def many_texts(m):
    """(the FASTA, the events TSV) of the large planted set, from the planting alone"""
    fa = "".join(">contig_id=%d_length=%d_subs=%d_ins=1_dels=1\n%s\n" % (t, len(g), m["t_subs"], "".join("ACGT"[b] for b in g)) for t, g in enumerate(m["truths"]))
    tsv = "".join("%d\t%d\t%s\t%d\t%s\t%s\t%d\t%d\n" % (t, pos, "SID"[kind], n, old, new, votes, cov) for t, pos, kind, n, old, new, votes, cov in m["events"])
    return fa, tsv
