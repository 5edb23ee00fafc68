"""The cases of the pair calls over both passes and of the SAM writer (tests/test_sam_cpu.py, tests/test_gpu_sam.py): the smallest shapes at which
the kernels can go wrong.  A case is the node set with its pairing, the ragged targets (target i begins at base offset 3 i mod 16), the
parameters of the two placement passes that run first (max_mismatches 0: only exact reads are placed by the Hamming pass, every edited read is
left to the gapped one; k = 12, so that one indel leaves a seed) and max_insert.  Every case is made for one outcome and carries a function that
asserts it from the checker's result, so a case cannot silently test nothing."""
import functools

import numpy as np

import gapped_cases as QC
import gapped_checker as GC
import place_checker as P
import sam_checker as SC

rand, edit, other = QC.rand, QC.edit, QC.other
EMPTY = np.zeros(0, np.uint8)
K, E = 12, 3


def fwd(g, a, n):
    """the `+` read that lies on g[a .. a + n)"""
    return g[a:a + n].copy()


def rev(g, a, n):
    """the `-` read that lies on g[a .. a + n)"""
    return P.revcomp(g[a:a + n])


def make(reads, seqs, pairs, outcome, max_insert=1000, place=None, gapped=None, stride=None):
    """pairs: the smaller read index of every pair (its mate is the next read)"""
    rows, lens = P.nodes_of(reads, stride)
    po = np.zeros(len(lens), np.uint8)
    for r in pairs:
        po[2 * r:2 * r + 2], po[2 * r + 2:2 * r + 4] = 1, 2
    tw, tb, tl = P.ragged(seqs, [(3 * i) % 16 for i in range(len(seqs))])
    return dict(rows=rows, lens=lens, pair_off=po if len(pairs) else None, twords=tw, tbegin=tb, tlen=tl, seqs=seqs, reads=reads, max_insert=max_insert,
                place=dict(dict(k=K, max_mismatches=0, max_insert=max_insert), **(place or {})), gapped=dict(dict(k=K, max_edits=E), **(gapped or {})), outcome=outcome)


def kinds(w, gp=True):
    c = w["case"]
    return [SC.view(c["lens"], w["pl"], w["gp"] if gp else None, r)["kind"] for r in range(len(c["lens"]) // 2)]


def _proper():
    """HH, HG and GG proper pairs, on two targets with an empty one in between; both orders of the strands"""
    a, b = rand(201, 400), rand(202, 380)
    reads = [fwd(a, 10, 100), rev(a, 200, 100),                                                                   # H H
             fwd(a, 20, 100), P.revcomp(edit(a[210:311], [("D", 50, 1)])),                                        # H G(-, deletion)
             P.revcomp(edit(b[200:299], [("I", 40, other(b[240]))])), edit(b[30:131], [("D", 60, 1)]),             # G(-) G(+): the `-` mate first
             rev(b, 150, 90), fwd(b, 5, 120)]                                                                     # H H, the `-` mate first

    def outcome(w):
        i = w["calls"]["info"]
        assert kinds(w) == ["H", "H", "H", "G", "G", "G", "H", "H"]
        assert (i["pairs"], i["pairs_proper"], i["pairs_with_gapped"], i["proper_with_gapped"]) == (4, 4, 2, 2), i
        assert all(int(f) & 0x2 for f in w["calls"]["flag"])
        assert w["no_gp"]["info"]["pairs_proper"] == 2 and w["no_gp"]["info"]["pairs_not_unique"] == 2            # what the Hamming pass alone sees
    return make(reads, [a, EMPTY, b], [0, 2, 4, 6], outcome)


def _split_improper():
    """a G mate on another target (split); the same strand; containment failing both ways (a > b, ea > eb)"""
    a, b = rand(203, 400), rand(204, 300)
    reads = [fwd(a, 10, 100), P.revcomp(edit(b[100:201], [("D", 50, 1)])),          # split, with a gapped mate
             fwd(a, 20, 100), fwd(a, 200, 100),                                     # same strand
             fwd(a, 200, 100), rev(a, 100, 100),                                    # a > b
             fwd(a, 100, 150), rev(a, 120, 100)]                                    # a <= b, ea = 250 > eb = 220

    def outcome(w):
        i = w["calls"]["info"]
        assert (i["pairs"], i["pairs_split"], i["pairs_improper"], i["pairs_proper"], i["pairs_with_gapped"]) == (4, 1, 3, 0, 1), i
        assert w["calls"]["tlen"][0] == 0 and w["calls"]["tlen"][2] == 280 and w["calls"]["tlen"][3] == -280 and w["calls"]["tlen"][6] == 150
    return make(reads, [a, b], [0, 2, 4, 6], outcome)


def _insert_bound():
    """insert == max_insert is proper, max_insert + 1 is not; a `-` mate with a deletion (end = pos + L + 1) that is proper by pos + L and not by
    end, and the converse with an insertion: the two pairs that tell `end` from `pos + len`"""
    a = rand(205, 500)
    reads = [fwd(a, 10, 100), rev(a, 210, 100),                                             # insert 300
             fwd(a, 10, 100), rev(a, 211, 100),                                             # insert 301
             fwd(a, 10, 100), P.revcomp(edit(a[211:311], [("D", 50, 1)])),                  # L 99 on [211, 311): pos + L - a = 300, end - a = 301
             fwd(a, 10, 100), P.revcomp(edit(a[210:310], [("I", 50, other(a[260]))]))]      # L 101 on [210, 310): pos + L - a = 301, end - a = 300

    def outcome(w):
        gp, fl = w["gp"], w["calls"]["flag"]
        assert (int(gp["pos"][5]), int(gp["end"][5]), int(w["case"]["lens"][11])) == (211, 311, 99) and (int(gp["pos"][7]), int(gp["end"][7]), int(w["case"]["lens"][15])) == (210, 310, 101)
        assert [bool(int(f) & 0x2) for f in fl[0::2]] == [True, False, False, True], fl
        assert w["calls"]["insert_hist"][300] == 2 and w["calls"]["info"]["pairs_improper"] == 2
    return make(reads, [a], [0, 2, 4, 6], outcome, max_insert=300)


def _not_unique():
    """a mate that lies on both copies of a repeat: the pair is not unique, MAPQ 0 on that mate"""
    g = rand(206, 300)
    two = np.concatenate([g[:150], rand(207, 40), g[:150], rand(208, 40)])
    reads = [fwd(two, 20, 100), rev(two, 155, 30), fwd(two, 150, 60), rev(two, 330, 50)]

    def outcome(w):
        assert w["pl"]["hits"][0] == 2 and w["calls"]["info"]["pairs_not_unique"] == 1 and w["calls"]["info"]["pairs_proper"] == 1
        assert b"r0\t97\t" in w["text"] or b"r0\t65\t" in w["text"]
    return make(reads, [two], [0, 2], outcome)


def _unplaced_and_dead():
    """one mate unplaced (it borrows RNAME and POS), both unplaced, a read shorter than k, a removed read whose mate is live, single reads
    between the pairs"""
    a = rand(209, 300)
    reads = [fwd(a, 5, 60),                                   # 0 single
             rev(a, 100, 80), rand(210, 70),                  # 1, 2: placed `-`, unplaced
             rand(211, 50), rand(212, 64),                    # 3, 4: both unplaced
             fwd(a, 150, 100),                                # 5 single
             fwd(a, 30, 10), rev(a, 120, 90),                 # 6, 7: shorter than k, placed
             None, fwd(a, 40, 100),                           # 8, 9: removed, live: a single read
             rand(213, 40)]                                   # 10 single, unplaced

    def outcome(w):
        fl = [int(f) for f in w["calls"]["flag"]]
        assert fl == [0, 0x1 | 0x8 | 0x10 | 0x40, 0x1 | 0x4 | 0x20 | 0x80, 0x1 | 0x4 | 0x8 | 0x40, 0x1 | 0x4 | 0x8 | 0x80, 0, 0x1 | 0x4 | 0x20 | 0x40, 0x1 | 0x8 | 0x10 | 0x80, 0, 0, 0x4], fl
        i = w["calls"]["info"]
        assert (i["reads"], i["live"], i["pairs"], i["pairs_not_unique"], i["unplaced"]) == (11, 10, 3, 3, 5), i
        lines = w["text"].split(b"\n")
        borrowed = [s for s in lines if s.startswith(b"r1\t") and b"\t*\t=\t" in s]
        assert len(borrowed) == 1 and borrowed[0].split(b"\t")[2:4] == [b"contig_id=0_length=300", b"101"], borrowed
        assert sum(s.startswith(b"r3\t") and b"\t*\t0\t0\t*\t*\t0\t0\t" in s for s in lines) == 2 and not any(s.startswith(b"r8\t") for s in lines)
    return make(reads, [a], [1, 3, 6, 8], outcome)


def _overhang():
    """reads hanging over the first and the last column of a target by 1 and by E bases, on both strands: leading and trailing I written as S, NM
    reduced by the clipped bases; paired with exact mates.  The overhanging bases differ from the target's end base, so that no script of equal cost
    has the insertion inside"""
    g = rand(214, 300)
    reads = []
    for x in (1, E):
        reads += [np.concatenate([other(g[0]) * x, g[:100 - x]]).astype(np.uint8), rev(g, 150, 100)]                       # leading I, `+`
        reads += [fwd(g, 100, 100), P.revcomp(np.concatenate([g[300 - 100 + x:], other(g[299]) * x]).astype(np.uint8))]      # trailing I, `-`
    reads += [P.revcomp(np.concatenate([other(g[0]) * 2, edit(g[:80], [("S", 30)])]).astype(np.uint8))]                        # a single `-` read: leading I in target orientation, one substitution

    def outcome(w):
        cg = GC.cigar_strings(w["gp"])
        assert [cg[r] for r in (0, 3, 4, 7, 8)] == ["1I99M", "99M1I", "3I97M", "97M3I", "2I80M"], cg
        lines = [s.split(b"\t") for s in w["text"].split(b"\n") if s and not s.startswith(b"@")]
        assert [lines[r][5] for r in (0, 3, 4, 7, 8)] == [b"1S99M", b"99M1S", b"3S97M", b"97M3S", b"2S80M"]
        assert [lines[r][11] for r in (0, 3, 4, 7, 8)] == [b"NM:i:0"] * 4 + [b"NM:i:1"] and w["calls"]["info"]["proper_with_gapped"] == 4
    return make(reads, [g], [0, 2, 4, 6], outcome)


def _runs():
    """a script of 2 E + 1 runs; equal p of both mates (the TLEN sign goes by the read index), in both orders of the strands"""
    g = rand(215, 400)
    w_ = g[100:250]
    reads = [edit(w_, [("D", 30, 1), ("I", 60, other(w_[60])), ("D", 100, 1)]), rev(g, 260, 100),
             fwd(g, 100, 80), rev(g, 100, 120),
             rev(g, 50, 150), fwd(g, 50, 70)]

    def outcome(w):
        assert len(GC.cigar_strings(w["gp"])[0].replace("M", " ").replace("I", " ").replace("D", " ").split()) == 2 * E + 1
        assert [int(x) for x in w["calls"]["tlen"]] == [260, -260, 120, -120, 150, -150] and all(int(f) & 0x2 for f in w["calls"]["flag"])
    return make(reads, [g], [0, 2, 4], outcome)


def _long_read():
    """a read of 1024 bases with a deleted base (the gapped pass's cap) paired with an exact one of 1024"""
    g = rand(216, 2300)
    reads = [edit(g[50:50 + 1025], [("D", 500, 1)]), rev(g, 1200, 1024)]

    def outcome(w):
        assert kinds(w) == ["G", "H"] and int(w["case"]["lens"][1]) == 1024 and w["calls"]["info"]["proper_with_gapped"] == 1 and int(w["calls"]["tlen"][0]) == 2174
    return make(reads, [EMPTY, g], [0], outcome, max_insert=3000, stride=P.blocks_of(1025))


def _singles():
    """no pairing at all (pair_off None): every read is a single read"""
    g = rand(217, 300)
    reads = [fwd(g, 10, 100), rev(g, 100, 100), edit(g[150:251], [("D", 40, 1)]), rand(218, 60)]

    def outcome(w):
        assert [int(f) for f in w["calls"]["flag"]] == [0, 0x10, 0, 0x4] and w["calls"]["info"]["pairs"] == 0 and kinds(w) == ["H", "H", "G", None]
    return make(reads, [g, EMPTY], [], outcome)


def _no_reads():
    def outcome(w):
        assert w["text"] == SC.header(w["pl"]).encode() and w["calls"]["info"]["reads"] == 0
    return make([], [rand(219, 100)], [], outcome)


def _no_targets():
    def outcome(w):
        assert w["text"].startswith(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@PG\t") and w["calls"]["info"]["unplaced"] == 2 and w["calls"]["info"]["pairs_not_unique"] == 1
    return make([rand(221, 100), rand(222, 50)], [], [0], outcome)


CASES = {"proper": _proper, "split_improper": _split_improper, "insert_bound": _insert_bound, "not_unique": _not_unique, "unplaced_and_dead": _unplaced_and_dead,
         "overhang": _overhang, "runs": _runs, "long_read": _long_read, "singles": _singles, "no_reads": _no_reads, "no_targets": _no_targets}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def checked(name):
    """what the checkers say of a case: the Hamming placement, the gapped one, the pair calls with and without it, the SAM text (plain names)"""
    c = case(name)
    pl = P.place(c["rows"], c["lens"], c["pair_off"], *targets(c), **c["place"])
    gp = GC.gapped_banded(c["rows"], c["lens"], pl, *targets(c), **c["gapped"])
    calls = SC.pair_calls(c["lens"], c["pair_off"], pl, gp, c["max_insert"])
    no_gp = SC.pair_calls(c["lens"], c["pair_off"], pl, None, c["max_insert"])
    return dict(case=c, pl=pl, gp=gp, calls=calls, no_gp=no_gp, text=SC.sam(c["rows"], c["lens"], c["pair_off"], pl, gp, calls))


@functools.lru_cache(maxsize=None)
def many_pairs(n_pairs):
    """n_pairs pairs drawn from a pool of 36 distinct ones on one 2 kb target -- exact, with a deleted base, with an overhang, unplaced -- so that
    the expectation can be computed per distinct pair"""
    g = rand(223, 2000)
    pool = []
    for i, a in enumerate(range(0, 1800, 50)):
        plus = fwd(g, a, 64) if i % 3 else edit(g[a:a + 65], [("D", 30, 1)])
        minus = rev(g, a + 100 + i, 50 + i) if i % 4 else rand(300 + i, 50 + i)
        pool.append((minus, plus) if i % 5 == 0 else (plus, minus))
    reads = [x for i in range(n_pairs) for x in pool[(7 * i) % len(pool)]]
    return make(reads, [g], list(range(0, 2 * n_pairs, 2)), None), len(pool)
