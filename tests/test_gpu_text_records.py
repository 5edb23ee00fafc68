"""Every text output through the one record writer (alga_amd/csrc/text_record.h), byte for byte against the checkers, on an input whose
records start, begin their sequence and end it at every residue mod 16 of the output buffer: the head and the tail of a record are written
byte by byte, the blocks between 16 bytes at a time, and an input whose records happen to be aligned would hide a wrong head or tail.

66 reads without an edge, each a contig of its own (lengths 21 .. 84, 1000 and 4099): unitigs -> consensus -> final contigs -> the contigs
placed on themselves -> polish -> scaffolds of one contig each.  Scaffolds with gaps and minus strands, trimmed windows, records across chunks
and records without an aligned block are the business of the tests of those stages; so is the contig-numbered consensus FASTA (a contig
result leaves reads without an edge out: this chain does not reach it)."""
import functools

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import final_checker as F
import gfa_writer as G
import place_checker as P
import polish_checker as Q
import scaffold_checker as SC
import unitig_checker as U

LENS = list(range(21, 85)) + [1000, 4099]
NO_EDGES = np.zeros((0, 3), np.int32)
GFA_HEAD = b"H\tVN:Z:1.0\n"
INSERT = 300                                                                     # no pair: the placement has no median to offer


def fasta_marks(text):
    """per record of a FASTA text: the offsets of its first byte, of its first base and of the byte after its last base"""
    marks, at = [], 0
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    for h, s in zip(lines[0:-1:2], lines[1::2]):
        assert h.startswith(b">") and s and set(s) <= set(b"ACGTN")
        marks.append((at, at + len(h) + 1, at + len(h) + 1 + len(s)))
        at += len(h) + len(s) + 2
    return marks


def gfa_marks(text):
    """the same of the segment lines of a GFA text without links, as offsets behind the header line (the host writes that line: the device
    buffer starts behind it)"""
    assert text.startswith(GFA_HEAD)
    marks, at = [], 0
    for line in text[len(GFA_HEAD):].split(b"\n")[:-1]:
        s, name, seq, ln = line.split(b"\t")
        assert s == b"S" and ln == b"LN:i:%d" % len(seq)
        marks.append((at, at + 2 + len(name) + 1, at + 2 + len(name) + 1 + len(seq)))
        at += len(line) + 1
    return marks


def reaches_every_residue(marks):
    return all(len({m[i] & 15 for m in marks}) == 16 for i in range(3))


@functools.lru_cache(maxsize=None)
def expected():
    """the chain by the checkers -> the inputs of every stage and the bytes of every file"""
    rng = np.random.default_rng(20261)
    reads = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in LENS]
    words, lens = P.nodes_of(reads)
    u = U.unitigs(words, lens, NO_EDGES, skip_isolated=False)
    cons = S.consensus_pileup(words, lens, u, 0)
    fin = F.final_contigs(u, cons, 1, 95, 0)
    order = fin["order"].astype(np.int64)
    T = len(LENS)
    assert fin["n_accepted"] == fin["n_written"] == T and fin["len"][order].tolist() == sorted(LENS, reverse=True)
    tbegin = 16 * np.asarray(u["word_off"]).astype(np.int64)[order] + fin["begin"][order]
    tlen = fin["len"][order].astype(np.int32)
    contigs = [P.codes_of(cons["words"], tbegin[j], int(tlen[j])) for j in range(T)]
    rows, rlens = P.nodes_of(contigs)                                            # the reads placed on the contigs: the contigs
    pl = P.place(rows, rlens, None, cons["words"], tbegin, tlen)
    assert pl["t_reads"].tolist() == [1] * T and pl["t_bases"].tolist() == tlen.tolist()
    pol = Q.polish_scatter(rows, rlens, pl, cons["words"], tbegin, tlen)
    sc = SC.scaffold_dicts(rows, rlens, None, pl, insert=INSERT)
    assert len(sc["s_len"]) == T == len(sc["s_members"])
    seqs = ["".join("ACGT"[x] for x in s) for s in Q.sequences(pol)]
    plain = [">contig_id=%d_length=%d" % (j, tlen[j]) for j in range(T)]
    deep = [P.depth_header(j, int(tlen[j]), pl["t_reads"][j], pl["t_bases"][j]) for j in range(T)]
    assert all(d == p + "_reads=1_depth=1.00" for d, p in zip(deep, plain))
    text = lambda heads: "".join("%s\n%s\n" % (h, s) for h, s in zip(heads, seqs)).encode()
    files = {
        "consensus": S.fasta_bytes(u, cons, 1)[0],
        "final": F.fasta_bytes(u, cons, fin)[0],
        "depth": text(deep),
        "polished": text(deep),
        "polished_plain": text(plain),
        "scaffold": SC.fasta(sc, Q.sequences(pol)),
        "gfa": G.gfa_bytes(words, lens, NO_EDGES, twins=True, sequences=True)[0],
    }
    return dict(words=words, lens=lens, rows=rows, rlens=rlens, files=files, pol=pol, T=T)


def assert_the_input_reaches_every_alignment(x, want):
    """from the expected text alone: in each file the first byte of a record, its first base and the byte after its last base take all 16
    residues mod 16, and so do the polished column offsets"""
    for name, text in want.items():
        marks = gfa_marks(text) if name == "gfa" else fasta_marks(text)
        assert len(marks) == x["T"] and reaches_every_residue(marks), name
    assert len({int(c) & 15 for c in x["pol"]["col_off"][:-1]}) == 16


@pytest.mark.gpu
def test_every_output_byte_for_byte(tmp_path):
    x = expected()
    want = x["files"]
    assert_the_input_reaches_every_alignment(x, want)
    words, lens, rows, rlens, T = x["words"], x["lens"], x["rows"], x["rlens"], x["T"]
    eng = alga_amd.Engine(0)
    try:
        got, infos = {}, {}

        def written(name, info):
            got[name], infos[name] = open(str(tmp_path / name), "rb").read(), info

        path = lambda name: str(tmp_path / name)
        written("gfa", eng.write_gfa(path("gfa"), words, lens, NO_EDGES, twins=True, sequences=True))
        u = eng.unitigs(words, lens, NO_EDGES, skip_isolated=False)
        c = eng.unitig_consensus(words, lens, u, min_votes=0)
        written("consensus", eng.write_consensus_fasta(path("consensus"), u, c, min_length=1))
        fin = eng.final_contigs(u, c, 1, 95, 0)
        assert fin.n_accepted == T == fin.n_written
        written("final", eng.write_final_fasta(path("final"), fin))
        pl = eng.place_reads(rows, rlens, final=fin)
        written("depth", eng.write_final_fasta(path("depth"), fin, placements=pl))
        pol = eng.polish(rows, rlens, pl)
        assert (pol.to_host()["col_off"] == x["pol"]["col_off"]).all()
        written("polished", eng.write_final_fasta(path("polished"), fin, placements=pl, polished=pol))
        written("polished_plain", eng.write_final_fasta(path("polished_plain"), fin, placements=pl, polished=pol, depth=False))
        sc = eng.scaffold(rows, rlens, None, pl, insert=INSERT)
        written("scaffold", eng.write_scaffold_fasta(path("scaffold"), pl, sc, polished=pol))
    finally:
        eng.close()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
        assert infos[name]["segments"] == T and infos[name]["bytes"] == len(want[name]) and infos[name]["links"] == 0, name
