"""GFA 1.0 export without a GPU: the library exports the entry point, and the Python statement of the format (tests/gfa_writer.py,
the checker of the device writer) gives the expected text on hand-made cases and round-trips the golden graphs."""
import numpy as np
import pytest

import alga_amd
import gfa_writer as G
import oracle_lib as O

ACGT = {c: i for i, c in enumerate("ACGT")}


def _rows(seqs):
    L = max(len(s) for s in seqs)
    codes = np.zeros((len(seqs), max(L, 1)), np.uint8)
    for i, s in enumerate(seqs):
        codes[i, : len(s)] = [ACGT[c] for c in s]
    lens = np.array([len(s) for s in seqs], np.int32)
    return alga_amd.pack_reads(codes, lens), lens


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _twin_nodes(reads):
    """ALGA's layout: node 2k = reverse complement of read k, node 2k+1 = read k ('' = removed pair)"""
    seqs = []
    for r in reads:
        seqs += [_revcomp(r), r]
    return _rows(seqs)


def test_library_exports_write_gfa_device():
    lib = alga_amd.load_library()
    assert hasattr(lib, "alga_write_gfa_device")
    assert "alga_write_gfa_device" in alga_amd.engine.EXPORTS
    assert lib.alga_abi_version() == 7


def test_twin_layout_hand_made():
    # read 2 is a removed pair (len 0), read 3 is contained in read 0
    words, lens = _twin_nodes(["ACGTAC", "TACGGA", "", "CGT"])
    edges = np.array([[0, 3, 1],      # twin (2, 1, 1) missing: written on its own
                      [1, 0, 3],      # self-twin (dst == src ^ 1): written once
                      [1, 3, 2],      # twin (2, 0, 2) present and sorts after it: this edge takes the line
                      [1, 7, 1],      # contained read: overlap len[1] - 1
                      [2, 0, 2]],     # twin (1, 3, 2) sorts first: merged into its line
                     np.int32)
    text, info = G.gfa_bytes(words, lens, edges)
    assert text == (b"H\tVN:Z:1.0\n"
                    b"S\t0\tACGTAC\tLN:i:6\n"
                    b"S\t1\tTACGGA\tLN:i:6\n"
                    b"S\t3\tCGT\tLN:i:3\n"
                    b"L\t0\t-\t1\t+\t5M\n"
                    b"L\t0\t+\t0\t-\t3M\n"
                    b"L\t0\t+\t1\t+\t4M\n"
                    b"L\t0\t+\t3\t+\t5M\n")
    assert info == dict(segments=3, links=4, links_merged=1, bytes=len(text))
    text2, _ = G.gfa_bytes(words, lens, edges, sequences=False)
    assert b"S\t0\t*\tLN:i:6\n" in text2 and b"ACGT" not in text2
    # every link expands into the edge list plus the twins the list lacks
    got = G.expand_links(text, lens)
    have = set(map(tuple, edges.tolist()))
    assert have <= got
    assert got - have == {(2, 1, 1), (6, 0, -2)}


def test_plain_layout_hand_made():
    words, lens = _rows(["ACG", "", "TT"])
    edges = np.array([[0, 2, 1], [2, 0, 1]], np.int32)
    text, info = G.gfa_bytes(words, lens, edges, twins=False)
    assert text == b"H\tVN:Z:1.0\nS\t0\tACG\tLN:i:3\nS\t2\tTT\tLN:i:2\nL\t0\t+\t2\t+\t2M\nL\t2\t+\t0\t+\t1M\n"
    assert info["links_merged"] == 0
    assert G.expand_links(text, lens, twins=False) == {(0, 2, 1), (2, 0, 1)}


def test_refusals():
    words, lens = _twin_nodes(["ACGTAC", "TACGGA"])
    with pytest.raises(ValueError):
        G.gfa_bytes(words, lens, np.array([[1, 3, 2], [0, 3, 1]], np.int32))            # unsorted
    with pytest.raises(ValueError):
        G.gfa_bytes(words, lens, np.array([[0, 4, 1]], np.int32))                       # id out of range
    with pytest.raises(ValueError):
        G.gfa_bytes(words[:3], lens[:3], np.zeros((0, 3), np.int32))                  # odd n in the twin layout
    G.gfa_bytes(words[:3], lens[:3], np.zeros((0, 3), np.int32), twins=False)


@pytest.mark.parametrize("name", ["f1_cfg1", "f3_paired", "f4_varlen", "f6_l40"])
def test_golden_graph_round_trip(golden_dir, name):
    """The links of a golden graph, each expanded into both of its edges, are the dump's edge set plus the twins the reduction's
    per-source caps dropped from it."""
    fx = O.Fixture(golden_dir, name)
    try:
        f1, f2 = fx.inputs()
        lo, rs = fx.explicit_params()
        nd = O.ingest(f1, f2, min_overlap=lo, rsoemo=rs)
    finally:
        fx.cleanup()
    n, e = O.parse_graph(fx.ref_graph())
    text, info = G.gfa_bytes(nd["words"], nd["len"], e)
    have = set(map(tuple, e.tolist()))
    lens = nd["len"].astype(np.int64)
    lacking = {(b ^ 1, a ^ 1, int(lens[b] - lens[a]) + o) for a, b, o in have} - have
    assert G.expand_links(text, nd["len"]) == have | lacking
    assert info["links"] + info["links_merged"] == len(e)
    assert info["segments"] == int((nd["len"][1::2] > 0).sum())
