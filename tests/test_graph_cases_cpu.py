"""The inputs of tests/graph_cases.py on the CPU: what oracle build + oracle cut + checker make of every read set equals the pinned
figures; reads of rings give one cut cycle per ring whose self-link offset is the ring's length; the checker's invariants hold; the
Python restatement of the reference's triangle cut equals the oracle's on the dense graphs; a self-linked segment is one GFA link."""
import numpy as np
import pytest

import gfa_writer as G
import graph_cases as GC
import oracle_lib as O
import unitig_checker as U
from test_unitig_cpu import check_invariants


@pytest.mark.parametrize("name", sorted(GC.SETS))
def test_pinned_figures(name):
    got = GC.figures(name)
    print(name, got)
    assert got == GC.PINNED[name]
    r = GC.reads_of(name)
    assert GC.sampled_ids(r) == GC.SAMPLED_IDS[name]
    # distinct starts per replicon: no read twice, so no 2-cycle of offset-0 edges
    assert len(set(zip(r.replicon.tolist(), r.start.tolist()))) == len(r.start)
    built, cut = GC.oracle_graphs(name)
    assert (built[:, 2] > 0).all() and len(cut) == len(built) - (GC.PINNED[name]["built"]["edges"] - GC.PINNED[name]["after_cut"]["edges"])


def test_the_sets_are_what_their_comments_say():
    p = GC.PINNED
    for name, s in GC.SETS.items():
        rings = len(s["circular"])
        if s["rings_only"]:
            assert p[name]["after_cut"]["pairs"] == rings and p[name]["after_cut"]["cycles_cut"] == rings, name
            assert p[name]["after_cut"]["unitig_edges"] == 2 * rings, name
            if name != "short_ring_beside_ring":                                 # (whose build has no transitive edge to cut)
                assert p[name]["built"]["pairs"] > rings, name                   # the cut is what makes the rings single cycles
    assert p["rings_and_linear"]["after_cut"]["pairs"] == 3 and p["rings_and_linear"]["after_cut"]["cycles_cut"] == 2
    assert GC.reads_of("rings_and_linear").replicon[0] == 0                      # pair 0 is a ring read: its cycle's smallest pair is 0
    assert (p["ring_with_repeat"]["after_cut"]["pairs"], p["ring_with_repeat"]["after_cut"]["cycles_cut"]) == (3, 0)      # it branches:
    assert p["ring_with_repeat"]["after_cut"]["unitig_edges"] == 8               # repeat -> either arc -> repeat, on both strands
    assert 2 * 120000 >= 1 << 16 and p["ring_400k"]["after_cut"]["longest_nodes"] == 120000
    many, none = GC.SAMPLED_IDS["short_ring_beside_ring"]
    assert none == 0 and many > 50
    assert len(GC.reads_of("short_ring_beside_ring").start) == 6040


@pytest.mark.parametrize("name", sorted(k for k, s in GC.SETS.items() if s["rings_only"]))
def test_ring_facts(name):
    r = GC.reads_of(name)
    for skip in (False, True):
        u = GC.checker(name, True, skip)
        GC.assert_ring_facts(r, u)
        assert u["info"]["isolated_skipped"] == 0
        assert u["info"]["total_nodes"] == len(r.start)


def test_ring_facts_bite():
    """a ring unitig one base short or with a wrong self-link offset does not pass"""
    r = GC.reads_of("ring_20k")
    u = GC.checker("ring_20k", True)
    bad = dict(u, edges=u["edges"].copy())
    bad["edges"][:, 2] += 1
    with pytest.raises(AssertionError):
        GC.assert_ring_facts(r, bad)
    bad = dict(u, words=u["words"].copy())
    bad["words"][len(bad["words"]) // 2] ^= 1
    with pytest.raises(AssertionError):
        GC.assert_ring_facts(r, bad)
    with pytest.raises(AssertionError):
        GC.assert_reads_in_unitigs(r, bad)


@pytest.mark.parametrize("name", sorted(GC.SETS))
def test_invariants(name):
    r = GC.reads_of(name)
    for after_cut in (False, True):
        u = GC.checker(name, after_cut)
        e = GC.oracle_graphs(name)[1 if after_cut else 0]
        check_invariants(r.words, r.lens, e, u, error_free=False)
        GC.assert_reads_in_unitigs(r, u)                                         # (the error-free property, vectorised)
    if name in ("ring_20k", "short_ring_beside_ring"):
        check_invariants(r.words, r.lens, e, u, error_free=True)                 # and read by read where that is quick


@pytest.mark.parametrize("mopp", GC.DENSE_MOPP)
@pytest.mark.parametrize("name", sorted(GC.DENSE))
def test_literal_cut_equals_oracle(name, mopp):
    n, e, _, _ = GC.dense_case(name)
    want = GC.literal_cut(n, e, mopp)
    got = O.cut_triangles(n, e, mopp)
    assert got.shape == want.shape and (got == want).all()
    print(name, mopp, "edges", len(e), "removed", len(e) - len(got))


def test_the_dense_graphs_are_what_their_rows_say():
    removed = 0
    for name, (n, mean_deg, max_off, parallel, loops, hubs) in GC.DENSE.items():
        n_, e, words, lens = GC.dense_case(name)
        assert n_ == n and n % 2 == 0 and (lens == max_off + 1).all()
        key = e[:, 0].astype(np.int64) * n + e[:, 1]
        assert (np.diff(key) >= 0).all() and len(np.unique(e, axis=0)) == len(e)
        assert (e[:, 2] >= 1).all() and e[:, 2].max() == max_off
        assert bool((np.diff(key) == 0).any()) == parallel
        assert bool((e[:, 0] == e[:, 1]).any()) == loops
        deg = np.bincount(e[:, 0], minlength=n)
        assert int((deg >= 100).sum()) == hubs
        U.check(lens, e)                                                         # a legal unitig input
        removed += len(e) - len(O.cut_triangles(n, e, 250))
        assert U.unitigs(words, lens, e)["info"]["compactable"] == 0             # too dense to compact anything;
        assert U.unitigs(words, lens, GC.thinned(name))["info"]["compactable"] > 100   # one edge in ten is not
    assert removed > 1000


def test_self_linked_pair_is_one_gfa_link():
    """segment 0 linked to itself on both strands (what a cut ring is): the - strand's edge sorts first and takes the line"""
    lens = np.array([12, 12], dtype=np.int32)
    words = np.zeros((2, 1), dtype=np.uint32)
    words[1, 0] = 0x00E4E4E4                                                     # ACGT ACGT ACGT
    text, info = G.gfa_bytes(words, lens, np.array([[0, 0, 8], [1, 1, 8]], dtype=np.int32))
    assert text == b"H\tVN:Z:1.0\nS\t0\tACGTACGTACGT\tLN:i:12\nL\t0\t-\t0\t-\t4M\n"
    assert (info["segments"], info["links"], info["links_merged"]) == (1, 1, 1)
    # without its twin in the list the + strand's edge is a link of its own
    text, info = G.gfa_bytes(words, lens, np.array([[1, 1, 8]], dtype=np.int32))
    assert text.endswith(b"L\t0\t+\t0\t+\t4M\n") and (info["links"], info["links_merged"]) == (1, 0)
