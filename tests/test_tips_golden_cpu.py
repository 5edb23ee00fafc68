"""Pins the Python restatement of the dangling-branch removal (tests/tips_checker.py) against the reference's own run
(tools/make_golden_simplifier.py: oracle/_ref/ALGA --threads=1 --serialize=1 leaves the graph after GraphSimplifier::simplifyGraphOld
and logs one count per pass): from the committed graph after the cut, the restated MST step, retainOnlySmallestOffset and the loop give
the reference's dump byte for byte and its counts pass for pass.  The reference's parallel removal skips one randomly chosen edge of a
removal list of c elements when (c - 1) % 3 == 0 or c == 1; the fixtures record which (`keep`), and the test checks that every kept
edge sits in such a pass -- the reference can skip a removal in no other way.
f5_messy is left out: no choice of kept edges reproduced its counts and dump (n5_aftersimplifier.json, "left_out")."""
import gzip
import json
import os

import pytest

import oracle_lib as O
import tips_checker as T


@pytest.mark.parametrize("name", ["f1_cfg1", "f2_err2", "f4_varlen"])
def test_restatement_matches_reference_dump(golden_dir, name):
    c = json.load(open(os.path.join(golden_dir, "n5_aftersimplifier.json")))[name]
    with gzip.open(os.path.join(golden_dir, c["graph_in"]), "rb") as f:
        n, cut = O.parse_graph(f.read())
    g = T.graph_from_edges(n, cut)
    T.remove_short_parallel_paths(g, c["max_offset_parallel_paths_scaled"])
    mst = T.edges_from_graph(g)
    assert len(mst) == c["edges_after_mst"]
    n_pass = len(c["pass_counts"])
    keep = [set() for _ in range(n_pass)]
    for p, a, b in c["keep"]:
        keep[p].add((a, b))
    trace = []
    got, counts = T.remove_dangling_branches(n, mst, c["max_offset_dangling_branches"], keep=keep, trace=trace)
    assert counts == c["pass_counts"]
    with gzip.open(os.path.join(golden_dir, name + ".aftersimplifier.graph.gz"), "rb") as f:
        assert O.graph_bytes(n, got) == f.read()
    assert len(got) == c["edges_after"]
    for p, ks in enumerate(keep):
        found = len(trace[p])
        for x in ks:
            assert x in trace[p] and ((found - 1) % 3 == 0 or found == 1), (p, x, found)
            assert counts[p] == found - 1
    if name != "f1_cfg1":
        assert sum(counts) > 0 and c["keep"]


def test_left_out_fixture_is_named(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "n5_aftersimplifier.json")))
    assert sorted(meta["left_out"]) == ["f5_messy"] and not os.path.exists(os.path.join(golden_dir, "f5_messy.aftersimplifier.graph.gz"))
