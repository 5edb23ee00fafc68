"""The Python statement of the unitig graph (tests/unitig_checker.py) against hand-written cases whose answers are written out in
tests/unitig_cases.py, and its invariants on every graph dump of the reference under tests/golden."""
import numpy as np
import pytest

import unitig_cases as K
import unitig_checker as U


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("case", sorted(K.CASES))
def test_hand_written_case(case, skip):
    c = K.CASES[case]
    words, lens = K.nodes_of(c["reads"])
    edges = np.array(c["edges"], dtype=np.int32).reshape(-1, 3)
    K.assert_equals_expected(U.unitigs(words, lens, edges, skip_isolated=skip), case, skip)
    # the order of the edges does not matter
    K.assert_equals_expected(U.unitigs(words, lens, edges[::-1], skip_isolated=skip), case, skip)


@pytest.mark.parametrize("name", sorted(K.REFUSALS))
def test_refusal(name):
    words, lens, edges = K.refusal_nodes(name)
    with pytest.raises(ValueError):
        U.unitigs(words, lens, edges)


def test_odd_node_count_is_refused():
    words, lens = K.nodes_of([K.A8, K.C8])
    with pytest.raises(ValueError):
        U.unitigs(words[:-1], lens[:-1], np.zeros((0, 3), np.int32))


def check_invariants(words, lens, edges, u, error_free):
    """what holds for every unitig graph, whoever computed it"""
    lens = np.asarray(lens, dtype=np.int64)
    live = np.nonzero(lens > 0)[0]
    pn, pp, po = u["path_node"].astype(np.int64), u["path_pos"].astype(np.int64), u["path_off"].astype(np.int64)
    # every live node in exactly one oriented unitig: the `+` paths and their twins partition the live nodes
    both = np.concatenate([pn, pn ^ 1])
    assert len(both) == len(live) and (np.sort(both) == live).all()
    P = u["n_pairs"]
    assert len(po) == P + 1 and po[0] == 0 and po[-1] == len(pn) and (np.diff(po) > 0).all()
    first, last = po[:-1], po[1:] - 1
    assert (pp[first] == 0).all()
    inner = np.ones(len(pn), dtype=bool)
    inner[first] = False
    assert (np.diff(pp)[inner[1:]] >= 0).all()
    assert (u["len"] == pp[last] + lens[pn[last]]).all()
    # numbering: the head of `+` is smaller than the head of the twin path, pairs ascend with it
    assert (pn[first] < (pn[last] ^ 1)).all() and (np.diff(pn[first]) > 0).all()
    # unitig edges: sorted, twin-symmetric
    e = u["edges"].astype(np.int64)
    if len(e):
        key = (e[:, 0] << 32) | e[:, 1]
        assert (np.diff(key) > 0).all()
        ul = np.repeat(u["len"].astype(np.int64), 2)
        tw = np.stack([e[:, 1] ^ 1, e[:, 0] ^ 1, ul[e[:, 1]] - ul[e[:, 0]] + e[:, 2]], axis=1)
        assert set(map(tuple, tw.tolist())) == set(map(tuple, e.tolist()))
    if error_free:
        # every read is a substring of its unitig's sequence at pos
        rows = U.unpack_rows(words, lens)
        for k in range(P):
            seq = np.array([0 if x == "A" else 1 if x == "C" else 2 if x == "G" else 3 for x in U.sequence(u, k)], dtype=np.uint8)
            for i in range(po[k], po[k + 1]):
                r = rows[pn[i]]
                assert (seq[pp[i]: pp[i] + len(r)] == r).all()


@pytest.mark.parametrize("graph", K.GOLDEN_GRAPHS)
def test_reference_dump(golden_dir, graph):
    words, lens, edges = K.golden(golden_dir, graph)
    u = U.unitigs(words, lens, edges)
    check_invariants(words, lens, edges, u, graph.split(".")[0] in K.ERROR_FREE)
    assert u["info"]["cycles_cut"] == 0
    live, sym, oriented, longest = K.GOLDEN_TABLE[graph]
    assert (int((lens > 0).sum()), u["info"]["edges_sym"], 2 * u["n_pairs"], u["info"]["longest_nodes"]) == (live, sym, oriented, longest)
    us = U.unitigs(words, lens, edges, skip_isolated=True)
    assert us["n_pairs"] == u["n_pairs"] - us["info"]["isolated_skipped"]
    if graph == "f1_cfg1.aftercut.graph":
        assert u["n_pairs"] == 1 and us["n_pairs"] == 1          # one segment: the genome
