"""The scaffold families of tests/scaffold_fuzz.py without a GPU: scaffold_dicts is the expectation of every family and variant; scaffold_walk equals
it on the families where it finishes in a few seconds (whole_chains, rings, bundle_edges, rivals; wide_span, many_targets and many_scaffolds are
left to the one statement: the walk looks at every link for every bundle and at every bundle for every end, which costs minutes there); what
holds for every result (tests/scaffold_invariants.py); the outcome tuples, written down from the checker; the Python placement equals the
placement a family writes down wherever it has at most 600 targets; and what each family is for, asserted from the checker's result."""
import numpy as np
import pytest

import place_cases as PC
import place_checker as P
import scaffold_checker as SC
import scaffold_fuzz as F
import scaffold_invariants as INV

KEYS7 = ("links", "bundles_supported", "ends_ambiguous", "joins", "joins_dropped_cycle", "scaffolds", "scaffolds_multi")
# (links, bundles_supported, ends_ambiguous, joins, joins_dropped_cycle, scaffolds, scaffolds_multi) of every variant of every case
OUTCOMES = {}


def assert_same(got, want, what=""):
    for k in SC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def dropped(res):
    return [(int(a), int(b)) for a, b, s in zip(res["b_a"], res["b_b"], res["b_state"]) if s & SC.B_DROPPED_CYCLE]


def starts(res):
    n = res["b_links"].astype(np.int64)
    return np.concatenate([[0], np.cumsum(n)[:-1]]), n


@pytest.mark.parametrize("key,i", F.every())
def test_the_two_statements_agree(key, i):
    c, want = F.case(key), F.checked(key, i)
    v = c["variants"][i]
    if key.split("/")[0] in F.WALKED:
        assert_same(SC.scaffold_walk(c["rows"], c["lens"], c["pair_off"], c["written"], **v), want, (key, i))
    INV.every_result(c, c["written"]["info"]["pairs_split"], want, v)
    assert tuple(want["info"][k] for k in KEYS7) == OUTCOMES[key][i], want["info"]
    print(key, i, want["info"])


def test_every_case_is_listed_and_two_thirds_are_walked():
    assert sorted(OUTCOMES) == sorted(F.CASES) and all(len(OUTCOMES[k]) == F.n_variants(k) == len(F.case(k)["variants"]) for k in F.CASES)
    assert sorted(k for f in F.FAMILIES for k in F.KEYS[f]) == sorted(F.CASES)
    both = len(F.every(F.WALKED))
    assert 3 * both >= 2 * len(F.every()), (both, len(F.every()))
    assert len(F.KEYS["whole_chains"]) == 2 * len(F.CHAIN_T) and len(F.KEYS["rings"]) == len(F.RING_M) + 1


@pytest.mark.parametrize("key", [k for k in F.CASES if k.split("/")[0] not in ("many_targets", "many_scaffolds")])
def test_the_python_placement_equals_the_written_one(key):
    c = F.case(key)
    assert len(c["tlen"]) <= F.PLACE_MAX_T
    pl = P.place(*PC.args(c), **c["params"])
    for k in ("target", "pos", "state", "col_off"):
        assert pl[k].dtype == c["written"][k].dtype and (pl[k] == c["written"][k]).all(), (key, k)
    assert pl["info"]["pairs_split"] == c["written"]["info"]["pairs_split"] == len(c["links"])


def test_the_large_families_are_the_ones_without_a_python_placement():
    for key in ("many_targets", "many_scaffolds"):
        assert len(F.case(key)["tlen"]) > F.PLACE_MAX_T
    assert sum(len(F.case(k)["lens"]) // 2 for k in ("many_targets", "many_scaffolds", "wide_span", "bundle_edges", "rivals")) < 5 * 10000
    assert all(int(F.case(k)["tlen"].sum()) <= 2 * 10 ** 6 and len(F.case(k)["lens"]) // 2 <= 10000 for k in F.CASES)


# ---- what each family is for ----------------------------------------------------------------------------------------------------------------
def test_whole_chains_cover_every_target_on_and_around_the_powers_of_two():
    assert F.CHAIN_T == (1, 2, 3, 4, 5, 127, 128, 129, 512, 513)
    for T in F.CHAIN_T:
        for which in ("first", "last"):
            key = "whole_chains/%d/%s" % (T, which)
            c, w = F.case(key), F.checked(key)
            assert len(c["tlen"]) == T and (c["tlen"] > 0).all()
            assert INV.layout(w) == [c["truth"]["path"]] and w["s_off"].tolist() == [0, T] and sorted(w["rank"].tolist()) == list(range(T))
            assert w["info"]["joins"] == T - 1 and (w["b_links"] == 5).all() and len(w["b_links"]) == T - 1
            if T > 1:                                                   # planted from the smaller terminal, or towards it
                planted = c["truth"]["planted"]
                assert (planted[0][0] < planted[-1][0]) == (which == "first") == (planted == c["truth"]["path"])
            if T >= 5:
                assert 0 < int(w["orient"].sum()) < T
    # the device's rounds are ceil(log2(2T)) + 1: 2T on a power of two, one state below and one above, at 2^8 and 2^10
    assert {2 * T for T in F.CHAIN_T} >= {2, 4, 8, 254, 256, 258, 1024, 1026}
    # a chain of T contigs needs ceil(log2 T) doublings before the first state sees the end: one less does not reach it
    for T in (128, 129, 512, 513):
        assert 2 ** (int(np.ceil(np.log2(T))) - 1) < T
    assert F.checked("whole_chains/513/first")["info"]["scaffolds_multi"] == 1 and len(F.checked("whole_chains/513/last")["s_members"]) == 513


def test_rings_are_opened_at_the_left_end_of_their_smallest_contig():
    places, enters = set(), set()
    for key in F.KEYS["rings"]:
        c, w = F.case(key), F.checked(key)
        rr, cc = c["truth"]["rings"], c["truth"]["chains"]
        want = [F.opened(r) for r in rr]
        assert dropped(w) == sorted(k for _, k in want) and w["info"]["joins_dropped_cycle"] == len(rr)
        for (a, b) in dropped(w):
            i = int(np.nonzero((w["b_a"] == a) & (w["b_b"] == b))[0][0])
            assert w["b_state"][i] == SC.B_SUPPORTED | SC.B_JOIN | SC.B_DROPPED_CYCLE
        lay = INV.layout(w)
        for path, (a, b) in want:
            c0 = min(x for x, _ in path)
            assert path in lay and path[0] == (c0, 0) and 2 * c0 in (a, b) and not w["end_state"][2 * c0] & SC.E_JOINED
        for chain in cc:
            assert chain in lay
        assert sum(len(p) for p in lay) == int((c["tlen"] > 0).sum()) and (c["tlen"] == 0).any()
        for r in rr:
            k = min(range(len(r)), key=lambda i: r[i][0])
            places.add(k * 8 // len(r))
            enters.add(r[k][1])
            counts = {int(n) for n, s in zip(w["b_links"], w["b_state"]) if s & SC.B_JOIN}
            assert len(counts) > 1                                      # the joins have different link counts
    assert enters == {0, 1} and len(places) >= 4                        # the smallest contig anywhere in the planted order, entered through either end
    assert [len(F.case("rings/%d" % m)["truth"]["rings"][0]) for m in F.RING_M] == [2, 3, 4, 5, 64, 65, 257]
    c, w = F.case("rings/mixed"), F.checked("rings/mixed")
    assert [len(r) for r in c["truth"]["rings"]] == [2, 3, 5, 9] and [len(x) for x in c["truth"]["chains"]] == [4, 2, 7] and int((c["tlen"] == 0).sum()) == 3
    assert w["info"]["scaffolds"] == 4 + 3 + 6 and w["info"]["scaffolds_multi"] == 7
    # with min_links 6 the joins of 5 links are gone: the ring is a set of chains and nothing is dropped
    for m in F.RING_M:
        assert F.checked("rings/%d" % m, 1)["info"]["joins_dropped_cycle"] == 0


def test_bundle_edges_fall_where_the_kernels_can_go_wrong():
    c, w = F.case("bundle_edges"), F.checked("bundle_edges")
    assert [(int(a), int(b), int(n)) for a, b, n in zip(w["b_a"], w["b_b"], w["b_links"])] == c["truth"]
    assert len(c["tlen"]) == 12 and len(set(w["b_a"].tolist()) | set(w["b_b"].tolist())) == 24
    st, n = starts(w)
    en = st + n
    assert set(F.EDGE_SIZES) <= set(n.tolist()) and F.EDGE_SIZES == (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
    assert len(set((st % 64).tolist())) >= 32                           # the starts on at least 32 lanes
    assert (st % 64 == 63).any()                                        # one on the last lane of a wave
    assert int((st // 256 != (en - 1) // 256).sum()) >= 3               # bundles that cross a block boundary
    behind = [i for i in range(1, len(n)) if n[i] == 1 and n[i - 1] >= 127 and st[i] % 64 != 0]
    assert behind                                                       # a bundle of one link behind a long one inside the same 64 links
    assert any(st[i - 1] // 256 + 2 <= (en[i - 1] - 1) // 256 for i in behind)   # ... and behind one that spans three blocks
    for i, m in enumerate((1, 64, 65, 1001)):
        assert c["variants"][i]["min_links"] == m and F.checked("bundle_edges", i)["info"]["bundles_supported"] == int((n >= m).sum())
    assert F.checked("bundle_edges", 3)["info"]["joins"] == 0 and not F.checked("bundle_edges", 3)["end_state"].any()


def test_wide_span_sums_above_2_to_the_32():
    c, w, w1 = F.case("wide_span"), F.checked("wide_span"), F.checked("wide_span", 1)
    spans = c["truth"]
    assert len(spans) == 4200 and all((1 << 20) - 2000 <= s <= 1 << 20 for s in spans)
    assert w["b_span"].tolist() == [sum(spans)] and sum(spans) > 1 << 32 and w["b_links"].tolist() == [4200] and w["info"]["links_too_far"] == 0
    assert w["b_gap"].tolist() == [(1 << 20) - sum(spans) // 4200] and w["info"]["joins"] == 1
    near = [s for s in spans if s <= F.WIDE_CUT]
    assert c["variants"][1]["max_insert"] == F.WIDE_CUT and w1["info"]["links_too_far"] == 4200 - len(near) > 1000 and len(near) > 1000
    assert w1["b_span"].tolist() == [sum(near)] and w1["b_links"].tolist() == [len(near)]
    assert min(len(t) for t in c["seqs"]) >= 590000


def test_rivals_sit_on_the_boundaries():
    c = F.case("rivals")
    hubs = c["truth"]
    assert len(c["tlen"]) == 200 and 140 <= c["tlen"].min() and c["tlen"].max() <= 200
    w = F.checked("rivals")                                             # min_links 1: every bundle is supported
    degree = np.bincount(np.concatenate([w["b_a"], w["b_b"]]), minlength=400)
    assert degree.max() >= 12 and 330 + sum(len(n) for _, n in hubs) == len(w["b_a"]) and 1 <= w["b_links"].min() and (w["b_links"][w["b_links"] < 13]).max() == 12
    for hub, counts in hubs:                                            # the planted counts are what the checker finds at the hub
        got = sorted(int(n) for a, b, n in zip(w["b_a"], w["b_b"], w["b_links"]) if hub in (a, b))
        assert got == sorted(counts), (hub, got)
    tops = [sorted(n, reverse=True) for _, n in hubs]
    assert sum(1 for n in tops if len(n) >= 3 and n[0] == n[1] == n[2]) >= 3          # ties of three at the top
    assert sum(1 for n in tops if n[0] == n[1] and (len(n) == 2 or n[1] > n[2])) >= 2    # ties between best and second
    for pct in (1, 50, 51, 100):
        assert any(100 * n[1] == pct * n[0] for n in tops), pct
        assert pct == 1 or any(100 * (n[1] + 1) == pct * n[0] for n in tops), pct       # one link less (below 1 % there is no bundle at all)
    seen = set()
    for i, v in enumerate(c["variants"]):
        res = F.checked("rivals", i)
        for hub, counts in hubs:
            sup = sorted((n for n in counts if n >= v["min_links"]), reverse=True)
            amb = len(sup) > 1 and 100 * sup[1] >= v["max_second_percent"] * sup[0]
            st = int(res["end_state"][hub])
            assert bool(st & SC.E_HAS_SUPPORTED) == bool(sup) and bool(st & SC.E_AMBIGUOUS) == amb, (i, hub, counts, st)
            assert bool(st & SC.E_JOINED) == (bool(sup) and not amb), (i, hub, counts, st)      # the other end has this bundle alone
            if len(sup) > 1 and 100 * sup[1] == v["max_second_percent"] * sup[0]:
                seen.add(v["max_second_percent"])
        assert res["info"]["ends_ambiguous"] == int(((res["end_state"] & SC.E_AMBIGUOUS) > 0).sum())
    assert seen == {1, 50, 51, 100}                                     # every percentage has an end exactly on its boundary among the supported
    assert [(v["min_links"], v["max_second_percent"]) for v in c["variants"]] == [(n, p) for n in (1, 3, 5) for p in (1, 50, 51, 100)]


def test_many_targets_make_the_key_wide():
    c, w = F.case("many_targets"), F.checked("many_targets")
    T, t = F.MANY_T, c["truth"]
    assert len(c["tlen"]) == T == 40000 and 2 * T > 1 << 16 and (2 * T).bit_length() == 17       # the ends need 17 bits, the key with its sentinel 50
    assert int((c["tlen"] == 0).sum()) == len(range(3, T, 7)) and (c["tlen"][3::7] == 0).all() and c["tlen"][c["tlen"] > 0].min() >= 30 and c["tlen"].max() <= 60
    keys = {(int(a), int(b)): int(s) for a, b, s in zip(w["b_a"], w["b_b"], w["b_state"])}
    top = (max(a for a, _ in keys) << 32).bit_length()
    assert top == 49 and int(w["b_a"].max()) >= 1 << 16 and int(w["b_a"].min()) <= 1
    for k in t["far"]:                                                  # the first targets joined to the last
        assert keys[k] == SC.B_SUPPORTED | SC.B_JOIN and k[0] < 4 and k[1] >= 2 * (T - 2)
    assert len(t["far"]) == 3 and [0, T - 1] == [t["far"][0][0] >> 1, t["far"][0][1] >> 1]
    for k1, k2 in t["high"]:
        x = ((k1[0] << 32) | k1[1]) ^ ((k2[0] << 32) | k2[1])
        assert k1 in keys and k2 in keys and x in (1 << 15, 1 << 16, 1 << 47, 1 << 48)
    assert {((a[0] << 32 | a[1]) ^ (b[0] << 32 | b[1])) for a, b in t["high"]} == {1 << 15, 1 << 16, 1 << 47, 1 << 48}
    for k1, k2 in t["low"]:
        assert k1 in keys and k2 in keys and ((k1[0] << 32) | k1[1]) ^ ((k2[0] << 32) | k2[1]) in (1, 1 << 32)
    assert len(t["high"]) == len(t["low"]) == 40
    assert all(min(x for x, _ in chain) > F.MANY_HIGH for chain in t["chains"]) and len(t["chains"]) == 150
    lay = {p[0][0]: p for p in INV.layout(w) if len(p) > 1}
    for chain in t["chains"]:
        assert lay[chain[0][0]] == chain
    assert len(t["rings"]) == 4 and w["info"]["joins_dropped_cycle"] == 4 and dropped(w) == sorted(F.opened(r)[1] for r in t["rings"])
    for r in t["rings"]:
        assert lay[min(x for x, _ in r)] == F.opened(r)[0]
    assert min(x for x, _ in t["rings"][3]) < 16000 < F.MANY_HIGH < max(x for x, _ in t["rings"][3])
    assert 2000 <= w["info"]["links"] <= 3500 and len(c["lens"]) // 2 <= 10000


def test_many_scaffolds_make_many_records():
    c, w, w1 = F.case("many_scaffolds"), F.checked("many_scaffolds"), F.checked("many_scaffolds", 1)
    assert len(c["tlen"]) == 3000 and c["tlen"].min() >= 40 and c["tlen"].max() <= 90
    assert INV.layout(w) == c["truth"] == INV.layout(w1) and 800 <= w["info"]["scaffolds"] <= 1000
    assert sorted({len(p) for p in c["truth"]}) == [1, 2, 3, 4, 5, 6] and int(w["orient"].sum()) > 500
    assert set((c["written"]["col_off"][:-1] % 16).tolist()) == set(range(16))               # the contigs begin at every residue of col_off mod 16
    assert set((c["tbegin"] % 16).tolist()) == set(range(16))                                 # ... and of their place in the packed words
    for res, v in ((w, c["variants"][0]), (w1, c["variants"][1])):
        g = res["gap_after"][res["gap_after"] > 0]
        assert (g == v["min_gap"]).any() and (g > v["min_gap"]).any(), v                      # gaps of min_gap and more
    assert F.fasta("many_scaffolds").count(b">") == w["info"]["scaffolds"]


OUTCOMES.update({
    "whole_chains/1/first": [(0, 0, 0, 0, 0, 1, 0)],
    "whole_chains/1/last": [(0, 0, 0, 0, 0, 1, 0)],
    "whole_chains/2/first": [(5, 1, 0, 1, 0, 1, 1)],
    "whole_chains/2/last": [(5, 1, 0, 1, 0, 1, 1)],
    "whole_chains/3/first": [(10, 2, 0, 2, 0, 1, 1)],
    "whole_chains/3/last": [(10, 2, 0, 2, 0, 1, 1)],
    "whole_chains/4/first": [(15, 3, 0, 3, 0, 1, 1)],
    "whole_chains/4/last": [(15, 3, 0, 3, 0, 1, 1)],
    "whole_chains/5/first": [(20, 4, 0, 4, 0, 1, 1)],
    "whole_chains/5/last": [(20, 4, 0, 4, 0, 1, 1)],
    "whole_chains/127/first": [(630, 126, 0, 126, 0, 1, 1)],
    "whole_chains/127/last": [(630, 126, 0, 126, 0, 1, 1)],
    "whole_chains/128/first": [(635, 127, 0, 127, 0, 1, 1)],
    "whole_chains/128/last": [(635, 127, 0, 127, 0, 1, 1)],
    "whole_chains/129/first": [(640, 128, 0, 128, 0, 1, 1)],
    "whole_chains/129/last": [(640, 128, 0, 128, 0, 1, 1)],
    "whole_chains/512/first": [(2555, 511, 0, 511, 0, 1, 1)],
    "whole_chains/512/last": [(2555, 511, 0, 511, 0, 1, 1)],
    "whole_chains/513/first": [(2560, 512, 0, 512, 0, 1, 1)],
    "whole_chains/513/last": [(2560, 512, 0, 512, 0, 1, 1)],
    "rings/2": [(12, 2, 0, 1, 1, 3, 1), (12, 1, 0, 1, 0, 3, 1)],
    "rings/3": [(18, 3, 0, 2, 1, 3, 1), (18, 2, 0, 2, 0, 3, 1)],
    "rings/4": [(27, 4, 0, 3, 1, 3, 1), (27, 3, 0, 3, 0, 3, 1)],
    "rings/5": [(35, 5, 0, 4, 1, 3, 1), (35, 4, 0, 4, 0, 3, 1)],
    "rings/64": [(447, 64, 0, 63, 1, 3, 1), (447, 51, 0, 51, 0, 15, 13)],
    "rings/65": [(455, 65, 0, 64, 1, 3, 1), (455, 52, 0, 52, 0, 15, 13)],
    "rings/257": [(1797, 257, 0, 256, 1, 3, 1), (1797, 205, 0, 205, 0, 54, 52)],
    "rings/mixed": [(167, 29, 0, 25, 4, 13, 7)],
    "bundle_edges": [(4178, 56, 11, 3, 0, 9, 2), (4178, 27, 8, 3, 0, 9, 2), (4178, 21, 7, 3, 0, 9, 2), (4178, 0, 0, 0, 0, 12, 0)],
    "wide_span": [(4200, 1, 0, 1, 0, 1, 1), (2112, 1, 0, 1, 0, 1, 1)],
    "rivals": [
        (3174, 395, 208, 4, 0, 196, 4), (3174, 395, 158, 15, 0, 185, 14), (3174, 395, 140, 23, 0, 177, 19), (3174, 395, 27, 76, 0, 124, 43),
        (3174, 326, 177, 9, 0, 191, 9), (3174, 326, 154, 14, 0, 186, 14), (3174, 326, 139, 22, 0, 178, 19), (3174, 326, 27, 75, 0, 125, 43),
        (3174, 265, 141, 14, 0, 186, 14), (3174, 265, 136, 16, 0, 184, 16), (3174, 265, 125, 22, 0, 178, 19), (3174, 265, 26, 73, 0, 127, 44)],
    "many_targets": [(2480, 797, 40, 713, 4, 33573, 195), (2480, 837, 0, 753, 4, 33533, 235)],
    "many_scaffolds": [(4262, 2131, 0, 2131, 0, 869, 710), (4262, 2131, 0, 2131, 0, 869, 710)],
})
