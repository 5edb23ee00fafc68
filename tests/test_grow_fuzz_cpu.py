"""The families of tests/grow_fuzz.py without a GPU: the two Python statements of the grow stage (tests/grow_checker.py) agree on every family and
variant (`many_targets` and `long_overhangs` on the reduced draws `*_small` of the same generators: the quadratic statement cannot take the
large ones), what holds for every result holds, and every family holds what it was made for, asserted from what it planted and from the
checker's output so that a later change of a generator cannot empty a family in silence.

Measured on one CPU core: the whole file in 18 s, of which the quadratic statement takes 13 s over its 20 variants (0.2 to 1.4 s each: `edges` at
k = 8 and min_anchor = 8 is the slowest, `many_targets_small` and `long_overhangs_small` take 1 s per variant); grow_index takes 0.5 to 0.8 s per
variant of `many_targets` and the placement checker 0.6 s.  The times are recorded, not asserted."""
import time

import numpy as np
import pytest

import grow_checker as GC
import grow_fuzz as F
import place_checker as P

# (candidates, overhanging, voting, bases_added) of every variant of every family
OUTCOMES = {"many_targets": [(3184, 2924, 2924, 16837), (3184, 2924, 2924, 4278), (3184, 2924, 2924, 3386)],
            "many_targets_small": [(183, 177, 177, 1062), (183, 177, 177, 376), (183, 177, 177, 207)],
            "long_overhangs": [(309, 309, 309, 7649), (309, 309, 309, 3885), (309, 309, 309, 7665)],
            "long_overhangs_small": [(71, 71, 71, 1884), (71, 71, 71, 816), (71, 71, 71, 1903)],
            "repeats": [(18, 18, 6, 60), (18, 8, 6, 60), (18, 18, 6, 40)],
            "votes": [(360, 360, 360, 101), (360, 360, 360, 77), (360, 360, 360, 54), (360, 360, 360, 72), (360, 360, 360, 48), (360, 360, 360, 25)],
            "edges": [(45, 44, 44, 228), (51, 50, 50, 259), (49, 47, 47, 236), (45, 41, 41, 228), (45, 44, 44, 37)]}
FLOOR = 3 * 256 + 30                                                 # more than three blocks of 256 threads and a partial one


def assert_same(got, want, name, i):
    diff = F.first_difference(got, want)
    if diff is not None:
        print("family %s variant %d seed %d: first difference (array, index, got, want): %s" % (name, i, F.SEEDS[name], diff))
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (name, i, F.SEEDS[name], k, diff)
    assert got["info"] == want["info"], (name, i, F.SEEDS[name], got["info"], want["info"])


def params(name, i):
    return dict(GC.DEFAULT, **F.case(name)["variants"][i])


@pytest.mark.parametrize("name,i", F.every(set(F.BRUTE.values())))
def test_the_two_statements_agree(name, i):
    c, want = F.case(name), F.checked(name, i)
    t0 = time.time()
    assert_same(GC.grow_bruteforce(c["rows"], c["lens"], F.placed(name), c["seqs"], **c["variants"][i]), want, name, i)
    print(name, i, "grow_bruteforce %.2f s" % (time.time() - t0), want["info"])


@pytest.mark.parametrize("name,i", F.every())
def test_outcomes_and_what_holds_for_every_result(name, i):
    c = F.case(name)
    t0 = time.time()
    want = F.checked(name, i)
    info, p = want["info"], params(name, i)
    print(name, i, "place and grow_index %.2f s (0 when another test computed them)" % (time.time() - t0), info)
    assert (info["candidates"], info["overhanging"], info["voting"], info["bases_added"]) == OUTCOMES[name][i], info
    T, R, G = len(c["tlen"]), len(c["lens"]) // 2, p["max_grow"]
    unplaced = (F.placed(name)["state"] & P.PLACED) == 0
    assert info["candidates"] == int((unplaced & (c["lens"][1::2] >= p["min_anchor"] + 1)).sum())
    assert info["candidates"] >= info["overhanging"] >= info["voting"] and info["multi"] == info["overhanging"] - info["voting"]
    assert info["stops_cover"] + info["stops_percent"] + info["stops_max"] == 2 * T and info["columns_before"] == int(c["tlen"].sum())
    assert info["columns_after"] == info["columns_before"] + info["bases_added"] == int(want["col_off"][-1]) and int(want["e_voters"].sum()) == info["voting"]
    assert ((want["end"] >= 0) == (want["state"] & GC.OVERHANGS > 0)).all() and ((want["over"] > 0) == (want["end"] >= 0)).all() and len(want["end"]) == R
    assert ((want["state"] & GC.VOTES > 0) == (want["hits"] == 1)).all() and (want["left"] <= G).all() and (want["right"] <= G).all()
    assert (want["len"] == c["tlen"] + want["left"].astype(np.int64) + want["right"]).all() and (want["begin"] == want["col_off"][:-1]).all()
    assert (want["left"][c["tlen"] < p["min_anchor"]] == 0).all() and (want["right"][c["tlen"] < p["min_anchor"]] == 0).all()
    votes = np.bincount(want["end"][want["hits"] == 1], weights=np.minimum(want["over"][want["hits"] == 1], G), minlength=2 * T)
    assert (want["count"].reshape(2 * T, G, 4).sum(axis=(1, 2)) == votes).all()
    new = GC.sequences(want)
    for t in range(T):                                               # the old target lies at `left` in the new one
        assert (new[t][int(want["left"][t]):int(want["left"][t]) + int(c["tlen"][t])] == c["seqs"][t]).all()
    assert len(F.fasta(name, i).split(b"\n")) == 2 * int((want["len"] > 0).sum()) + 1


def test_every_family_is_listed():
    assert sorted(OUTCOMES) == sorted(F.CASES) == sorted(F.SEEDS) and all(len(OUTCOMES[n]) == len(F.case(n)["variants"]) for n in F.CASES)
    assert set(F.GPU_FAMILIES) | {"many_targets_small", "long_overhangs_small"} == set(F.CASES) and set(F.BRUTE) == set(F.GPU_FAMILIES)
    assert len(set(F.SEEDS.values())) == len(F.SEEDS)
    for name in F.CASES:
        c = F.case(name)
        assert (c["tbegin"] & 15).tolist() == [3 * i % 16 for i in range(len(c["tbegin"]))]
        again = F.CASES[name]()                                                                 # deterministic
        assert (again["rows"] == c["rows"]).all() and (again["lens"] == c["lens"]).all() and (again["twords"] == c["twords"]).all()


@pytest.mark.parametrize("name", ["many_targets", "many_targets_small"])
def test_many_targets_holds_what_it_is_for(name):
    c, pl = F.case(name), F.placed(name)
    big = name == "many_targets"
    tlen, kinds = c["tlen"].astype(np.int64), np.array(c["made"]["kinds"])
    lens = c["lens"][1::2]
    assert c["variants"] == [dict(min_cover=1), dict(), dict(min_cover=2, max_grow=5)] and set(tlen[:-1].tolist()) <= set(F.TARGET_LENGTHS)
    if big:
        assert set(tlen[:-1].tolist()) == set(F.TARGET_LENGTHS) and len(tlen) >= 900 and len(tlen) + 1 > FLOOR
    W = np.repeat(np.minimum(tlen, int(lens.max()) - 1), 2)                                    # W_e of every end
    eoff = np.concatenate([[0], np.cumsum(W)])
    small_ends = int(((W >= 1) & (W <= 15)).sum())
    assert small_ends >= (20 if big else 2)
    if big:
        assert np.bincount(eoff[:-1][W > 0] >> 4).max() >= 3                                   # three ends begin inside one word of the end array
        assert (tlen.sum() + 15) // 16 > FLOOR and (W.sum() + 15) // 16 > FLOOR
    # what the shuffled order holds beside the overhanging reads
    assert {k: int((kinds == k).sum()) for k in ("long", "inside", "unmatched", "n63", "n64")} == \
        (dict(long=8, inside=40, unmatched=260, n63=30, n64=30) if big else dict(long=8, inside=4, unmatched=6, n63=3, n64=3))
    assert ((pl["state"][kinds == "inside"] & P.PLACED) > 0).all() and ((pl["state"][kinds != "inside"] & P.PLACED) == 0).all()
    assert (lens[kinds == "n63"] == 63).all() and (lens[kinds == "n64"] == 64).all() and (lens[kinds == "long"] == F.LONG_READ).all()
    assert ((lens[kinds == "long"] - 1) // 21 == 66).all() and not (np.diff(np.nonzero(kinds == "long")[0]) == 1).all()   # 66 seeds; short reads between them
    for i in range(3):
        w = F.checked(name, i)
        info = w["info"]
        assert (w["end"][(kinds == "inside") | (kinds == "unmatched") | (kinds == "n63")] == -1).all()
        assert (w["over"][kinds == "n64"] == 1).all() and (w["hits"][kinds == "n64"] == 1).all()
        assert sorted(w["over"][kinds == "long"].tolist()) == list(range(F.LONG_H0, F.LONG_H0 + 8)) and (w["end"][kinds == "long"] == 2 * len(tlen) - 1 - c["made"]["spans"][-1][2]).all()
        assert (w["mm"][kinds == "over"] <= 1).all() and (w["mm"][kinds == "over"] == 1).sum() >= (100 if big else 5) and (w["state"] & GC.MINUS > 0).sum() >= info["voting"] // 3
        assert info["stops_cover"] > 0 and info["stops_percent"] > 0 and info["stops_max"] > 0
        if big:
            assert info["candidates"] > 3 * 1024 + 30 and (info["columns_after"] + 15) // 16 > FLOOR
            assert (w["left"] > 0).sum() >= 100 and (w["right"] > 0).sum() >= 100
    assert F.checked(name, 2)["info"]["stops_max"] > (100 if big else 10) and F.checked(name, 2)["info"]["longest_growth"] == 5


@pytest.mark.parametrize("name", ["long_overhangs", "long_overhangs_small"])
def test_long_overhangs_holds_what_it_is_for(name):
    c = F.case(name)
    assert c["variants"] == [dict(min_cover=1, max_grow=200), dict(min_cover=2, max_grow=65), dict(min_cover=1, max_grow=4096)]
    made = c["made"]
    assert sum(1 for _, _, subs in made if len(subs) == 2) >= len(made) // 4 and max(h for _, h, _ in made) > 128
    for i in range(3):
        w = F.checked(name, i)
        assert w["end"].tolist() == [e for e, _, _ in made] and w["over"].tolist() == [h for _, h, _ in made] and (w["hits"] == 1).all()
        assert (w["over"][w["state"] & GC.VOTES > 0] > 128).any() and w["e_voters"].min() >= 2 and w["e_voters"].max() == 6
        assert w["mm"].max() == 2
    assert F.checked(name, 0)["info"]["longest_growth"] > 64 and F.checked(name, 0)["info"]["stops_max"] > 0
    assert F.checked(name, 1)["info"]["stops_max"] > 0 and F.checked(name, 1)["info"]["longest_growth"] == 65
    assert F.checked(name, 2)["info"]["stops_max"] == 0 and F.checked(name, 2)["info"]["longest_growth"] > 200


def test_repeats_holds_what_it_is_for():
    c = F.case("repeats")
    made = c["made"]
    assert c["variants"] == [dict(min_cover=1, max_occ=65535), dict(min_cover=1), dict(max_occ=65535)] and F.ONE_LETTER >= 10 and F.SHARED >= 64
    for i in (0, 2):                                                 # max_occ 65535: every placement counts
        w = F.checked("repeats", i)
        row = lambda r: (int(w["end"][r]), int(w["over"][r]), int(w["mm"][r]), int(w["hits"][r]), int(w["state"][r]))
        t0, r0 = made["one_letter"]
        assert row(r0) == (2 * t0 + 1, 10, 0, 255, GC.OVERHANGS) and row(r0 + 1) == (2 * t0 + 1, 1, 0, F.ONE_LETTER, GC.OVERHANGS)
        for part, per_end, short in (("period2", 2, 67), ("period3", 3, 70)):
            t0, r0 = made[part]
            assert c["lens"][2 * r0 + 1] == short and all((c["seqs"][t][-99:] == c["seqs"][t0][-99:]).all() for t in range(t0, t0 + F.SHARED))
            assert per_end * F.SHARED <= 255                         # counted whole: the tie goes to the smallest e, there to the smallest h
            assert row(r0) == (2 * t0 + 1, 1, 0, per_end * F.SHARED, GC.OVERHANGS) and row(r0 + 1) == (2 * t0 + 1, 1, 0, per_end * F.SHARED, GC.OVERHANGS | GC.MINUS)
            assert row(r0 + 2) == (2 * t0 + 1, 100 - 99 // per_end * per_end, 0, 255, GC.OVERHANGS) and row(r0 + 3) == (2 * t0 + 1, 100 - 99 // per_end * per_end, 0, 255, GC.OVERHANGS | GC.MINUS)
        assert w["info"]["hits_saturated"] == 5 and w["info"]["seeds_over_max_occ"] == 0
    for i in range(3):
        w = F.checked("repeats", i)
        row = lambda r: (int(w["end"][r]), int(w["over"][r]), int(w["mm"][r]), int(w["hits"][r]), int(w["state"][r]))
        t0, r0 = made["period10"]                                    # two overhangs of one end tie: the smaller h, no vote
        assert row(r0) == (2 * t0 + 1, 20, 0, 2, GC.OVERHANGS) and row(r0 + 1) == (2 * t0 + 1, 20, 0, 2, GC.OVERHANGS | GC.MINUS)
        t0, r0 = made["voters"]
        assert w["e_voters"][2 * t0 + 1] == 3 and w["e_voters"][2 * t0 + 2] == 3 and int(w["e_voters"].sum()) == 6   # nobody else votes
        assert (w["over"][r0:r0 + 6] == [30, 25, 20, 30, 25, 20]).all()
        assert (int(w["right"][t0]), int(w["left"][t0 + 1])) == ((30, 30) if i < 2 else (20, 20)) and int(w["left"].sum() + w["right"].sum()) == w["info"]["bases_added"]
    w = F.checked("repeats", 1)                                      # the default max_occ: the seeds of the repeats are over it, nothing overhangs there
    assert (w["end"][:made["period10"][1]] == -1).all() and w["info"]["seeds_over_max_occ"] > 0 and w["info"]["hits_saturated"] == 0 and w["hits"].max() == 2


# (growth, stop reason) of the end of every entry of VOTE_ENDS at min_cover 1, worked out by hand from the columns planted there
VOTES_BY_HAND = {51: [(16, 0), (5, 1), (16, 0), (16, 0), (11, 1), (10, 1), (16, 0), (11, 1)],
                 80: [(16, 0), (5, 1), (16, 0), (9, 1), (7, 1), (10, 1), (9, 1), (5, 1)],
                 100: [(16, 0), (5, 1), (16, 0), (4, 1), (3, 1), (2, 1), (6, 1), (2, 1)]}


def test_votes_holds_what_it_is_for():
    c = F.case("votes")
    made = c["made"]
    assert c["variants"] == [dict(min_percent=p, min_cover=n) for n in (1, 3) for p in (51, 80, 100)]
    assert [n for n, _, _ in F.VOTE_ENDS] == [1, 2, 3, 5, 20, 64, 65, 200]
    # the engineered columns: 100 top == min_percent cover exactly, and one voter fewer
    cols = lambda j: made[j][1]
    assert cols(3)[4] == (5, 4) and cols(4)[3] == (20, 16) and cols(6)[6] == (65, 52) and cols(7)[2] == (200, 160) and cols(7)[5] == (200, 102)
    assert cols(4)[7] == (20, 15) and cols(6)[9] == (65, 51) and cols(7)[8] == (200, 159) and cols(7)[11] == (200, 101)
    assert cols(1)[5] == (2, 1) and cols(4)[11] == (20, 10) and cols(5)[10] == (64, 32)                 # two bases tied
    assert cols(5)[2] == (64, 63) and cols(7)[13] == (200, 199)                                           # a single dissent
    assert [x[0] for x in cols(2)] == [3] * 8 + [2] * 4 + [1] * 4 and [x[0] for x in cols(7)] == [200] * 14 + [100] * 2
    for i, v in enumerate(c["variants"]):
        w = F.checked("votes", i)
        count = w["count"].reshape(len(w["e_voters"]), 64, 4)
        assert w["e_voters"].max() == 200 and sorted(w["e_voters"].tolist()) == [0] * 8 + [1, 2, 3, 5, 20, 64, 65, 200]
        for j, (e, planted) in enumerate(made):
            assert w["e_voters"][e] == F.VOTE_ENDS[j][0] and e == 2 * j + 1 - j % 2
            assert [(int(x.sum()), int(x.max())) for x in count[e, :len(planted)]] == planted and count[e, len(planted):].sum() == 0
            x, why = len(planted), 0                                 # the first column that fails, from the planted numbers
            for q, (cover, top) in enumerate(planted):
                if cover < v["min_cover"] or 100 * top < v["min_percent"] * cover:
                    x, why = q, 0 if cover < v["min_cover"] else 1
                    break
            got = (int((w["right"] if e & 1 else w["left"])[e >> 1]), int(w["e_stop"][e]))
            assert got == (x, why), (i, j, got, x, why)
            by_hand = VOTES_BY_HAND[v["min_percent"]][j]
            if v["min_cover"] == 3 and j < 3:
                by_hand = [(0, 0), (0, 0), (8, 0)][j]                # the cover falls through 3 at column 8 of the third end
            assert got == by_hand, (i, j, got, by_hand)
        assert (w["left"][1::2].sum(), w["right"][0::2].sum()) == (w["left"].sum(), w["right"].sum())


def test_edges_holds_what_it_is_for():
    c = F.case("edges")
    made, lens = c["made"], c["lens"][1::2]
    one = dict(min_cover=1)
    assert c["variants"] == [one, dict(one, k=8, min_anchor=8), dict(one, k=31, min_anchor=31), dict(one, max_mismatches=0), dict(one, max_grow=1)]
    assert int(lens.max()) == 100
    for i in range(5):
        w = F.checked("edges", i)
        # a == W: the whole target is the anchored part, at either end
        t0, r0 = made["whole"]
        n = len(F.EDGE_W)
        assert (c["tlen"][t0:t0 + n] == F.EDGE_W).all() and (lens[r0:r0 + n] - 4 == c["tlen"][t0:t0 + n]).all() and (c["tlen"][t0:t0 + n] < 99).all()
        assert (w["over"][r0:r0 + n] == 4).all() and (w["end"][r0:r0 + n] == [2 * (t0 + j) + j % 2 for j in range(n)]).all() and (w["mm"][r0:r0 + n] == 0).all()
        # L = min_anchor + 1 and one less; a = k = min_anchor
        t0, r0 = made["bound"]
        assert lens[r0:r0 + 8].tolist() == [64, 63, 32, 31, 9, 8, 40, 40]
        want = {0: [1, 0, 0, 0, 0, 0, 0, 0], 1: [1, 1, 1, 1, 1, 0, 32, 9], 2: [1, 1, 1, 0, 0, 0, 0, 9]}.get(i, [1, 0, 0, 0, 0, 0, 0, 0])
        assert w["over"][r0:r0 + 8].tolist() == want and (w["end"][r0:r0 + 8][np.array(want) > 0] == 2 * t0 + 1).all(), (i, w["over"][r0:r0 + 8])
        assert (w["state"][r0 + 7] & GC.MINUS > 0) == (want[7] > 0)
        # mm at the bound with a mismatch in the last anchored base; the first overhanging base is not the column behind the end
        t0, r0 = made["mm"]
        base = P.codes_of(c["rows"][2 * r0 + 1], 0, 100)
        assert base[70] != 3 - c["seqs"][t0 + 1][98] and t0 + 1 == made["grow1"][0]
        if i == 3:
            assert w["end"][r0:r0 + 5].tolist() == [2 * t0 + 1, -1, -1, -1, -1]
        elif i in (0, 4):
            assert w["end"][r0:r0 + 5].tolist() == [2 * t0 + 1] * 3 + [-1, 2 * t0 + 1] and w["mm"][r0:r0 + 5].tolist() == [0, 1, 2, 0, 2] and (w["over"][r0:r0 + 3] == 30).all()
        # max_grow 1
        t0, r0 = made["grow1"]
        assert (int(w["left"][t0]), int(w["right"][t0])) == ((1, 1) if i == 4 else (35, 30))
        if i == 4:
            assert w["e_stop"][2 * t0] == 2 and w["e_stop"][2 * t0 + 1] == 2 and w["info"]["stops_max"] == w["info"]["ends_grown"] and w["info"]["longest_growth"] == 1
