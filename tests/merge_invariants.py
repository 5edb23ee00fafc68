"""What holds for every result of the merge stage, whatever the input (tests/test_merge_cpu.py, tests/test_merge_fuzz_cpu.py): the counters against
the arrays, a join is mutual and unique at both ends, every non-empty target is a member once, the merged contigs are numbered by their first
contig, every merged contig holds its members' bases where the layout says but for the mismatches of its joins, the FASTA and the TSV."""
import numpy as np

import merge_checker as MC
import place_checker as P


def assert_invariants(c, want, v):
    """c: a case (tests/merge_cases.py: _make), want: a result on it, v: the parameters of the call that differ from the defaults"""
    info = want["info"]
    # what holds for every result
    T, tlen = len(c["tlen"]), c["tlen"].astype(np.int64)
    p = dict(MC.DEFAULT, **v)
    J, D = MC.JOINED, MC.DROPPED_CYCLE
    st = want["end_state"]
    assert list(MC.COUNTERS) == list(info) and info["columns_before"] == int(tlen.sum()) and info["columns_after"] == info["columns_before"] - info["bases_removed"]
    assert info["columns_after"] == int(want["col_off"][-1]) == int(want["len"].sum()) and (want["begin"] == want["col_off"][:-1]).all()
    assert ((want["partner"] >= 0) == (want["hits"] > 0)).all() and ((st & MC.HAS_OVERLAP > 0) == (want["hits"] > 0)).all() and ((st & MC.AMBIGUOUS > 0) == (want["hits"] > 1)).all()
    assert int((st & J > 0).sum()) == 2 * info["joins"] and int((st & D > 0).sum()) == 2 * info["joins_dropped_cycle"] and not (st & J & (st & D) >> 1).any()
    assert ((want["olen"] >= p["min_overlap"]) | (want["hits"] == 0)).all() and (want["olen"] <= p["max_overlap"]).all() and (want["mm"] <= p["max_mismatches"]).all()
    assert ((want["merged"] >= 0) == (tlen > 0)).all() and ((want["rank"] >= 0) == (tlen > 0)).all() and info["merged"] == len(want["len"]) == int((want["rank"] == 0).sum())
    assert int(want["m_off"][-1]) == len(want["m_members"]) == int((tlen > 0).sum()) and int(want["overlap_after"].sum()) == info["bases_removed"]
    assert sorted(want["m_members"].tolist()) == [t for t in range(T) if tlen[t] > 0]
    firsts = [int(want["m_members"][int(o)]) for o in want["m_off"][:-1]]
    assert firsts == sorted(firsts)                                              # numbered by the ascending id of the first contig
    for x in np.nonzero(st & J)[0]:                                              # a join is mutual, unique at both ends, at one o, between two targets
        y = int(want["partner"][x])
        assert want["partner"][y] == x and want["hits"][x] == want["hits"][y] == 1 and want["olen"][x] == want["olen"][y] and want["mm"][x] == want["mm"][y] and y >> 1 != x >> 1
    # every merged contig holds its members' bases where the layout says, but for the mismatches of its joins
    new = MC.sequences(want)
    diff = 0
    for t in range(T):
        if tlen[t]:
            s = P.revcomp(c["seqs"][t]) if want["orient"][t] else c["seqs"][t]
            diff += int((new[int(want["merged"][t])][int(want["start"][t]):int(want["start"][t]) + len(s)] != s).sum())
    assert diff == info["join_mismatches"]
    text = MC.fasta(want).decode().split("\n")
    assert text[-1] == "" and [len(s) for s in text[1::2]] == want["len"].tolist()
    assert len(MC.merge_tsv(want, c["tlen"]).decode().splitlines()) == int((tlen > 0).sum())
