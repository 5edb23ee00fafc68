"""What holds for every scaffold result, whoever computed it (tests/scaffold_checker.py or the device): the counters add up, the bundle keys
ascend, every non-empty target is in exactly one scaffold, the scaffolds are numbered by their first contig and laid out from their smaller
terminal, the lengths are the members' plus the gaps, a joined end is not ambiguous, the rendered FASTA and layout have the sizes the arrays
say.  The two CPU files and the GPU file of the scaffold families call it."""
import numpy as np

import scaffold_checker as SC


def layout(res):
    """the scaffolds as [[(contig, orient)]]"""
    return [[(int(c), int(res["orient"][c])) for c in res["s_members"][int(res["s_off"][j]):int(res["s_off"][j + 1])]] for j in range(len(res["s_len"]))]


def every_result(c, pairs_split, res, v, text=True):
    """c: the case dict, pairs_split: what the placement counted, res: a result with its info, v: the variant's parameters
    text: also render the FASTA and the layout in Python (the GPU file passes False where it has compared the device's bytes already)"""
    info = res["info"]
    tlen = c["tlen"].astype(np.int64)
    assert info["pairs_split"] == pairs_split == info["links"] + info["links_too_far"] == (len(c["links"]) if c["pair_off"] is not None else 0)
    assert int(res["b_links"].sum()) == info["links"] and info["bundles"] == len(res["b_a"]) and (res["b_a"] < res["b_b"]).all()
    keys = (res["b_a"].astype(np.int64) << 32) | res["b_b"]
    assert (np.diff(keys) > 0).all()
    assert ((res["scaffold"] == -1) == (tlen == 0)).all() and ((res["rank"] == -1) == (tlen == 0)).all()
    assert len(res["s_members"]) == int((tlen > 0).sum()) == int(res["s_off"][-1]) and sorted(res["s_members"].tolist()) == np.nonzero(tlen > 0)[0].tolist()
    firsts = [int(res["s_members"][o]) for o in res["s_off"][:-1]]
    assert firsts == sorted(firsts) and all(p[0][0] <= p[-1][0] for p in layout(res))
    assert int(res["s_len"].sum()) == int(tlen.sum()) + int(res["gap_after"].sum()) and info["joins"] == int((res["join_links"] > 0).sum()) == int((res["gap_after"] > 0).sum())
    assert (res["gap_after"][res["gap_after"] > 0] >= v["min_gap"]).all()
    joined = (res["end_state"] & SC.E_JOINED).astype(bool)
    assert int(joined.sum()) == 2 * info["joins"] and not (joined & (res["end_state"] & SC.E_AMBIGUOUS).astype(bool)).any()
    if text:
        # the rendered FASTA: one record per scaffold, as long as s_len says, the gaps as N
        lines = SC.fasta(res, c["seqs"]).decode().split("\n")
        assert lines[-1] == "" and [len(s) for s in lines[1::2]] == res["s_len"].tolist() and sum(s.count("N") for s in lines[1::2]) == int(res["gap_after"].sum())
        assert len(SC.layout_tsv(res, tlen).decode().splitlines()) == len(res["s_members"])
