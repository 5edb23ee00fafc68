"""What holds for every result of the gapped placement, whatever the input (tests/test_gapped_cpu.py, tests/test_gapped_fuzz_cpu.py): defaults where
a read is not placed, the counters against the arrays, the CIGAR offsets and run counts, every script against its read and target, the cover."""
import numpy as np

import gapped_checker as GC
import place_checker as P


def assert_invariants(c, pl, want, v):
    """c: a case (tests/gapped_cases.py: make), pl: its Hamming placement, want: a result on it, v: the gapped parameters in full"""
    info = want["info"]
    R, E = len(c["lens"]) // 2, v["max_edits"]
    st, lens, tlen = want["state"], c["lens"][1::2], c["tlen"]
    on = (st & GC.PLACED) > 0
    assert list(GC.COUNTERS) == list(info) and not (on & ((pl["state"] & P.PLACED) > 0)).any()
    assert ((want["target"] >= 0) == on).all() and ((want["pos"] >= 0) == on).all() and ((want["end"] >= 0) == on).all() and (want["edits"][~on] == 0).all() and (st[~on] == 0).all()
    assert (want["edits"] <= E).all() and int(want["edits"].sum()) == info["edits"] and int(on.sum()) == info["placed"] and int(((st & GC.UNIQUE) > 0).sum()) == info["unique"]
    off = want["cigar_off"].astype(np.int64)
    assert len(off) == R + 1 and off[0] == 0 and int(off[-1]) == len(want["cigar"]) and ((off[1:] - off[:-1] > 0) == on).all() and (off[1:] - off[:-1] <= 2 * E + 1).all()
    extra = np.zeros(int(tlen.sum()), np.int64)
    for r in np.nonzero(on)[0]:
        runs = [(int(x) >> 2, int(x) & 3) for x in want["cigar"][off[r]:off[r + 1]]]
        t, p, e = int(want["target"][r]), int(want["pos"][r]), int(want["end"][r])
        assert 0 <= p < e <= int(tlen[t]) and all(n > 0 for n, _ in runs) and all(a[1] != b[1] for a, b in zip(runs, runs[1:]))
        assert sum(n for n, op in runs if op != GC.OP_D) == int(lens[r]) and sum(n for n, op in runs if op != GC.OP_I) == e - p
        indel = sum(n for n, op in runs if op != GC.OP_M)
        assert indel <= int(want["edits"][r]) and (indel > 0) == bool(st[r] & GC.INDEL)
        # the script applied to the target gives the read but for edits - indel substitutions
        node = P.codes_of(c["rows"][2 * r + (0 if st[r] & GC.MINUS else 1)], 0, int(lens[r]))
        tc, i_r, i_t, subs = c["seqs"][t], 0, p, 0
        for n, op in runs:
            if op == GC.OP_M:
                subs += int((node[i_r:i_r + n] != tc[i_t:i_t + n]).sum())
            i_r, i_t = i_r + (n if op != GC.OP_D else 0), i_t + (n if op != GC.OP_I else 0)
        assert subs + indel == int(want["edits"][r])
        if st[r] & GC.UNIQUE:
            extra[int(pl["col_off"][t]) + p:int(pl["col_off"][t]) + e] += 1
    assert (want["cover"].astype(np.int64) == pl["cover"].astype(np.int64) + extra).all()
    assert len(GC.tsv(want).splitlines()) == info["placed"]
