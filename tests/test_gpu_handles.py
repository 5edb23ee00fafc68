"""The provenance of the handles a stage is given (alga_placement_is_current, alga_gapped_is_current, alga_polished_is_current of
alga_amd/csrc/stage_common.h): a copy of the current alga_placements, alga_gapped or alga_polished that differs in ONE field -- any size, any
pointer, also those no stage reads -- is refused by every consumer with code -1, on the host (the text is the host predicate's, which no device
verdict shares), no file is touched, and afterwards every consumer gives with the genuine handles what it gave before.  On the smallest paired
case of tests/sam_cases.py."""
import copy

import numpy as np
import pytest

import alga_amd
import sam_cases as SQ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def altered(handle, wrapper_cls):
    """(field, value, a copy of `handle` whose C struct differs in that field alone) for every field: a size +-1 (n_reads also +-2), a pointer
    plus one element"""
    item = {"d_" + k[0]: np.dtype(k[2]).itemsize for k in wrapper_cls.KEYS}
    item["d_counts"] = 4
    for field, ctype in handle._c._fields_:
        old = getattr(handle._c, field) or 0
        if field.startswith("n_"):
            deltas = (1, -1, 2, -2) if field == "n_reads" else (1, -1)
        else:
            deltas = (item[field],)
        for d in deltas:
            f = copy.copy(handle)
            f._c = type(handle._c).from_buffer_copy(handle._c)
            setattr(f._c, field, old + d)
            assert [k for k, _ in f._c._fields_ if getattr(f._c, k) != getattr(handle._c, k)] == [field]
            yield field, d, f


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k, w in want.items():
        if k == "info":
            assert {a: b for a, b in got[k].items() if not a.startswith("ms_")} == {a: b for a, b in w.items() if not a.startswith("ms_")}, (what, k)
        elif w is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and (got[k] == w).all(), (what, k)


def test_a_handle_altered_in_one_field_is_refused_on_the_host(eng, tmp_path):
    c = SQ.case("proper")
    rows, lens, po, tg = c["rows"], c["lens"], c["pair_off"], SQ.targets(c)
    path, other_path = str(tmp_path / "r.sam"), str(tmp_path / "untouched")
    open(other_path, "wb").write(b"kept")
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, **c["place"])
    assert pl.n_reads >= 4 and pl.n_targets >= 2 and pl.n_columns >= 2 and pl.n_hist >= 2       # every size - 1 (n_reads - 2) is still a size

    def every_consumer():
        """the eight consumers of `pl` with the genuine handles -> what they gave (host copies), the handles of the last three stages"""
        r = {}
        pol = eng.polish(rows, lens, pl, counts=True)
        r["polish"] = pol.to_host()
        scaf = eng.scaffold(rows, lens, po, pl, insert=300)
        r["scaffold"] = scaf.to_host()
        r["break_contigs"] = eng.break_contigs(rows, lens, po, pl, polished=pol, margin=0).to_host()
        r["grow_ends"] = eng.grow_ends(rows, lens, pl, polished=pol).to_host()
        gp = eng.place_gapped(rows, lens, pl, targets=tg, **c["gapped"])
        r["place_gapped"] = gp.to_host()
        r["polish_indels"] = eng.polish_indels(rows, lens, pl, gp).to_host()
        calls = eng.judge_pairs(rows, lens, pl, gapped=gp, pair_off=po, max_insert=c["max_insert"])
        r["judge_pairs"] = calls.to_host()
        eng.write_sam(path, rows, lens, pl, calls, gapped=gp)
        r["write_sam"] = dict(text=np.frombuffer(open(path, "rb").read(), dtype=np.uint8))
        eng.write_scaffold_fasta(path, pl, scaf, polished=pol)
        r["write_scaffold_fasta"] = dict(text=np.frombuffer(open(path, "rb").read(), dtype=np.uint8))
        return r, pol, scaf, gp, calls
    before, pol, scaf, gp, calls = every_consumer()
    assert before["place_gapped"]["info"]["placed"] >= 1 and pol._c.d_counts

    consumers = {
        "placement": (pl, type(pl), {
            "polish": lambda f: eng.polish(rows, lens, f),
            "scaffold": lambda f: eng.scaffold(rows, lens, po, f, insert=300),
            "break_contigs": lambda f: eng.break_contigs(rows, lens, po, f, margin=0),
            "grow_ends": lambda f: eng.grow_ends(rows, lens, f),
            "place_gapped": lambda f: eng.place_gapped(rows, lens, f, targets=tg, **c["gapped"]),
            "polish_indels": lambda f: eng.polish_indels(rows, lens, f, gp),
            "judge_pairs": lambda f: eng.judge_pairs(rows, lens, f, gapped=gp, pair_off=po, max_insert=c["max_insert"]),
            "write_sam": lambda f: eng.write_sam(other_path, rows, lens, f, calls, gapped=gp)}),
        "gapped": (gp, type(gp), {
            "polish_indels": lambda f: eng.polish_indels(rows, lens, pl, f),
            "judge_pairs": lambda f: eng.judge_pairs(rows, lens, pl, gapped=f, pair_off=po, max_insert=c["max_insert"]),
            "write_sam": lambda f: eng.write_sam(other_path, rows, lens, pl, calls, gapped=f)}),
        # no field of alga_polished is exempt: the shared check ignores none (the copies it replaced looked at the sizes and d_words alone)
        "polished": (pol, type(pol), {
            "grow_ends": lambda f: eng.grow_ends(rows, lens, pl, polished=f),
            "break_contigs": lambda f: eng.break_contigs(rows, lens, po, pl, polished=f, margin=0),
            "write_scaffold_fasta": lambda f: eng.write_scaffold_fasta(other_path, pl, scaf, polished=f)}),
    }
    wrong, n = [], 0
    for kind, (handle, cls, calls_of) in consumers.items():
        fields = set()
        for field, delta, forged in altered(handle, cls):
            fields.add(field)
            for name, call in calls_of.items():
                n += 1
                try:
                    call(forged)
                    wrong.append((kind, field, delta, name, "accepted"))
                except alga_amd.AlgaError as err:
                    if err.code != -1 or "not the result of the last" not in str(err):
                        wrong.append((kind, field, delta, name, str(err)))
        assert fields == {k for k, _ in handle._c._fields_}, kind                   # every field was altered, also those no stage reads
    print(n, "calls;", len(wrong), "not refused by the host predicate:", wrong)
    assert not wrong, wrong
    assert n == 8 * (4 * 2 + 2 + 12) + 3 * (4 * 2 + 2 + 11) + 3 * (3 * 2 + 7)
    assert open(other_path, "rb").read() == b"kept"
    # the results at hand are as they were (the gapped result and the calls were the inputs of the refused calls; the polish is read back), and
    # every consumer gives with the genuine handles what it gave before
    same(pol.to_host(), before["polish"], "the polish at hand")
    same(gp.to_host(), before["place_gapped"], "the gapped result at hand")
    same(calls.to_host(), before["judge_pairs"], "the calls at hand")
    after = every_consumer()[0]
    for name in before:
        same(after[name], before[name], name)
