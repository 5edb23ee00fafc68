"""The read error correction on the GPU (alga_correct_parsed_reads, alga_correct_reads_device, alga_ingest_corrected_device): rows (every word,
padding included), lengths and every counter but `slices` and the times equal to the Python definition (tests/correct_checker.py) on the cases of
tests/correct_cases.py, through the host-array call and through the in-place call on tensors; slice budgets and directory sizes that change
nothing; refusals that leave the rows alone; files in, corrected node set out; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import correct_cases as CC
import correct_checker as K
from alga_amd.engine import device_view

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got_rows, got_info, want_rows, want_info, what):
    assert got_rows.dtype == np.uint32 and got_rows.shape == want_rows.shape, what
    bad = np.nonzero((got_rows != want_rows).any(axis=1))[0] if got_rows.size else []
    assert len(bad) == 0, (what, "rows differ", bad[:10])
    for k in K.COUNTERS:
        assert got_info[k] == want_info[k], (what, k, got_info[k], want_info[k])


def on_tensors(eng, rows, lens, **params):
    import torch
    dev = torch.device("cuda", eng.device)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32).copy()).to(dev)
    lens_t = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32).copy()).to(dev)
    info = eng.correct_reads_device(rows_t, lens_t, **params)
    assert (lens_t.cpu().numpy() == lens).all()
    return rows_t.cpu().numpy().view(np.uint32).reshape(rows.shape), info


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_device_equals_the_definition(eng, name):
    c = CC.case(name)
    want_rows, want_info = CC.checked(name)
    before = c["rows"].copy()
    rows, info = eng.correct_reads(c["rows"], c["lens"], **c["params"])
    assert (c["rows"] == before).all()
    assert_same(rows, info, want_rows, want_info, (name, "host arrays"))
    rows_t, info_t = on_tensors(eng, c["rows"], c["lens"], **c["params"])
    assert_same(rows_t, info_t, want_rows, want_info, (name, "tensors"))
    print(name, info)
    if info["kmers_total"]:
        assert info["slices"] >= 1


def test_slices_and_directory_change_nothing(eng):
    c = CC.case("rand_k21")
    want_rows, want_info = CC.checked("rand_k21")
    try:
        for slice_keys, dir_bits in ((256, 0), (1 << 28, 4), (1 << 28, 20), (256, 20), (1 << 28, 0)):
            eng.set_option("correct_slice_keys", slice_keys)
            eng.set_option("correct_dir_bits", dir_bits)
            rows, info = eng.correct_reads(c["rows"], c["lens"], **c["params"])
            assert_same(rows, info, want_rows, want_info, (slice_keys, dir_bits))
            assert (info["slices"] > 1) == (slice_keys == 256), info
        # a bin above the budget is a slice of its own
        eng.set_option("correct_slice_keys", 256)
        eng.set_option("correct_dir_bits", 0)
        h = CC.case("heavy")
        rows, info = eng.correct_reads(h["rows"], h["lens"], **h["params"])
        assert_same(rows, info, *CC.checked("heavy"), "heavy, 256 keys a slice")
        assert info["slices"] > 1
    finally:
        eng.set_option("correct_slice_keys", 1 << 28)
        eng.set_option("correct_dir_bits", 0)


def test_refusals_leave_the_rows_alone(eng):
    c = CC.case("two_errors")
    rows, lens = c["rows"], c["lens"]
    wrong_twin = rows.copy()
    wrong_twin[2 * 2, 1] ^= 4                                    # an error-free pair in front of the reads that would be fixed
    short_twin = lens.copy()
    short_twin[2 * 3] -= 1
    for what, r, l, kw in (("twin", wrong_twin, lens, {}), ("lengths", rows, short_twin, {}), ("even k", rows, lens, dict(k=20)), ("k 33", rows, lens, dict(k=33)),
                           ("solid_min 0", rows, lens, dict(solid_min=0))):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.correct_reads(r, l, **kw)
        assert ei.value.code == -1, what
        import torch
        dev = torch.device("cuda", eng.device)
        rows_t = torch.from_numpy(r.view(np.int32).copy()).to(dev)
        lens_t = torch.from_numpy(l.copy()).to(dev)
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.correct_reads_device(rows_t, lens_t, **kw)
        assert ei.value.code == -1, what
        assert (rows_t.cpu().numpy().view(np.uint32) == r).all(), what              # nothing written
    got, info = eng.correct_reads(rows, lens, **c["params"])                         # the engine is usable afterwards
    assert_same(got, info, *CC.checked("two_errors"), "after the refusals")


_files = {}


def file_set(tmp_path_factory):
    """set 1 as a FASTA and as a paired FASTQ, and for each: parse_files -> checker"""
    if not _files:
        d = tmp_path_factory.mktemp("correct_files")
        reads = ["".join("ACGT"[x] for x in r) for r in K.forward_reads(CC.case("rand_k21")["rows"], CC.case("rand_k21")["lens"])]
        fa = str(d / "set1.fasta")
        with open(fa, "w") as f:
            for i, s in enumerate(reads):
                f.write(">r%d\n%s\n" % (i, s))
        half = len(reads) // 2
        fq = [str(d / "set1_1.fastq"), str(d / "set1_2.fastq")]
        for path, part in zip(fq, (reads[:half], reads[half:2 * half])):
            with open(path, "w") as f:
                for i, s in enumerate(part):
                    f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
        for name, (f1, f2) in (("fasta", (fa, None)), ("fastq", (fq[0], fq[1]))):
            pr = alga_amd.parse_files(f1, f2)
            rows, info = K.correct(pr["rows"], pr["len"], k=21, solid_min=3, min_run=1)
            _files[name] = (f1, f2, pr, rows, info)
    return _files


def read_back(ds):
    n, st = ds.n, ds.stride_words
    words = device_view(ds.d_words, (n, st)).cpu().numpy().view(np.uint32).copy()
    lens = device_view(ds.d_len, (n,)).cpu().numpy().copy()
    pair = device_view(ds.d_pair_off, ((n + 3) // 4,)).cpu().numpy().view(np.uint8)[:n].copy()
    return words, lens, pair, (ds.n, ds.stride_words, ds.removed_prefix, ds.removed_short, ds.max_len)


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_corrected_ingest_is_parse_checker_preprocess(eng, tmp_path_factory, kind):
    f1, f2, pr, rows, info = file_set(tmp_path_factory)[kind]
    assert info["runs_fixed"] > 100
    plain = read_back(eng.ingest_device(f1, f2)[0])
    uncorrected = read_back(eng.preprocess_nodes(pr["rows"], pr["len"], pr["remove_pref_reads"], 3 + pr["li_kmer_length"]))
    for a, b in zip(plain, uncorrected):                          # without `correct` the call is what it was
        assert a.shape == b.shape and (a == b).all() if isinstance(a, np.ndarray) else a == b
    want = read_back(eng.preprocess_nodes(rows, pr["len"], pr["remove_pref_reads"], 3 + pr["li_kmer_length"]))
    ds, got_info = eng.ingest_device(f1, f2, correct=dict(k=21, solid_min=3, min_run=1))
    got = read_back(ds)
    for a, b in zip(got, want):
        assert a.shape == b.shape and (a == b).all() if isinstance(a, np.ndarray) else a == b
    for k in K.COUNTERS:
        assert got_info["correct"][k] == info[k], k
    assert got[3][0] != plain[3][0] or not (got[0] == plain[0]).all()                # the correction did change the node set
    assert got_info["paired"] == (kind == "fastq")


def test_command_line_writes_the_corrected_reads(tmp_path_factory, tmp_path):
    f1, f2, pr, rows, info = file_set(tmp_path_factory)["fasta"]
    out = str(tmp_path / "corrected.fasta")
    r = subprocess.run([os.path.join(ROOT, "alga_amd", "bin", "alga_hip"), "--file1=" + f1, "--output=" + str(tmp_path / "o.fasta"), "--serialize=0",
                        "--correct_reads=1", "--correct_k=21", "--correct_solid=3", "--corrected_reads=" + out], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "Reads corrected" in r.stderr and ("%d fixed" % info["runs_fixed"]) in r.stderr
    want = ["".join("ACGT"[x] for x in read) for read in K.forward_reads(rows, pr["len"]) if read is not None and len(read) > 0]
    got = [line for line in open(out).read().split("\n") if line and not line.startswith(">")]
    assert got == want
    r = subprocess.run([os.path.join(ROOT, "alga_amd", "bin", "alga_hip"), "--file1=" + f1, "--output=" + str(tmp_path / "o.fasta"), "--correct_reads=1",
                        "--alga=/nonexistent/ALGA"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "--alga" in r.stderr
