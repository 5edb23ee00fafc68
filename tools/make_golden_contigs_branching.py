#!/usr/bin/env python3
"""Golden vectors for the contigs of branching graphs: the reference itself, run as tools/make_golden_contigs.py runs it (oracle/_ref/ALGA
--threads=1 --serialize=1), on the two fixtures whose simplified graph branches (f2_err2, f4_varlen).  Its `o.fasta` goes to
tests/golden/<name>.contigs.fasta.gz; the `*_afterSimplifier.graph` it leaves is checked to be the stored dump.  tests/test_contigs_cpu.py holds
tests/contig_checker.py to these contigs, tests/test_gpu_contigs.py the device.
Data only: the reference's outputs.  Needs oracle/_ref/ALGA.  usage: tools/make_golden_contigs_branching.py"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_lib as O  # noqa: E402
from make_golden_contigs import run_reference  # noqa: E402

SETS = ["f2_err2", "f4_varlen"]


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
    for name in SETS:
        fx = O.Fixture(GOLD, name)
        try:
            with tempfile.TemporaryDirectory() as wd:
                dump, fasta = run_reference(fx, wd)
        finally:
            fx.cleanup()
        with gzip.open(os.path.join(GOLD, name + ".aftersimplifier.graph.gz"), "rb") as f:
            assert f.read() == dump, "%s: the after-simplifier dump differs from the stored one" % name
        with gzip.GzipFile(os.path.join(GOLD, name + ".contigs.fasta.gz"), "wb", mtime=0) as f:
            f.write(fasta)
        records = [r for r in fasta.split(b">") if r]
        print(name, [(r.split(b"\n")[0].decode(), len(b"".join(r.split(b"\n")[1:]))) for r in records])


if __name__ == "__main__":
    main()
