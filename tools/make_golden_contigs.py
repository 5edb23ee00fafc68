#!/usr/bin/env python3
"""Golden vectors for the unitig consensus: the reference itself, run as tools/make_golden_simplifier.py runs it (oracle/_ref/ALGA --threads=1
--serialize=1), on the two fixtures whose simplified graph is ONE path (f1_cfg1, f3_paired).  Its `o.fasta` -- a single contig, the output of
Contig::correctSnipsInContig on that path -- goes to tests/golden/<name>.contigs.fasta.gz, and the `*_afterSimplifier.graph` it leaves to
tests/golden/<name>.aftersimplifier.graph.gz where that file does not exist yet (f1's does; it is checked to be the same dump).
tests/test_consensus_cpu.py pins tests/consensus_checker.py to these contigs, tests/test_gpu_consensus.py the device.
Data only: the reference's outputs.  Needs oracle/_ref/ALGA.  usage: tools/make_golden_contigs.py"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "ALGA")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

SETS = ["f1_cfg1", "f3_paired"]


def run_reference(fx, wd):
    f1, f2 = fx.inputs()
    cmd = [REF, "--file1=" + f1, "--threads=1", "--serialize=1", "--output=o.fasta"] + ([("--file2=" + f2)] if f2 else []) + list(fx.meta.get("extra_args", []))
    p = subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    dumps = [f for f in os.listdir(wd) if f.endswith("_afterSimplifier.graph")]
    if len(dumps) != 1 or not os.path.exists(os.path.join(wd, "o.fasta")):
        raise SystemExit("no after-simplifier dump or no contigs for %s:\n%s" % (fx.name, p.stderr[-2000:]))
    return open(os.path.join(wd, dumps[0]), "rb").read(), open(os.path.join(wd, "o.fasta"), "rb").read()


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
    for name in SETS:
        fx = O.Fixture(GOLD, name)
        try:
            with tempfile.TemporaryDirectory() as wd:
                dump, fasta = run_reference(fx, wd)
        finally:
            fx.cleanup()
        records = [r for r in fasta.split(b">") if r]
        if len(records) != 1:
            raise SystemExit("%s: %d contigs, expected the one path" % (name, len(records)))
        graph = os.path.join(GOLD, name + ".aftersimplifier.graph.gz")
        if os.path.exists(graph):
            with gzip.open(graph, "rb") as f:
                assert f.read() == dump, "%s: the after-simplifier dump differs from the stored one" % name
        else:
            with gzip.GzipFile(graph, "wb", mtime=0) as f:
                f.write(dump)
        with gzip.GzipFile(os.path.join(GOLD, name + ".contigs.fasta.gz"), "wb", mtime=0) as f:
            f.write(fasta)
        seq = b"".join(records[0].split(b"\n")[1:])
        print(name, "contig of", len(seq), "nt;", len(O.parse_graph(dump)[1]), "edges after the simplifier")


if __name__ == "__main__":
    main()
