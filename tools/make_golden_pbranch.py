#!/usr/bin/env python3
"""Golden vectors for the extension of contigs by paired connections: a genome G of 20 kb and a second chromosome Z whose last 140 nt are
G[10000:10140], so that Z's reads run into G and the contracted graph branches there.  Only the pairs tell which predecessor of the junction
continues: the reference, run as tools/make_golden_contigs.py runs it (oracle/_ref/ALGA --threads=1 --serialize=1), marks a reliable
predecessor on the paired input and none on the same reads given as one file, and its two `o.fasta` differ.

tests/golden/f8_pbranch_1 / _2.fasta.gz, .json, .graph.gz       inputs, the reference's numbers and before-simplifier dump (tools/make_golden.py)
tests/golden/f8_pbranch.aftersimplifier.graph.gz                 the dump the contigs start from
tests/golden/f8_pbranch.contigs.fasta.gz                         o.fasta of the paired run
tests/golden/f8_pbranch.single.contigs.fasta.gz                  o.fasta of the single-file run (the mates interleaved)
Data only: the reference's outputs.  Needs oracle/_ref/ALGA.  usage: tools/make_golden_pbranch.py"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "ALGA")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_reads  # noqa: E402
import make_golden  # noqa: E402

NAME, SEED, SHARED = "f8_pbranch", 8, 140
FRAG, LENGTH = 400, 150


def read_set():
    rng = np.random.default_rng(SEED)
    G = rng.integers(0, 4, size=20000, dtype=np.uint8)
    Z = np.concatenate([rng.integers(0, 4, size=3000, dtype=np.uint8), G[10000:10000 + SHARED]])
    a, b = [], []
    for chrom, n in ((G, 3400), (Z, 530)):
        starts = rng.integers(0, len(chrom) - FRAG + 1, size=n)
        swap = rng.random(n) < 0.5
        fr = chrom[starts[:, None] + np.arange(FRAG)[None, :]]
        m1, m2 = fr[:, :LENGTH], gen_reads.revcomp_codes(fr)[:, :LENGTH]
        a.append(np.where(swap[:, None], m2, m1))
        b.append(np.where(swap[:, None], m1, m2))
    a, b = np.concatenate(a), np.concatenate(b)
    perm = rng.permutation(len(a))
    return a[perm].astype(np.uint8), b[perm].astype(np.uint8)


def run(wd, files):
    cmd = [REF, "--file1=" + files[0], "--threads=1", "--serialize=1", "--output=o.fasta"] + (["--file2=" + files[1]] if len(files) > 1 else [])
    p = subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    dumps = [f for f in os.listdir(wd) if f.endswith("_afterSimplifier.graph")]
    if len(dumps) != 1 or not os.path.exists(os.path.join(wd, "o.fasta")):
        raise SystemExit("no after-simplifier dump or no contigs:\n" + p.stderr[-2000:])
    m = re.findall(r"reliablePredecessors\.size\(\): (\d+)", p.stdout + p.stderr)
    return open(os.path.join(wd, dumps[0]), "rb").read(), open(os.path.join(wd, "o.fasta"), "rb").read(), [int(x) for x in m]


def records(fasta):
    return [(r.split(b"\n")[0].decode(), len(b"".join(r.split(b"\n")[1:]))) for r in fasta.split(b">") if r]


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
    a, b = read_set()
    make_golden.emit(NAME, [("/1", make_golden.seqs_from_codes(a)), ("/2", make_golden.seqs_from_codes(b))])
    with tempfile.TemporaryDirectory() as wd:
        gen_reads.write_fasta(os.path.join(wd, NAME + "_1.fasta"), a, suffix="/1")
        gen_reads.write_fasta(os.path.join(wd, NAME + "_2.fasta"), b, suffix="/2")
        dump, paired, rel_p = run(wd, [NAME + "_1.fasta", NAME + "_2.fasta"])
    with tempfile.TemporaryDirectory() as wd:
        both = np.empty((2 * len(a), LENGTH), dtype=np.uint8)
        both[0::2], both[1::2] = a, b
        gen_reads.write_fasta(os.path.join(wd, NAME + ".fasta"), both)
        dump_s, single, rel_s = run(wd, [NAME + ".fasta"])
    print("paired:", records(paired), "reliablePredecessors", rel_p)
    print("single:", records(single), "reliablePredecessors", rel_s)
    if not (rel_p and max(rel_p) >= 1 and max(rel_s + [0]) == 0 and paired != single):
        raise SystemExit("the fixture does not separate the paired run from the single-file run: change SEED")
    for path, data in ((NAME + ".aftersimplifier.graph.gz", dump), (NAME + ".contigs.fasta.gz", paired), (NAME + ".single.contigs.fasta.gz", single)):
        with gzip.GzipFile(os.path.join(GOLD, path), "wb", mtime=0) as f:
            f.write(data)
    meta_path = os.path.join(GOLD, NAME + ".json")
    meta = json.load(open(meta_path))
    meta.update(reliable_predecessors_paired=max(rel_p), reliable_predecessors_single=max(rel_s + [0]), shared_nt=SHARED,
                single_run_same_after_simplifier_dump=bool(dump == dump_s))
    with open(meta_path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    for fn in sorted(os.listdir(GOLD)):
        if fn.startswith(NAME):
            print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    main()
