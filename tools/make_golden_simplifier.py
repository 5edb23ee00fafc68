#!/usr/bin/env python3
"""Golden vectors for the dangling-branch removal: the reference itself, run as tools/make_golden.py runs
it (oracle/_ref/ALGA --threads=1 --serialize=1), also leaves `*_afterSimplifier.graph`, the graph after the whole
GraphSimplifier::simplifyGraphOld (src/Params.cpp:393, src/main.cpp:393-400) -> tests/golden/<name>.aftersimplifier.graph.gz, and prints one
`dangling branches removed, N branches removed` line per pass -> tests/golden/n5_aftersimplifier.json, with the bound and the `keep` edges.

`keep`: the reference's parallel removal leaves out one randomly chosen element of a pass's removal list when the list has c elements with
(c - 1) % 3 == 0 or c == 1 (one thread; tests/tips_checker.py).  Which one is found here pass by pass: wherever the reference's count is
one below what the restatement finds, every found edge of that pass is tried in turn (those still in the reference's final graph first)
and the first with which all later counts and the final graph agree is recorded.  A fixture for which no bound near the derived one and
no such choice reproduces the dump is left out and named under "left_out".
Data only: the reference's outputs.  Needs oracle/_ref/ALGA.  usage: tools/make_golden_simplifier.py"""
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import tips_checker as T  # noqa: E402

SETS = ["f1_cfg1", "f2_err2", "f4_varlen", "f5_messy"]
MOPP = {"f1_cfg1": 250}                                      # max(250, int(1.75 * LEN)); 262 for the 150-bp sets (tools/make_golden_n3.py)


def run_reference(fx, wd):
    f1, f2 = fx.inputs()
    cmd = [REF, "--file1=" + f1, "--threads=1", "--serialize=1", "--output=o.fasta"] + ([("--file2=" + f2)] if f2 else []) + list(fx.meta.get("extra_args", []))
    p = subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    dumps = [f for f in os.listdir(wd) if f.endswith("_afterSimplifier.graph")]
    if len(dumps) != 1:
        raise SystemExit("no after-simplifier dump for %s:\n%s" % (fx.name, p.stderr[-2000:]))
    counts = [int(x) for x in re.findall(r"dangling branches removed, (\d+) branches removed", p.stderr)]
    return open(os.path.join(wd, dumps[0]), "rb").read(), counts


def start_graph(name, bound_mst):
    with gzip.open(os.path.join(GOLD, name + ".aftercut.graph.gz"), "rb") as f:
        n, cut = O.parse_graph(f.read())
    g = T.graph_from_edges(n, cut)
    T.remove_short_parallel_paths(g, bound_mst)
    return n, cut, T.edges_from_graph(g)


def derive_keep_from(n, edges, bound, ref_counts, ref_final, keep):
    """-> one keep set per pass, or None: `keep` holds the sets of the passes settled so far"""
    final_set = set(map(tuple, ref_final[:, :2].tolist()))
    trace = []
    got, counts = T.remove_dangling_branches(n, edges, bound, keep=list(keep), trace=trace)
    if counts == ref_counts and np.array_equal(got, ref_final):
        return keep + [set()] * (len(ref_counts) - len(keep))
    p = next((i for i in range(min(len(counts), len(ref_counts))) if counts[i] != ref_counts[i]), None)
    if p is None or p < len(keep):
        return None
    c = len(trace[p])
    if ref_counts[p] != counts[p] - 1 or not ((c - 1) % 3 == 0 or c == 1):
        return None
    for x in sorted(trace[p], key=lambda x: x not in final_set):
        trial = keep + [set()] * (p - len(keep)) + [{x}]
        rest = derive_keep_from(n, edges, bound, ref_counts, ref_final, trial)
        if rest is not None:
            return rest
    return None


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
    meta, left_out = {}, {}
    for name in SETS:
        fx = O.Fixture(GOLD, name)
        try:
            with tempfile.TemporaryDirectory() as wd:
                dump, ref_counts = run_reference(fx, wd)
            f1, f2 = fx.inputs()
            lens = O.ingest(f1, f2)["len"]
        finally:
            fx.cleanup()
        n_ref, ref_final = O.parse_graph(dump)
        mopp = MOPP.get(name, 262)
        with gzip.open(os.path.join(GOLD, name + ".aftercut.graph.gz"), "rb") as f:
            n, cut = O.parse_graph(f.read())
        assert n == n_ref == len(lens)
        live = np.zeros(n, dtype=bool)
        live[cut[:, 0]] = True; live[cut[:, 1]] = True
        avg = float(lens[live & (lens > 0)].astype(np.float64).mean())
        bound = int(mopp * avg / np.float32(100))                            # both steps use this value (MAX_OFFSET_PARALLEL_PATHS == .._DANGLING_BRANCHES)
        n, cut, mst = start_graph(name, bound)
        ref_sorted = ref_final[np.lexsort((ref_final[:, 2], ref_final[:, 1], ref_final[:, 0]))]
        keep = derive_keep_from(n, mst, bound, ref_counts, ref_sorted, [])
        if keep is None or O.graph_bytes(n, T.remove_dangling_branches(n, mst, bound, keep=list(keep))[0]) != dump:
            left_out[name] = "bound %d (mean live read length %.3f): no choice of kept edges reproduces the reference's counts %s and dump" % (bound, avg, ref_counts)
            print(name, "LEFT OUT:", left_out[name])
            continue
        with gzip.GzipFile(os.path.join(GOLD, name + ".aftersimplifier.graph.gz"), "wb", mtime=0) as f:
            f.write(dump)
        meta[name] = dict(graph_in=name + ".aftercut.graph.gz", max_offset_parallel_paths_scaled=bound, max_offset_dangling_branches=bound,
                          avg_read_length=avg, pass_counts=ref_counts, edges_after_mst=len(mst), edges_after=len(ref_final),
                          keep=[[p, int(a), int(b)] for p, ks in enumerate(keep) for a, b in sorted(ks)])
        print(name, {k: v for k, v in meta[name].items()})
    meta["left_out"] = left_out
    json.dump(meta, open(os.path.join(GOLD, "n5_aftersimplifier.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
