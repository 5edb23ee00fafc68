"""Unitig consensus timings (alga_unitig_consensus_device, alga_write_consensus_fasta_device): the graph of a BASELINE config, built on the
device (supplemented when the config has errors), cut by the first simplifier step, optionally without its short parallel paths and tips,
compacted into unitigs without isolated reads; then the consensus of every unitig and the FASTA of the windows into a scratch directory
(deleted afterwards).
    python tools/consensus_measure.py [--config cfg2_1M_150bp] [--repeat 3] [--paths] [--clip] [--min-votes 3] [--min-length 200]
                                      [--score] [--no-fasta] [--dir DIR] [--out profiles/consensus_<config>.jsonl]
One JSON line per run: alga_consensus_info, `ms_seq` of the unitig call the consensus was made from (the yardstick: k_ut_sequence reads the
same rows once) and the ratio ms_vote / ms_seq, then alga_gfa_info of the FASTA ("fasta").
--score (configs with errors): for every unitig whose window has at least --min-length bases, the window is placed on the generating genome
by a 24-mer from its middle (either strand; unitigs without an exact 24-mer hit are counted as unplaced) and the mismatches of the SPELLED
sequence and of the CONSENSUS over that window are counted on the host: "score" = placed unitigs, columns, mismatches of each."""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402

SEED_K = 24


def _kmer_keys(codes, k):
    """2-bit packed k-mers of a code array at every position (uint64)"""
    c = codes.astype(np.uint64)
    key = np.zeros(len(c) - k + 1, dtype=np.uint64)
    for i in range(k):
        key |= c[i: len(c) - k + 1 + i] << np.uint64(2 * (k - 1 - i))
    return key


def _codes(words, a, n):
    q = a + np.arange(n)
    return ((words[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3).astype(np.uint8)


def score(genome, uh, ch, min_length):
    """mismatches against the genome over the windows of the unitigs with len >= min_length -> dict"""
    keys = _kmer_keys(genome, SEED_K)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    wo = uh["word_off"].astype(np.int64)
    out = dict(unitigs=0, unplaced=0, columns=0, spelled_mismatches=0, consensus_mismatches=0)
    for k in np.nonzero(ch["len"] >= max(min_length, SEED_K))[0]:
        t, L = int(ch["trim_left"][k]), int(ch["len"][k])
        cons = _codes(ch["words"][wo[k]: wo[k + 1]], t, L)
        spel = _codes(uh["words"][wo[k]: wo[k + 1]], t, L)
        placed = False
        for strand in (0, 1):
            c, s = (cons, spel) if strand == 0 else ((3 - cons)[::-1], (3 - spel)[::-1])
            mid = (L - SEED_K) // 2
            key = _kmer_keys(c[mid: mid + SEED_K], SEED_K)[0]
            i = int(np.searchsorted(skeys, key))
            if i < len(skeys) and skeys[i] == key:
                g0 = int(order[i]) - mid
                if g0 >= 0 and g0 + L <= len(genome):
                    g = genome[g0: g0 + L]
                    out["unitigs"] += 1
                    out["columns"] += L
                    out["spelled_mismatches"] += int((s != g).sum())
                    out["consensus_mismatches"] += int((c != g).sum())
                    placed = True
                    break
        if not placed:
            out["unplaced"] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--paths", action="store_true", help="remove the short parallel paths between the cut and the unitigs")
    ap.add_argument("--clip", action="store_true", help="clip the tips (after the parallel paths) before the unitigs")
    ap.add_argument("--min-votes", type=int, default=3)
    ap.add_argument("--min-length", type=int, default=200)
    ap.add_argument("--score", action="store_true", help="mismatches of spelled / consensus sequences against the generating genome (host side, once)")
    ap.add_argument("--no-fasta", action="store_true", help="the consensus call only (no file)")
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--dir", default=None, help="scratch directory for the file (default: a new temporary one)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    import torch
    ws = workload.device_build(n, L, G, seed, err=err, return_genome=a.score)
    torch.cuda.synchronize()                                      # made on torch's stream; the engine's own stream does not order with it
    eng = alga_amd.Engine(0)
    w, l = ws["words"], ws["lens"]
    nn = int(l.shape[0])
    d, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
    if err > 0:
        m_len = int(l[1])
        d, m = eng.pkb_supplement_device(w, l, d, m, eng.pkb_params(float(m_len), err, min(2 * m_len // 3, 60)))
    mopp = max(250, int(1.75 * L))
    d, m, _ = eng.cut_triangles_device(nn, d, m, mopp)
    edges, m_edges = d, m
    bound = int(mopp * float(int(l[1])) / np.float32(100))
    if a.paths:
        edges, _ = eng.remove_short_parallel_paths(nn, edges, bound, n_edges=m_edges)
        m_edges = None
    if a.clip:
        edges, _ = eng.remove_dangling_branches(nn, edges, bound, n_edges=m_edges)
        m_edges = None
    tmp = tempfile.mkdtemp(prefix="consensus_", dir=a.dir)
    sink = open(a.out, "a") if a.out else None
    try:
        for r in range(a.repeat):
            u = eng.unitigs(w, l, edges, n_edges=m_edges, skip_isolated=True)
            c = eng.unitig_consensus(w, l, u, min_votes=a.min_votes)
            out = dict(config=a.config, reads=n, run=r, nodes=nn, paths=a.paths, clip=a.clip, min_votes=a.min_votes, unitig_pairs=u.n_pairs,
                       longest_bases=u.info["longest_bases"], ms_seq=u.info["ms_seq"], ms_vote_over_ms_seq=c.info["ms_vote"] / max(u.info["ms_seq"], 1e-9),
                       source=alga_amd.engine.source_fingerprint(), **c.info)
            if not a.no_fasta:
                path = os.path.join(tmp, "c.fasta")
                out["fasta"] = eng.write_consensus_fasta(path, u, c, min_length=a.min_length)
                os.unlink(path)
            if a.score and r == 0:
                out["score"] = score(ws["genome_codes"], u.to_host(), c.to_host(), a.min_length)
            line = json.dumps(out)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
    finally:
        if sink:
            sink.close()
        shutil.rmtree(tmp, ignore_errors=True)
        eng.close()


if __name__ == "__main__":
    main()
