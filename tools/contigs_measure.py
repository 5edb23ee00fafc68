"""Contig timings (alga_contigs_device): the graph of a BASELINE config, built on the device (supplemented when the config has errors), cut by the
first simplifier step, optionally without its short parallel paths and tips; then the contigs (contract, cut the contracted graph, contract
again) and their consensus.
    python tools/contigs_measure.py [--config cfg2_1M_150bp] [--repeat 3] [--paths] [--clip] [--min-votes 3] [--reads N]
                                    [--out profiles/contigs_<config>.jsonl]
One JSON line per run: alga_contig_info (rounds, the per-round counts, ms_* per stage), next to it `unitig_ms_total` -- alga_unitigs_device on the
same input, the yardstick -- and N50 / longest of the consensus windows of the contigs against those of the unitigs."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402


def n50(lengths):
    ls = np.sort(np.asarray(lengths, dtype=np.int64))[::-1]
    if not len(ls) or ls.sum() == 0:
        return 0
    return int(ls[np.searchsorted(np.cumsum(ls), (ls.sum() + 1) // 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--paths", action="store_true", help="remove the short parallel paths between the cut and the contigs")
    ap.add_argument("--clip", action="store_true", help="clip the tips (after the parallel paths) before the contigs")
    ap.add_argument("--min-votes", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    import torch
    ws = workload.device_build(n, L, G, seed, err=err)
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
    sink = open(a.out, "a") if a.out else None
    try:
        for r in range(a.repeat):
            u = eng.unitigs(w, l, edges, n_edges=m_edges, skip_isolated=True)
            uw = eng.unitig_consensus(w, l, u, min_votes=a.min_votes).len.cpu().numpy()
            ui = dict(u.info)
            k = eng.contigs(w, l, edges, mopp, n_edges=m_edges)
            kc = eng.unitig_consensus(w, l, k, min_votes=a.min_votes)
            kw = kc.len.cpu().numpy()
            out = dict(config=a.config, reads=n, run=r, nodes=nn, paths=a.paths, clip=a.clip, max_offset=mopp, contig_pairs=k.n_pairs, contig_edges=k.n_edges,
                       unitig_pairs=u.n_pairs, unitig_ms_total=ui["ms_total"], ms_total_over_unitig_ms_total=k.info["ms_total"] / max(ui["ms_total"], 1e-9),
                       windows=dict(contig_n50=n50(kw), contig_longest=int(kw.max()) if len(kw) else 0, unitig_n50=n50(uw),
                                    unitig_longest=int(uw.max()) if len(uw) else 0),
                       consensus_ms_total=kc.info["ms_total"], source=alga_amd.engine.source_fingerprint(), **k.info)
            line = json.dumps(out)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
    finally:
        if sink:
            sink.close()
        eng.close()


if __name__ == "__main__":
    main()
