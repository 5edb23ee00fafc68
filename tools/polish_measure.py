"""Timings of the polish (alga_polish_placed_device) on a BASELINE shape: reads generated on the device, the chain build -> cut -> [parallel
paths] -> [clip] -> contigs -> consensus -> final contigs, every read of the set placed on the final contigs, then the placed contigs voted again.
    python tools/polish_measure.py [--config cfg2_1M_150bp] [--err 0.0] [--reads N] [--paths 0|1] [--clip 0|1] [--min-cover 3] [--min-percent 60]
                                   [--multi 0|1] [--counts 0|1] [--repeat 3] [--out profiles/polish_<config>.jsonl]
One JSON line per run: alga_polish_info (ms_sort / ms_vote / ms_total, voters, votes, voted_columns, changed, ambiguous, max_cover) beside the
same run's placement times (ms_index / ms_place / ms_depth), the contigs and their columns.  The build is the exact one (no supplement): with
--err > 0 the contigs are what the exact overlaps of the erroneous reads give.  For the per-kernel times run this script under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--err", type=float, default=None, help="substitution rate of the reads (default: the config's)")
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--paths", type=int, default=0)
    ap.add_argument("--clip", type=int, default=0)
    ap.add_argument("--min-cover", type=int, default=3)
    ap.add_argument("--min-percent", type=int, default=60)
    ap.add_argument("--multi", type=int, default=0)
    ap.add_argument("--counts", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    err = err if a.err is None else a.err
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    import torch
    ws = workload.device_build(n, L, G, seed, err=err)
    torch.cuda.synchronize()
    w, l = ws["words"], ws["lens"]
    nn = int(l.shape[0])
    mopp = max(250, int(1.75 * L))
    eng = alga_amd.Engine(0)
    sink = open(a.out, "a") if a.out else None
    try:
        d_edges, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
        d_cut, m_cut, _ = eng.cut_triangles_device(nn, d_edges, m, mopp)
        edges = alga_amd.engine.device_view(d_cut, (m_cut, 3), "cuda:0").clone()
        if a.paths:
            edges = eng.remove_short_parallel_paths(nn, edges, mopp)[0].clone()
        if a.clip:
            edges = eng.remove_dangling_branches(nn, edges, mopp)[0].clone()
        u = eng.contigs(w, l, edges, mopp)
        c = eng.unitig_consensus(w, l, u)
        fin = eng.final_contigs(u, c, max(200, int(1.75 * L)), 95, 25)
        for r in range(a.repeat):
            pl = eng.place_reads(w, l, final=fin, depth_multi=bool(a.multi))
            pol = eng.polish(w, l, pl, min_cover=a.min_cover, min_percent=a.min_percent, multi=bool(a.multi), counts=bool(a.counts))
            out = dict(config=a.config, reads=nn // 2, err=err, paths=a.paths, clip=a.clip, run=r, min_cover=a.min_cover, min_percent=a.min_percent, multi=a.multi,
                       counts=a.counts, source=alga_amd.engine.source_fingerprint(), contigs=fin.n_written, vote="per-word",
                       ms_index=pl.info["ms_index"], ms_place=pl.info["ms_place"], ms_depth=pl.info["ms_depth"], ms_place_total=pl.info["ms_total"],
                       unique_share=pl.info["unique"] / max(pl.info["reads"], 1), cover_matches=bool((pol.counts.sum(dim=1) == pl.cover).all().item()) if a.counts else None,
                       **pol.info)
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
