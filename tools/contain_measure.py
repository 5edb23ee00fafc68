"""Timings of the containment stage (alga_drop_contained_device) on a BASELINE shape: a paired read set generated on the device (the recipe of
tools/extend_measure.py: fragments of 401 nt, mates of the config's read length), the chain build -> cut -> [parallel paths] -> [clip] ->
contigs -> consensus -> final contigs, every read placed on the final contigs, rounds of grow -> placement on the grown contigs, the merge of
the last round's targets, then this stage on the merged contigs, and a placement on the merged and on the kept contigs.
    python tools/contain_measure.py [--config cfg3_5M_150bp] [--reads N] [--genome-factor F] [--paths 0|1] [--clip 0|1] [--rounds 3]
                                    [--max-permille 10] [--fasta PATH] [--repeat 3] [--out profiles/contain_<config>.jsonl]
--genome-factor F stretches the genome F times under the same reads (tools/grow_measure.py); the scaffold table's recipe is --genome-factor 20.
One JSON line per run: alga_contain_info (ms_index / ms_contain / ms_build / ms_total and the counters) beside the same run's merge ms_index /
ms_overlap / ms_build / ms_total (mg_*) -- the yardstick -- and the UNIQUE count of the placement before (on the merged contigs) and after (on
the kept contigs); run 0 is marked cold.  --fasta also writes the kept FASTA of the last run and adds its bytes and wall time.  For the
per-kernel times run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402
from extend_measure import paired_device_build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3_5M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--genome-factor", type=float, default=1.0, help="stretch the genome (divide the coverage) by this factor")
    ap.add_argument("--paths", type=int, default=0)
    ap.add_argument("--clip", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3, help="grow rounds before the merge")
    ap.add_argument("--max-permille", type=int, default=10)
    ap.add_argument("--fasta", default=None, help="write the kept FASTA of the last run here")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    G = int(G * a.genome_factor)
    import torch
    ws = paired_device_build(n, L, G, seed, err)
    torch.cuda.synchronize()
    w, l, po = ws["words"], ws["lens"], ws["pair_off"]
    nn = int(l.shape[0])
    mopp = max(250, int(1.75 * L))
    params = dict(max_permille=a.max_permille)
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
            pl = eng.place_reads(w, l, final=fin, pair_off=po)
            added = 0
            for rnd in range(1, a.rounds + 1):
                gw = eng.grow_ends(w, l, pl)
                added += gw.info["bases_added"]
                if not gw.info["bases_added"]:
                    break
                pl = eng.place_reads(w, l, targets=gw.targets(), pair_off=po)
            mg = eng.merge_ends(gw.targets())
            pm = eng.place_reads(w, l, targets=mg.targets(), pair_off=po)
            kp = eng.drop_contained(mg.targets(), **params)
            pk = eng.place_reads(w, l, targets=kp.targets(), pair_off=po)
            mi = mg.info
            out = dict(config=a.config, genome=G, reads=nn // 2, pairs=ws["pairs"], err=err, paths=a.paths, clip=a.clip, run=r, cold=r == 0, grow_rounds=rnd, grow_bases_added=added,
                       source=alga_amd.engine.source_fingerprint(), contigs=kp.n_targets, mg_ms_index=mi["ms_index"], mg_ms_overlap=mi["ms_overlap"],
                       mg_ms_build=mi["ms_build"], mg_ms_total=mi["ms_total"], contain_ratio=kp.info["ms_contain"] / mi["ms_overlap"] if mi["ms_overlap"] else None,
                       index_ratio=kp.info["ms_index"] / mi["ms_index"] if mi["ms_index"] else None, unique_before=pm.info["unique"], unique_after=pk.info["unique"],
                       placed_before=pm.info["placed"], placed_after=pk.info["placed"], multi_before=pm.info["multi"], multi_after=pk.info["multi"], **params, **kp.info)
            if a.fasta and r == a.repeat - 1:
                fi = eng.write_kept_fasta(a.fasta, kp)
                out.update(fasta_bytes=fi["bytes"], fasta_ms_total=fi["ms_total"])
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
