"""Unitig graph timings (alga_unitigs_device, alga_write_unitig_gfa_device): the graph of a BASELINE config, built on the device, cut by
the first simplifier step (alga_cut_triangles_device, max(250, int(1.75 * read length))), compacted into unitigs without isolated reads
and written as GFA with sequences into a scratch directory (deleted afterwards); beside it the read-level export of the same cut graph.
    python tools/unitig_measure.py [--config cfg2_1M_150bp] [--repeat 3] [--ruling -1|0|1] [--no-gfa] [--dir DIR]
One JSON line per run: alga_unitig_info, then alga_gfa_info of the unitig file ("unitig_gfa") and of the read-level file ("read_gfa")."""
import argparse
import json
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--ruling", type=int, default=-1, choices=[-1, 0, 1], help="engine option unitig_ruling (0: plain pointer jumping)")
    ap.add_argument("--no-gfa", action="store_true", help="the unitig call only (no files)")
    ap.add_argument("--dir", default=None, help="scratch directory for the files (default: a new temporary one)")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    import torch
    ws = workload.device_build(n, L, G, seed, err=err)
    torch.cuda.synchronize()                                      # made on torch's stream; the engine's own stream does not order with it
    eng = alga_amd.Engine(0)
    eng.set_option("unitig_ruling", a.ruling)
    w, l = ws["words"], ws["lens"]
    d, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
    d2, m2, removed = eng.cut_triangles_device(int(l.shape[0]), d, m, max(250, int(1.75 * L)))
    tmp = tempfile.mkdtemp(prefix="unitig_", dir=a.dir)
    try:
        for r in range(a.repeat):
            u = eng.unitigs(w, l, d2, n_edges=m2, skip_isolated=True)
            out = dict(config=a.config, ruling=a.ruling, run=r, nodes=int(l.shape[0]), edges=m, edges_after_cut=m2, pairs=u.n_pairs, unitig_edges=u.n_edges, **u.info)
            if not a.no_gfa:
                path = os.path.join(tmp, "u.gfa")
                out["unitig_gfa"] = eng.write_unitig_gfa(path, u)
                os.unlink(path)
                # the read-level writer takes lists sorted by (src, dst, offset): the cut leaves them in the reference's order
                ds = eng.sort_edges_device(d2, m2, int(l.shape[0]))
                out["read_gfa"] = eng.write_gfa(path, w, l, ds, n_edges=m2, sequences=False)
                os.unlink(path)
            print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        eng.close()


if __name__ == "__main__":
    main()
