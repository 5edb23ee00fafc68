"""Short-parallel-path removal timings (alga_remove_short_parallel_paths_device): the graph of a BASELINE config built on the device (with the
supplement where the config has errors), cut by the first simplifier step, then the parallel paths, then the clip; beside it the unitig table
(pairs, links, longest, N50, total bases) for the cut alone, cut + clip and cut + paths + clip.  The bound is the reference's
int(max(250, int(1.75 * LEN)) * AVG_READ_LENGTH / 100.0f) over the reads the cut graph still has an edge at.
    python tools/mst_measure.py [--config cfg2_1M_150bp | cfg5_10M_150bp_err2] [--reads N] [--repeat 3]
One JSON line per run (the first is cold: buffers are allocated in it): alga_mst_info with the winners per round, "tips_after_paths" =
alga_tips_info of the clip on its output, "unitigs_cut" / "unitigs_clip" / "unitigs_paths_clip" = alga_unitig_info plus pairs and N50."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402
from tips_measure import unitig_table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--reads", type=int, default=0, help="that many reads at the config's coverage instead of the config's own number")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    if a.reads:
        n, G = a.reads, int(G * a.reads / n)
    import numpy as np
    import torch
    ws = workload.device_build(n, L, G, seed, err=err)
    torch.cuda.synchronize()                                      # made on torch's stream; the engine's own stream does not order with it
    eng = alga_amd.Engine(0)
    w, l = ws["words"], ws["lens"]
    N = int(l.shape[0])
    d, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
    if err > 0:
        pre = alga_amd.engine.device_view(d, (m, 3), w.device).clone()   # the supplement's build reuses the engine's edge buffer
        p = eng.pkb_params(float(l.float().mean().item()), err, min(2 * ws["min_overlap"] // 3, 60))
        d, m = eng.pkb_supplement_device(w, l, pre.data_ptr(), m, p)
    d2, m2, cut = eng.cut_triangles_device(N, d, m, max(250, int(1.75 * L)))
    e2 = alga_amd.engine.device_view(d2, (m2, 3), w.device).clone()
    live = torch.zeros(N, dtype=torch.bool, device=w.device)
    live[e2[:, 0].long()] = True
    live[e2[:, 1].long()] = True
    avg = float(l[live & (l > 0)].double().mean().item()) if m2 else 0.0
    bound = int(max(250, int(1.75 * L)) * avg / np.float32(100))
    try:
        for r in range(a.repeat):
            mst, info = eng.remove_short_parallel_paths(N, e2, bound)
            out = dict(config=a.config, run=r, reads=n, nodes=N, edges=m, triangle_edges_cut=cut, edges_after_cut=m2, avg_live_read_length=avg, bound=bound, **info)
            both, tinfo = eng.remove_dangling_branches(N, mst, bound)             # the device list goes straight in
            both = both.clone()
            out["tips_after_paths"] = tinfo
            if r == a.repeat - 1:
                clip = eng.remove_dangling_branches(N, e2, bound)[0].clone()
                out["unitigs_cut"] = unitig_table(eng, w, l, e2, m2)
                out["unitigs_clip"] = unitig_table(eng, w, l, clip, int(clip.shape[0]))
                out["unitigs_paths_clip"] = unitig_table(eng, w, l, both, int(both.shape[0]))
            print(json.dumps(out), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
