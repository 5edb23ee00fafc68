"""GFA export timings (alga_write_gfa_device): the graph of a BASELINE config, built on the device, written as GFA into a scratch
directory (deleted afterwards); ms_format (device: checks, sizes, scan, formatting) and ms_total (wall, the file write included).
    python tools/gfa_measure.py [--config cfg2_1M_150bp] [--no-sequences] [--repeat 3] [--dir DIR]
One JSON line per write."""
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
    ap.add_argument("--no-sequences", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default=None, help="scratch directory for the file (default: a new temporary one)")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    import torch
    ws = workload.device_build(n, L, G, seed, err=err)
    torch.cuda.synchronize()                                      # made on torch's stream; the engine's own stream does not order with it
    eng = alga_amd.Engine(0)
    d, m = eng.prefsuf_device(ws["words"], ws["lens"], ws["min_overlap"], ws["rsoemo"])
    tmp = tempfile.mkdtemp(prefix="gfa_", dir=a.dir)
    try:
        for r in range(a.repeat):
            path = os.path.join(tmp, "g.gfa")
            info = eng.write_gfa(path, ws["words"], ws["lens"], d, n_edges=m, sequences=not a.no_sequences)
            os.unlink(path)
            print(json.dumps(dict(config=a.config, sequences=not a.no_sequences, run=r, nodes=int(ws["lens"].shape[0]), edges=m, **info)), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        eng.close()


if __name__ == "__main__":
    main()
