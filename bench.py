#!/usr/bin/env python3
"""bench.py -- overlap-graph construction throughput of the HIP engine on MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg4_50M_150bp] [--dump-outputs DIR] [--full [--no-cpu-baseline] ...]

A "step" is one complete pass of the hot path (GraphCreatorPrefSuf + retainOnlySmallestOffset, reference
src/main.cpp:244-296: index of the targets, probe of every source, transitive reduction, sorted adjacency lists) over one
synthetic read set that is already resident in HBM when the timed region starts.  Prints ONE JSON line (rank 0):
  metric   overlap_edges_per_sec   (BASELINE.json: overlap edges/sec; Gbp/s of input reads is `gbp_per_sec`)
  value    edges in the emitted graph x steps / wall time of the K steps (max over ranks), whole job, inputs resident in HBM
  ms_per_step  wall time of one timed step
A plain run does only that: set up, W untimed steps (at least one), the K timed steps, the line.  --dump-outputs DIR writes the
edge list of the last timed step (dump_outputs).  --full adds everything else, each leg as described here:
  first_call  the first builds of a fresh engine, with and without alga_engine_reserve
  timed_edges_digest_equal_pairwise  the last timed step's list against one counted pass of the pairwise kernels
  roofline dominant kernel (the probe): SURVEY.md section 8(d) algorithmic bytes / its HIP-event duration vs the 8 TB/s HBM peak
  cpu_baseline  the real reference binary (oracle/_ref/ALGA, kind "reference") -- or the C oracle (kind "port") where it is
                absent -- timed on this box's host cores on a bounded sample of the same workload; the GPU graph of the same
                sample is compared with the reference's --serialize=1 dump byte for byte.
  pcie_inclusive  the same graph through the host-buffer entry point (packed host reads in, host edge list out): never `value`.

Workload: BASELINE.json configs[3]'s read set, the one `metric` is quoted on -- 50 M x 150 bp error-free reads over a 250 Mb
genome (SURVEY.md section 8(d) generator, seed 11), generated on the device; it fits one GPU (5.8 GB of rows).
N > 1 (one process per GPU under torch.distributed.run, RCCL): STRONG scaling -- the same 50 M reads for every N; every rank
holds the node set, builds the target index, probes 1/N of the sources (contiguous id range) and the edge lists are gathered
on rank 0 over RCCL.  Other configs (`--config cfg2_1M_150bp` ...) are built on the host exactly as the reference's input
stages would number the nodes.
"""
import argparse
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)


def algorithmic_bytes(st, W):
    """packed reads once + one 16 B table probe per (node, overlap length) +
    one packed-read fetch per raw candidate (probe kernel); one packed-read fetch per transitive compare
    (reduce kernel); 12 B per emitted edge."""
    probe = st["nodes_live"] * 4 * W + st["windows_probed"] * 16 + st["raw_overlaps"] * 4 * W
    reduce_ = st["transitive_compares"] * 4 * W
    emit = st["edges"] * 12
    return dict(probe=probe, reduce=reduce_, emit=emit, total=probe + reduce_ + emit)


def cpu_baseline_reference(codes, threads, eng, err=0.0):
    """The real reference (oracle/_ref/ALGA) on `codes` (uint8 [k, L]): creator wall time between its stderr markers 'Creating
    GraphCreator' and 'Before first simplifier' (its own timers report CPU-seconds, src/Utils/TimeMeasurer.cpp:26-39), its
    --serialize=1 dump compared byte for byte with the graph the engine builds from the same reads."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ALGA")
    if not os.path.exists(exe):
        return None
    from alga_amd import workload
    with tempfile.TemporaryDirectory() as wd:
        workload.write_fasta_fast(os.path.join(wd, "s.fasta"), codes)
        extra = ["--error_rate=%g" % err] if err > 0 else []     # > 0.01: the reference adds its approximate supplement (src/main.cpp:300-355)
        p = subprocess.Popen([exe, "--file1=s.fasta", "--threads=%d" % threads, "--serialize=1", "--output=o.fasta"] + extra, cwd=wd,
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, errors="replace", bufsize=1)
        t0 = t1 = None
        edges = None
        for line in p.stderr:
            if t0 is None and "Creating GraphCreator" in line:
                t0 = time.perf_counter()
            m = re.search(r"Before first simplifier graph has (\d+) edges", line)
            if m:
                t1 = time.perf_counter()
                edges = int(m.group(1))
                break
        p.kill()
        p.wait()
        if t0 is None or t1 is None:
            return None
        dumps = glob.glob(os.path.join(wd, "*_beforeSimplifier.graph"))
        bytes_equal = None
        if dumps:
            # the engine on the same reads: node set numbered as the reference numbers it (alga_amd/workload.make_nodes)
            words, lens, _ = workload.make_nodes(codes)
            lo, rs = workload.derive_params(float(codes.shape[1] - 6))
            ge = eng.prefsuf_host(words, lens, lo, rs)
            mine = os.path.join(wd, "gpu.graph")
            eng.write_graph(mine, len(lens), ge)
            bytes_equal = open(mine, "rb").read() == open(dumps[0], "rb").read()      # (the dump is the EXACT path's graph, before any supplement)
    dt = t1 - t0
    return dict(value=edges / dt, unit="edges/s", cores=threads, kind="reference",
                sample="%d x %d bp reads of the same workload (every read that starts in the first genome_len * sample / n_reads positions: same coverage), ALGA --threads=%d --serialize=1%s, "
                       "creator region src/main.cpp:244-%d, %.2f s wall, %d edges" % (len(codes), codes.shape[1], threads, " --error_rate=%g" % err if err > 0 else "",
                                                                                     355 if err > 0 else 296, dt, edges),
                seconds=dt, edges=edges, gbp_per_sec=codes.size / dt / 1e9, graph_bytes_equal_gpu=bytes_equal)


def cpu_baseline_port(words, lens, lo, rs, budget_nodes):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if not os.path.exists(os.path.join(ROOT, "oracle", "liboracle.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"], stdout=subprocess.DEVNULL)
    import oracle_lib as O
    w, l = words[:budget_nodes], lens[:budget_nodes]
    t0 = time.perf_counter()
    e, _, _ = O.prefsuf(w, l, lo, rs)
    dt = time.perf_counter() - t0
    return dict(value=len(e) / dt, unit="edges/s", cores=1, kind="port",
                sample="first %d nodes of the workload, single-thread C oracle, %.2f s" % (len(l), dt), seconds=dt, edges=len(e))


def profiled_traffic(config, src_sha):
    """({kernel name: HBM bytes per dispatch}, HBM bytes per STEP over all kernels) from the rocprofv3 --pmc passes of `bench.py --traffic-pass`
    (tools/profile_cmd.sh passes r, x -> tools/pmc_to_traffic.py -> profiles/hbm_traffic.json: 128 B per read request, 32 / 64 B per write
    request), only when they were taken on THESE kernel sources (alga_amd.engine.source_fingerprint); else ({}, None)."""
    try:
        ent = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json"))).get(config)
    except Exception:
        return {}, None
    if not ent or ent.get("src_sha256") != src_sha:
        return {}, None
    # per kernel: the bytes of ONE build (a kernel that runs several times per build -- the passes of the radix sort -- counts with all of them)
    return {k: (v.get("bytes_per_build") or v["read_bytes"] + v["write_bytes"]) for k, v in ent["per_dispatch"].items()}, ent.get("per_step_bytes")


def traffic_of(traffic, prefix):
    v = [b for k, b in traffic.items() if k.startswith(prefix)]
    return int(sum(v)) if v else None


DUMP_ROWS = 1_500_000      # 36 MB of float64 edge rows + 12 MB of their row numbers: the dump stays under 64 MB
DUMP_SEED = 2024


def dump_outputs(out_dir, edges):
    """What the timed path hands its caller: the edge list [m, 3] (src, dst, offset; device int32) of the graph of the last timed step, as
    float64 .npy files (float64 holds every int32 exactly):
      edges.npy         the whole list when it has at most DUMP_ROWS rows; else the rows at edges_rows.npy
      edges_rows.npy    (only when sampled) sorted row numbers, drawn with a fixed seed: the same rows for the same edge count
      edges_digest.npy  [count, the list's position-weighted int64 checksum (alga_amd.multigpu.edges_digest) as four 16-bit limbs, low first]"""
    import torch
    from alga_amd import multigpu
    os.makedirs(out_dir, exist_ok=True)
    m = int(edges.shape[0])
    rows = None
    if m > DUMP_ROWS:
        rows = np.unique(np.random.default_rng(DUMP_SEED).integers(0, m, DUMP_ROWS))
        sample = edges[torch.from_numpy(rows).to(edges.device)]
    else:
        sample = edges
    np.save(os.path.join(out_dir, "edges.npy"), sample.cpu().numpy().astype(np.float64).reshape(-1, 3))
    if rows is not None:
        np.save(os.path.join(out_dir, "edges_rows.npy"), rows.astype(np.float64))
    count, checksum = [int(x) for x in multigpu.edges_digest(edges).cpu()]
    checksum &= (1 << 64) - 1
    np.save(os.path.join(out_dir, "edges_digest.npy"), np.array([count] + [(checksum >> (16 * i)) & 0xFFFF for i in range(4)], dtype=np.float64))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="cfg4_50M_150bp")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: first-call legs, the counted pass (work counters, roofline, digest of the timed list against "
                         "it), PCIe-inclusive forms, CPU baseline (the --no-* options below switch single legs off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the edge list of the last one as DIR/*.npy (float64; a fixed sample of rows when it is large)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pcie", action="store_true")
    ap.add_argument("--no-first-call", action="store_true")
    ap.add_argument("--traffic-pass", action="store_true",
                    help="for the rocprofv3 --pmc passes (tools/profile_cmd.sh): only W + K steps of the TIMED form -- no first-call legs, no counted pass, no "
                         "PCIe leg, no CPU baseline -- so that every dispatch the counters see belongs to a step as it is timed (tools/pmc_to_traffic.py ... --builds W+K)")
    ap.add_argument("--cpu-sample-reads", type=int, default=1_000_000, help="reads of the workload the CPU baseline runs on (~10 s of the reference at 16 threads)")
    ap.add_argument("--probe", default="auto", choices=["auto", "table", "cluster"])
    ap.add_argument("--multi-plain", action="store_true", help="N > 1: time the driver's plainest form (no sharded key pass, no pieces)")
    ap.add_argument("--multi-form", default="replicated", choices=["replicated", "bucket_sharded"],
                    help="N > 1: replicated = every rank the whole index, its own source ids (default: the faster one by the one-GPU emulation, DESIGN.md section 7); "
                         "bucket_sharded = the index sharded by seed bucket (alga_shard_*); either is timed only after it reproduced the plain form's graph in this run")
    return ap.parse_args(argv)


def main():
    t_process = time.perf_counter()
    args = parse_args()
    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with: python -m torch.distributed.run --nproc-per-node %d bench.py --gpus %d ..." % (args.gpus, args.gpus))
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        import datetime
        # a collective that never completes aborts the job after 5 minutes instead of holding the node
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank), timeout=datetime.timedelta(seconds=300))
    out = run(args, rank, world, local_rank, dist, t_process)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        if args.full:
            wall = time.perf_counter() - t_process
            out["fits_in_driver_run"] = {"wall_s": round(wall, 1), "limit_s": 600, "fits": wall < 600,
                                         "note": "whole bench.py --full process: workload generation, first-call legs, counted pass, warmup, timed steps, PCIe leg, CPU baseline"}
        print(json.dumps(out))
        if out.get("timed_edges_digest_equal_pairwise") is False:
            raise SystemExit("bench.py: the edge list of the last timed step differs from the counted (pairwise) pass: %s" % (out["timed_edges_digest"],))


def run(args, rank, world, local_rank, dist, t_process=None):
    """The measurement of one rank -> the JSON object (rank 0) or None.  `dist`: torch.distributed with the process group up (N > 1), or
    a stand-in with the same calls (tests/test_gpu_parity.py rehearses this function as N thread-ranks on one GPU)."""
    import torch
    import alga_amd
    from alga_amd import workload
    from alga_amd import multigpu

    # ---- workload (synthetic).  Every rank builds the same node set on its own GPU: the generator is seeded. ----------------
    n_reads, read_len, G, seed, err = workload.CONFIGS[args.config]
    sample_codes = None
    host_words = host_lens = None
    t_build = time.perf_counter()
    if n_reads >= 4_000_000:
        wl = workload.device_build(n_reads, read_len, G, seed, err=err, sample_reads=(args.cpu_sample_reads if rank == 0 and args.full else 0))
        d_words, d_lens = wl["words"], wl["lens"]
        sample_codes = wl["sample_codes"]
        how = "generated on the device (alga_amd.workload.device_build)"
    else:
        wl = workload.build(args.config, stride_words="aligned")
        host_words, host_lens = wl["words"], wl["lens"]
        d_words = torch.from_numpy(wl["words"].view(np.int32)).cuda()
        d_lens = torch.from_numpy(wl["lens"]).cuda()
        sample_codes = wl["codes"][:args.cpu_sample_reads]
        how = "built on the host as the reference's input stages number the nodes (alga_amd.workload.build)"
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t_build
    lo, rs = wl["min_overlap"], wl["rsoemo"]
    n_nodes = int(d_lens.shape[0])
    max_len = int(d_lens.max().item()) if n_nodes else 0
    W = (2 * max_len + 31) // 32
    # error_rate > 0.01: the scored path is the exact graph PLUS the approximate supplement (src/main.cpp:244-355); one GPU
    # (N > 1: the k-mer groups of the supplement are dealt out over the ranks by hash, alga_amd.multigpu.ShardedSupplement / alga_pkb_shard_*)
    supplement = err > 0.01
    pkb = alga_amd.Engine.pkb_params(float(d_lens[d_lens > 0].float().mean().item()), err, min(2 * lo // 3, 60)) if supplement else None

    # ---- the FIRST call of a process (what an assembler pays: it builds its graph once) --------------------------------------
    first = None
    eng = alga_amd.Engine(local_rank)
    eng.set_option("probe", args.probe)
    if world == 1 and not args.no_first_call and not args.traffic_pass and not args.full:
        # a plain run: the reserve call alone (part of setting up, as in an assembler), so that the timed engine is prepared as under --full
        eng.reserve(n_nodes, max_len, lo)
    elif world == 1 and not args.no_first_call and not args.traffic_pass:
        # (a) the first engine of this process: alga_engine_reserve (an assembler calls it while it still parses / uploads), then the build
        t0 = time.perf_counter()
        eng.reserve(n_nodes, max_len, lo)
        torch.cuda.synchronize()
        t_res = time.perf_counter() - t0
        t0 = time.perf_counter()
        eng.prefsuf_device(d_words, d_lens, lo, rs)
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        first = {"reserve_ms": t_res * 1e3, "first_call_ms": t_first * 1e3, "first_call_device_ms": eng.last_stats()["ms_total"]}
        # (b) a second fresh engine WITHOUT the reserve call: every device buffer is allocated inside the build (each hipMalloc waits for
        #     the stream, so the kernels around it no longer overlap their launches)
        cold = alga_amd.Engine(local_rank)
        cold.set_option("probe", args.probe)
        t0 = time.perf_counter()
        cold.prefsuf_device(d_words, d_lens, lo, rs)
        torch.cuda.synchronize()
        first["unprepared_first_call_ms"] = (time.perf_counter() - t0) * 1e3
        first["unprepared_first_call_device_ms"] = cold.last_stats()["ms_total"]
        cold.close()
        del cold
        first["note"] = ("wall time of alga_prefsuf_build_device on a fresh engine.  (a) the FIRST engine of this process after alga_engine_reserve (reserve_ms: every device "
                         "buffer sized from the node count + a miniature build of the same shape that makes the HIP runtime load the kernels' code objects -- an assembler "
                         "calls it while it still parses / uploads); (b) unprepared = a second fresh engine of the same process without reserve: it allocates inside its build, "
                         "but finds the code objects loaded.  Without either, the first build of a process took 58 ms at this size (code-object loading ~20 ms, allocations ~1 ms).")
    backend = multigpu.HipBackend(eng, d_words, d_lens, lo, rs)
    runner = multigpu.ShardedPrefSuf(backend, rank, world, dist)
    backend.pkb = pkb
    sharded_sup = multigpu.ShardedSupplement(backend, rank, world, dist) if (supplement and world > 1) else None

    def sync_all():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # N > 1: the driver's defaults are its plainest form (every rank computes all keys, one piece per rank: ADVICE of round 2).  The
    # faster one -- keys of the own nodes only + in-place key all-gather, the source range in pieces whose edge transfers overlap the
    # next piece's probe -- is taken for the timed steps only after it has reproduced, in THIS run and over the real transport, the
    # plain form's complete graph on rank 0 byte for byte (count + position-weighted checksum); otherwise the plain form is timed.
    multi_form = None
    if world > 1 and not args.multi_plain:
        fast_kw = dict(bucket_sharded=True, pieces=1) if args.multi_form == "bucket_sharded" else {}
        runner, multi_form = multigpu.validated_runner(backend, rank, world, dist, plain=runner, **fast_kw)
    elif world > 1:
        multi_form = {"form": "plain (all keys on every rank, one piece per rank)", "validated": "--multi-plain"}

    final = {}

    def step(collect_stats=False):
        """one pass of the hot path over the resident read set -> (edges of the graph handed to the simplifier, stats)"""
        m, st = runner.step(collect_stats=collect_stats)
        final["edges"] = runner.edges
        if supplement and world > 1:
            with backend.stream_scope():
                final["edges"] = sharded_sup.run(runner.edges)
                m = int(final["edges"].shape[0])
        elif supplement:
            p2, m = eng.pkb_supplement_device(d_words, d_lens, runner.edges.data_ptr(), m, pkb)
            final["edges"] = alga_amd.engine.device_view(p2, (m, 3), d_words.device)
        if supplement:
            ps = eng.pkb_last_stats()
            st = dict(st)
            st["ms_supplement"] = ps["ms_total"]
            st["pkb"] = ps
        return m, st

    def digest():
        """[count, position-weighted checksum] of the list the last step left (rank 0 holds the complete graph)"""
        e = final.get("edges")
        if e is None or rank != 0:
            return None
        torch.cuda.synchronize()
        return [int(x) for x in multigpu.edges_digest(e).cpu()]

    if args.traffic_pass:
        for _ in range(args.warmup + args.steps):
            n_edges, s = step()
        sync_all()
        return {"traffic_pass": True, "builds": args.warmup + args.steps, "edges": int(n_edges), "config": {"workload": args.config},
                "pile_buckets": int(s.get("pile_buckets", 0)), "pile_irregular": int(s.get("pile_irregular", 0)), "src_sha256": alga_amd.engine.source_fingerprint()} if rank == 0 else None

    if args.full:
        # one counted pass (work counters for the roofline's algorithmic bytes); not timed.  A build that collects the work counters runs
        # the PAIRWISE kernels (the counters are defined by what those do) -- its edge list is the independent one the timed list is compared with
        n_edges, st = step(collect_stats=True)
        stats = dict(st)
        digest_counted = digest()
        if world > 1:
            stats["nodes_live"] = n_nodes                 # whole-job counters (all_reduced); nodes are replicated
        warm = args.warmup - 1                            # (the counted pass is the first untimed step)
    else:
        warm = max(1, args.warmup)                        # at least one, as with the counted pass: --warmup 0 still times a warmed engine
    for _ in range(max(0, warm)):
        step()
    sync_all()
    keys_ms = ("seed", "probe", "group", "reduce", "emit", "exchange", "probe_pairs", "keys", "sort", "gather", "dir", "pile", "supplement")
    phase = {k: 0.0 for k in keys_ms}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        n_edges, s = step()
        for k in phase:
            phase[k] += s.get("ms_" + k, 0.0)
    sync_all()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, final["edges"])       # before anything else can reuse the engine memory the list lies in
    digest_timed = digest() if args.full else None          # of the LAST timed step's list, after the clock has stopped
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    out = None
    if rank == 0:
        ms_step = dt / args.steps * 1e3
        bases = n_reads * read_len
        workload_desc = ("%s: %d x %d bp reads, genome %d, seed %d, err %.2f -> %d nodes (both strands, duplicates removed), "
                         "min_overlap %d, rsoemo %d; %s in %.1f s%s" %
                         (args.config, n_reads, read_len, G, seed, err, n_nodes, lo, rs, how, t_build,
                          "; a step = exact overlap graph + approximate supplement (error_rate %.2f)" % err if supplement else ""))
        if not args.full:
            out = {"metric": "overlap_edges_per_sec", "value": n_edges * args.steps / dt, "unit": "edges/s",
                   "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
                   "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
                   "gbp_per_sec": bases / (ms_step * 1e-3) / 1e9,
                   "config": {"workload": workload_desc, "nodes": n_nodes, "edges": int(n_edges)},
                   "device": eng.device_name()}
            if world > 1:
                out["multi_gpu_form"] = multi_form
            return out
        ms = {k: v / args.steps for k, v in phase.items()}
        alg = algorithmic_bytes(stats, W)
        alg_probe_launch = alg["probe"] / world           # one launch = one rank's share of the sources
        achieved = alg_probe_launch / (ms["probe"] * 1e-3) / 1e9
        # The probe of the clustered path is TWO kernels: k_probe_stream (four-source rows, rounds packed from a sliding window of two quads) finishes the regular sources and
        # defers the others, k_probe_clustered takes the deferred ones.  `roofline` is the dominant one on the sources it FINISHES;
        # `probe_phase` is both kernels over all sources (the HIP events around the two launches).
        n_src = max(1, stats["nodes_live"])
        # The counted pass above ran the PAIRWISE kernels (a build that collects the work counters does: they are defined by what those
        # do); the timed steps take the probe through piles where the input allows it (prefsuf_pile.hip): k_pile_probe instead of
        # k_probe_stream, and its own number of sources handed to the general kernel.
        piled = world == 1 and s.get("pile_buckets", 0) > 0 and s.get("pile_irregular", 0) * alga_amd.engine.PILE_DECLINE_ONE_IN <= s.get("pile_buckets", 0) and ms["pile"] > 0
        first_name = "k_pile_probe" if piled else "k_probe_stream"
        deferred = int((s if piled else stats).get("deferred_sources", 0))
        two_kernels = stats.get("probe_used") == 2 and ms["probe_pairs"] > 0 and world == 1
        first_dominates = two_kernels and 2 * ms["probe_pairs"] >= ms["probe"]
        if first_dominates:
            probe_kernel, kernel_ms = first_name, ms["probe_pairs"]
            kernel_bytes = alg_probe_launch * (1.0 - deferred / n_src)
        else:
            # one kernel did (nearly all of) the probing -- seed-table probe; the general clustered kernel on reads with sequencing
            # errors, where the quad kernel's waves hand their share on; N > 1, where the split is not collected: the phase as a whole
            probe_kernel = "k_probe_sources" if stats.get("probe_used") != 2 else ("k_probe_stream + k_probe_clustered (probe phase)")
            kernel_ms, kernel_bytes = ms["probe"], alg_probe_launch
        src_sha = alga_amd.engine.source_fingerprint()     # of the kernel sources: what the counter passes are keyed on
        traffic, traffic_step = profiled_traffic(args.config, src_sha) if world == 1 else ({}, None)
        tr_kernel = traffic_of(traffic, first_name) if first_dominates else (
            (traffic_of(traffic, "k_probe_stream") or 0) + (traffic_of(traffic, "k_probe_clustered") or 0) or traffic_of(traffic, "k_probe_sources"))
        # The kernel's OWN byte model: what its formulation has to move per source.  Pile path: a 16-byte side record, a 64-byte run list, the
        # first 64 bytes of a bucket record per run, one 8-byte slot.  Pairwise clustered kernels: the source's entry and run list, a 16-byte
        # directory record per run, every entry scanned.  Seed-table probe: SURVEY section 8(d)'s figure is its own model (one 16-byte probe per
        # window, one row per candidate).
        eq = (W + 3 + 3) // 4
        runs_per_node = 1.0 + 2.0 * (stats["windows_probed"] / n_src - 1.0) / (min(64, lo - max(lo - 63, min(lo, 16)) + 1) + 1.0)
        if piled:
            own_bytes = (n_src - deferred) * (16 + 64 + runs_per_node * 64 + 8)
            own_def = "per source: 16 B side record + 64 B run list + 64 B of a bucket record per run (%.2f runs) + 8 B slot" % runs_per_node
        elif stats.get("probe_used") == 2:
            own_bytes = (kernel_bytes / max(1.0, alg_probe_launch)) * (n_src * (16 * eq + 64 + runs_per_node * 16) + stats["slots_scanned"] * 16 * eq)
            own_def = "per source: its %d B entry + 64 B run list + 16 B directory record per run (%.2f runs) + %d B per entry scanned (%.1f per source)" % (
                16 * eq, runs_per_node, 16 * eq, stats["slots_scanned"] / n_src)
        else:
            own_bytes, own_def = kernel_bytes, "SURVEY section 8(d): 4W + 16 per window + 4W per verified candidate"
        # PRIMARY figure = what the kernel physically sustains: HBM bytes from the memory-request counters / its launch duration / peak when a
        # counter pass of THESE kernel sources exists, else its own byte model.  SURVEY section 8(d)'s pairwise bytes / duration stays next to
        # it as frac_pairwise_equivalent: for a kernel that no longer moves those bytes (the pile path) it exceeds 1 and is a statement about
        # the algorithm, not about HBM.
        phys_bytes, basis = (tr_kernel, "counters") if tr_kernel else (own_bytes, "own_byte_model")
        achieved_kernel = phys_bytes / (kernel_ms * 1e-3) / 1e9
        pairwise_equiv = kernel_bytes / (kernel_ms * 1e-3) / 1e9
        # step level: the bytes a build cannot avoid (every row and length read once, every edge written once) against what all kernels of a
        # step move together (counter traffic summed over a step's dispatches)
        compulsory = n_nodes * (4 * W + 4) + int(n_edges) * 12
        roofline_step = {"compulsory_bytes": int(compulsory), "compulsory_def": "n_nodes * (4W + 4) + edges * 12: rows and lengths read once, edges written once",
                         "ms_per_step": ms_step, "frac_compulsory": compulsory / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "traffic_bytes": traffic_step, "frac_traffic": (traffic_step / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic_step else None,
                         "traffic_amplification": (traffic_step / compulsory) if traffic_step else None,
                         "traffic_source": "sum over every dispatch of a timed-form step (bench.py --traffic-pass under rocprofv3 --pmc; null = not profiled on these kernel sources)"}
        out = {
            "metric": "overlap_edges_per_sec", "value": n_edges * args.steps / dt, "unit": "edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
            "gbp_per_sec": bases / (ms_step * 1e-3) / 1e9,
            "config": {"workload": workload_desc,
                       "nodes": n_nodes, "edges": int(n_edges), "parallelism": "1 GPU" if world == 1 else
                       "strong scaling: the same read set for every N; node set and target index on every rank, sources sharded over %d ranks "
                       "(contiguous id ranges); edge lists gathered on rank 0 over RCCL" % world},
            "timed_edges_digest_equal_pairwise": bool(digest_timed is not None and digest_timed == digest_counted),
            "timed_edges_digest": {"timed_last_step": digest_timed, "counted_pairwise_pass": digest_counted,
                                   "note": "[count, position-weighted int64 checksum] of the edge list the LAST timed step left against the list of the counted pass, "
                                           "which ran other kernels (a build that collects work counters takes the pairwise probe); the run fails when they differ"},
            "roofline": {"bound": "hbm", "kernel": probe_kernel, "achieved": achieved_kernel, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved_kernel / HBM_PEAK_GBS, "basis": basis, "traffic": tr_kernel,
                         "own_byte_model": {"bytes": int(own_bytes), "def": own_def, "frac": own_bytes / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
                         "frac_pairwise_equivalent": pairwise_equiv / HBM_PEAK_GBS,
                         "pairwise_equivalent_note": "SURVEY.md section 8(d)'s algorithmic bytes of the reference's pairwise algorithm (4W + 16 P + 4W raw per source) / this kernel's duration / peak: "
                                                     "above 1 when the kernel decides the same overlaps without moving those bytes (pile path) -- not a roofline fraction",
                         "traffic_source": "rocprofv3 --pmc passes of bench.py --traffic-pass on this build (tools/profile_cmd.sh r, x -> profiles/hbm_traffic.json, kernel sources %s): "
                                           "128 B per memory-side read request (gfx950 issues no other size), 32 / 64 B per write request; null = not profiled on this build "
                                           "(frac then rests on the kernel's own byte model)" % src_sha,
                         "algorithmic_bytes": kernel_bytes, "kernel_ms": kernel_ms,
                         "units": "%d source nodes finished by this kernel per launch (of %d; %d deferred to k_probe_clustered)" % (n_src - deferred, n_src, deferred) if first_dominates else "%d source nodes per launch" % (n_src // world),
                         "per_unit": "per source node: 4W + 16 P + 4W * raw/node bytes (W=%d words, P=%.1f windows, raw/node=%.2f)" %
                                     (W, stats["windows_probed"] / max(1, stats["nodes_live"]), stats["raw_overlaps"] / max(1, stats["nodes_live"]))},
            "roofline_step": roofline_step,
            "probe_phase": {"kernels": [first_name, "k_probe_clustered"] + (["k_pile_deg"] if piled else []) if two_kernels else [probe_kernel], "ms": ms["probe"],
                            "algorithmic_bytes": alg_probe_launch, "achieved": achieved, "frac": achieved / HBM_PEAK_GBS},
            "phases_ms": {k: ms[k] for k in ("seed", "probe", "group", "reduce", "emit", "exchange")},
            "counters": {k: int(stats[k]) for k in ("nodes_live", "windows_probed", "slots_scanned", "raw_overlaps", "records",
                                                    "transitive_listed", "transitive_compares", "transitive_removed", "edges",
                                                    "max_in_records", "table_slots", "probe_used", "reduction_used", "big_sources", "deferred_sources", "probe_rounds")},
            "algorithmic_bytes_total": alg["total"],
            "device": eng.device_name(),
        }
        if stats.get("probe_used") == 2 and world == 1 and ms["keys"] > 0:
            # every kernel of a step that takes 2 % of it or more: live HIP-event time (alga_prefsuf_stats), the bytes the kernel has to
            # move by its own definition (DESIGN.md section 5 lists the formulas), the counter traffic where profiled on this build
            n, E = n_nodes, int(stats["edges"])
            eq = (W + 3 + 3) // 4
            runs_per_node = 1.0 + 2.0 * (stats["windows_probed"] / n_src - 1.0) / (min(64, lo - max(lo - 63, min(lo, 16)) + 1) + 1.0)
            nb = int(stats["table_slots"])
            rk = [("k_node_runs", ms["keys"], n * (4 * W + 4) + n * (13 + 8 * runs_per_node), "VALU-bound: ~1650 vector instructions per node"),
                  ("k_rs_hist + k_rs_scan + k_rs_scatter", ms["sort"], 3 * (4 * n + 2 * 8 * n) - 4 * n,
                   "the engine's own radix sort of (key, id) (radix_sort.hip): the 29 key bits the directory needs in 3 passes of 10; per pass 4 B (histogram) + 8 B in + 8 B out "
                   "per pair, the first pass makes the ids up instead of reading them"),
                  ("k_tgt_gather", ms["gather"], n * (4 * W + 8 + 16 * eq), "one isolated 64-byte row per entry: 128 bytes fetched for it (not run for a build the pile path keeps)"),
                  ("k_tgt_dir", ms["dir"], 4 * n + 16 * (nb + 1), "includes the zero fill of the directory (16 B per bucket) in front of the kernel"),
                  ("k_pile_build + k_pile_runs_consensus + k_pile_own_ids", ms["pile"], n * (4 * W + 8 + 16 + 16) + 64 * (n / 6.0) + n * 16 + (n / 6.0) * (128 + 48),
                   "pile records of the key order: every node's row read once BY ID (no entry array is built for a build the pile path keeps: one isolated row per entry, "
                   "128 bytes fetched for it), its sorted (key, id) pair and a directory record, 64 B written per k-mer group (~6 entries) and a 16-byte side record per entry; "
                   "then the run list of each pile: side records read, two 64-byte run lists in and 48 bytes out per group; part of the index build"),
                  (probe_kernel if first_dominates else first_name, ms["probe_pairs"], own_bytes, own_def),
                  ("k_probe_clustered" + (" + k_pile_deg" if piled else ""), ms["probe"] - ms["probe_pairs"], alg_probe_launch * (deferred / n_src) + (16 * n if piled else 0),
                   "the sources handed on, priced by SURVEY section 8(d)'s per-source bytes (this kernel does verify pairwise)" + ("; + the streaming pass that moves the out-degrees (16 B per node)" if piled else "")),
                  ("scan + k_local_emit_* + k_sort_rows_list", ms["emit"], n * 16 + E * 12, None)]
            out["roofline_kernels"] = []
            for name, kms, ab, note in rk:
                if kms < 0.02 * ms_step or (piled and name == "k_tgt_gather"):      # (a build the pile path keeps: that kernel only looks at the sample's counters)
                    continue
                head = name.split()[0]
                if head == "rocprim":
                    tr = None                              # several dispatches of different kernels per sort: the per-dispatch means of profiles/hbm_traffic.json do not add up to one sort
                elif head == "scan":
                    tr = sum(filter(None, (traffic_of(traffic, q) for q in ("k_scan", "k_local_emit", "k_sort_rows")))) or None
                else:
                    tr = sum(filter(None, (traffic_of(traffic, q.split()[0]) for q in name.split(" + ")))) or None
                phys = tr if tr else ab                        # counters where profiled on these sources, else the kernel's own byte model
                ent = {"kernel": name, "ms": kms, "share_of_step": kms / ms_step, "own_model_bytes": int(ab), "frac_own_model": ab / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       "traffic": tr, "achieved": phys / (kms * 1e-3) / 1e9, "frac": phys / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, "basis": "counters" if tr else "own_byte_model",
                       "traffic_over_own_model": (tr / ab) if tr else None}
                if note:
                    ent["note"] = note
                out["roofline_kernels"].append(ent)
            out["index_build_ms"] = {k: ms[k] for k in ("keys", "sort", "gather", "dir", "pile")}
            if piled:
                out["roofline"]["pile_path"] = {
                    "note": "the timed steps probe through PILES (alga_amd/csrc/prefsuf_pile.hip): one compare of a source against the consensus of a minimizer's targets instead of one per target",
                    "sampled_buckets": int(s.get("pile_buckets", 0)), "sampled_irregular_buckets": int(s.get("pile_irregular", 0)), "deferred_sources": deferred}
        if supplement:
            ps = stats["pkb"]
            ab = sum(ps["kmers"]) * 24 + sum(ps["can_align_calls"]) * 8 * W + sum(ps["edges_after"]) * 8
            out["supplement"] = {"ms": ms["supplement"], "exact_path_ms": ms_step - ms["supplement"], "kmers": ps["kmers"], "can_align_calls": ps["can_align_calls"],
                                 "edges_after_round": ps["edges_after"], "edges_exact": int(stats["edges"]), "groups": ps["groups"],
                                 "group_hist_2_3_4_7_15_31_64_more": ps.get("group_hist"),
                                 "algorithmic_bytes": int(ab), "achieved": ab / (ms["supplement"] * 1e-3) / 1e9, "frac": ab / (ms["supplement"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "per_unit": "SURVEY.md section 8(d) for cfg 5: 24 B per LI k-mer + 8W B per canAlign call (+ 8 B per edge key of the graph merged per round); "
                                             "the sorts are the engine's own radix sort (radix_sort.hip), the merge of a round's additions rocPRIM's, the group joins k_pkb_groups_*; from round 1 on a round's sort runs on a second stream beside the round before (DESIGN.md section 9)"}
        if first is not None:
            first["warm_ms"] = ms_step - (ms["supplement"] if supplement else 0.0)
            first["first_over_warm"] = first["first_call_ms"] / first["warm_ms"]
            out["first_call"] = first
        if world > 1:
            if err > 0.01:
                out["supplement"]["n_gpu_form"] = "k-mer groups dealt out over the ranks by hash (alga_pkb_shard_*): the exact graph broadcast from rank 0, each round's additions all-gathered, every rank merges them all; counters are rank 0's"
            out["multi_gpu_form"] = multi_form
            out["multi_gpu_validation"] = "the N-rank path has not run over RCCL on hardware (no multi-GPU node available to the builder): N-rank graph == one-GPU graph is checked over gloo and as N ranks on one GPU only"
        out["src_sha256"] = src_sha
        if world == 1 and not args.no_pcie and not supplement:
            # the same graph through the host-buffer entry point (packed host reads in, host edge list out): never `value`
            if host_words is None:
                # host rows as the reference-side adapter lays them out (alga_adapter::NodeArrays: exactly the Bitset blocks of a read -- 9 words
                # for 150-bp reads, not the 16 of the engine's own HBM layout); the engine re-strides on the device
                stride_host = max(1, W)
                host_words = np.ascontiguousarray(d_words[:, :stride_host].cpu().numpy().view(np.uint32))
                host_lens = d_lens.cpu().numpy()
            # ALGA's node set comes in twin pairs (node 2k = reverse complement of node 2k + 1): the adapter sends the rows of the odd nodes
            # alone and the engine rebuilds the even ones on the device (alga_prefsuf_params.twin_rows) -- what is timed here
            twin_words = np.ascontiguousarray(host_words[1::2])
            best, m_host, dg_host = eng.prefsuf_host_timed(twin_words, host_lens, lo, rs, repeat=3, twin_rows=True, digest=True)
            st_h = eng.last_stats()
            full_best, m_full, _ = eng.prefsuf_host_timed(host_words, host_lens, lo, rs, repeat=2)
            out["pcie_inclusive"] = {"ms_per_graph": best * 1e3, "edges_per_sec": m_host / best,
                                     "edges_equal_resident": bool(m_host == int(n_edges)),
                                     "edges_digest_equal_resident": bool(digest_timed is not None and dg_host == digest_timed),
                                     "host_bytes_in": int(twin_words.nbytes + host_lens.nbytes), "host_bytes_out": int(m_host) * 12,
                                     "phases_ms": {k: st_h[k] for k in ("host_ms_check", "host_ms_upload", "host_ms_build", "host_ms_download")},
                                     "all_rows_uploaded": {"ms_per_graph": full_best * 1e3, "host_bytes_in": int(host_words.nbytes + host_lens.nbytes),
                                                           "edges_equal": bool(m_full == m_host)},
                                     "note": "alga_prefsuf_build_host from pageable host arrays as the adapter lays them out (the Bitset's own blocks, 9 words per 150-bp read; rows of the ODD nodes only, the "
                                             "reverse-complement twins rebuilt on the device: twin_rows; all_rows_uploaded = the same without that): "
                                             "staged H2D of the packed reads (pinned buffers, 8 copy threads; the lengths as one byte per node) + re-stride + build + staged D2H of the edge triples; wall time of the C call, best of 3"}
            # ... and with the graph brought down in COMPACT form (a degree byte per node + 5 bytes per edge: what the reference-side adapter consumes,
            # alga_adapter::fill_graph_compact), from pageable arrays and from pinned ones (alga_host_alloc: no staging copy)
            ec, best_c = eng.prefsuf_host_compact(twin_words, host_lens, lo, rs, twin_rows=True, repeat=3)
            st_c = eng.last_stats()
            dg_c = alga_amd.engine.host_edges_digest(ec)
            del ec
            pw = eng.host_array(twin_words.shape, np.uint32)
            pl = eng.host_array(host_lens.shape, np.int32)
            pw[...] = twin_words
            pl[...] = host_lens
            ep, best_p = eng.prefsuf_host_compact(pw, pl, lo, rs, twin_rows=True, repeat=3)
            st_p = eng.last_stats()
            dg_p = alga_amd.engine.host_edges_digest(ep)
            del ep, pw, pl
            out["pcie_inclusive"]["compact_edges"] = {
                "ms_per_graph": best_c * 1e3, "edges_digest_equal_resident": bool(digest_timed is not None and dg_c == digest_timed),
                "host_bytes_out": int(m_host) * 5 + n_nodes, "phases_ms": {k: st_c[k] for k in ("host_ms_check", "host_ms_upload", "host_ms_build", "host_ms_download")},
                "pinned_node_arrays": {"ms_per_graph": best_p * 1e3, "edges_digest_equal_resident": bool(digest_timed is not None and dg_p == digest_timed),
                                       "phases_ms": {k: st_p[k] for k in ("host_ms_check", "host_ms_upload", "host_ms_build", "host_ms_download")}},
                "note": "alga_prefsuf_build_host_compact: the same upload, the graph down as {degree byte per node, u32 neighbour + offset byte per edge}"}
            # SURVEY.md section 8(d)'s headline is END TO END from packed host reads; `value` (the contract's number) is the HBM-resident rate.
            # Quoted for the form the adapter uses (compact edges, pageable node arrays); every form's list is digest-checked against the timed one
            e2e = min(best, best_c)
            out["value_end_to_end"] = m_host / e2e
            out["ms_end_to_end"] = e2e * 1e3
            out["end_to_end_form"] = "compact edges" if best_c <= best else "edge triples"
        if not args.no_cpu_baseline and world == 1:        # the CPU baseline is a rank-0, N=1 measurement
            try:
                cores = len(os.sched_getaffinity(0))
            except AttributeError:
                cores = os.cpu_count() or 1
            cores = max(1, min(cores, 16))          # the GPU box gives one GPU's CPU share: 16 cores
            cb = cpu_baseline_reference(sample_codes, cores, eng, err) if sample_codes is not None else None
            if cb is not None and err > 0:
                cb["note"] = ("reads with errors: the reference's own --threads > 1 result differs by a few edges from run to run (its creator races on ties, "
                              "SURVEY.md section 0.6), so graph_bytes_equal_gpu is informative only here; the exact path equals the --threads=1 dump (tests/test_gpu_fullsize.py)")
            if cb is None:
                hw = host_words if host_words is not None else d_words[:200_000].cpu().numpy().view(np.uint32)
                hl = host_lens if host_lens is not None else d_lens[:200_000].cpu().numpy()
                cb = cpu_baseline_port(hw, hl, lo, rs, min(n_nodes, 200_000))
            out["cpu_baseline"] = cb
    return out


if __name__ == "__main__":
    main()
