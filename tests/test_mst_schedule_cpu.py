"""Removal of short parallel paths without a GPU: the round schedule of alga_remove_short_parallel_paths_device (tests/mst_schedule.py) gives
the lists of the sequential restatement (tests/tips_checker.py: remove_short_parallel_paths, pinned to the reference's dumps by
tests/test_tips_golden_cpu.py), list for list, with the winners of a round run in reversed order; the worst case of the schedule; the library
exports the call; the compiler's resource report of the new kernels."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import mst_schedule as S
import oracle_lib as O
import tips_checker as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rounds at the recorded bound, largest ball: worked out once on the CPU with exactly this schedule
ROUNDS = {"f2_err2": (18, 26), "f7_pkb": (18, 43), "f4_varlen": (68, 108), "f1_cfg1": (0, 0)}


def recorded_bound(golden_dir, name):
    meta = json.load(open(os.path.join(golden_dir, "n5_aftersimplifier.json")))
    # f7_pkb has f2_err2's reads; f5_messy's bound is in the "left_out" note of the fixture file
    return meta[name]["max_offset_parallel_paths_scaled"] if name in meta else {"f7_pkb": 377, "f5_messy": 283}[name]


def both(n, edges, bound):
    g = T.graph_from_edges(n, edges)
    T.remove_short_parallel_paths(g, bound)
    h = T.graph_from_edges(n, edges)
    info = S.remove_short_parallel_paths_rounds(h, bound)
    return g, h, info


@pytest.mark.parametrize("name", ["f1_cfg1", "f2_err2", "f4_varlen", "f5_messy", "f7_pkb"])
def test_schedule_equals_the_sequential_run_on_the_graphs_after_the_cut(golden_dir, name):
    with gzip.open(os.path.join(golden_dir, name + ".aftercut.graph.gz"), "rb") as f:
        n, cut = O.parse_graph(f.read())
    for bound in (recorded_bound(golden_dir, name), 60):
        g, h, info = both(n, cut, bound)
        assert g == h, (name, bound)
        assert info["begs_run"] <= info["branching_nodes"] and len(info["winners"]) == info["rounds"]
        print(name, "bound", bound, "rounds", info["rounds"], "largest ball", info["ball_max"], "begs", info["begs_run"], "of", info["branching_nodes"])
        if bound != 60 and name in ROUNDS:
            assert (info["rounds"], info["ball_max"]) == ROUNDS[name]
        if name != "f1_cfg1":
            assert info["rounds"] > 1 and max(info["winners"]) > 1
            assert bound == 60 or sum(len(x) for x in g) < len(cut)


def test_200_random_graphs():
    most = 0
    for seed in range(200):
        n, e, bound = S.random_graph(np.random.default_rng(7000 + seed), n_max=300)
        g, h, info = both(n, e, bound)
        assert g == h, seed
        most = max(most, info["rounds"])
        # a superset of the ball gives the same lists
        if seed % 10 == 0:
            k = T.graph_from_edges(n, e)
            wide = S.remove_short_parallel_paths_rounds(k, bound, ball_of=lambda gg, v, mo: S.ball(gg, v, 2 * mo + 1))
            assert k == g and wide["rounds"] >= info["rounds"] and wide["begs_run"] == info["begs_run"]
    assert most >= 10


def test_ids_ascending_along_a_chain_is_the_worst_case():
    n, e = S.ascending_chain(120)
    g, h, info = both(n, e, 10 ** 6)
    assert g == h
    assert info["begs_run"] == 119 and info["rounds"] == info["begs_run"] and set(info["winners"]) == {1}
    assert sum(len(x) for x in g) == len(e) - 118                                     # the bubbles went
    # the same line with its ids shuffled: the same step, far fewer rounds at a bound of a few edges
    perm = np.random.default_rng(5).permutation(n)
    p = np.stack([perm[e[:, 0]], perm[e[:, 1]], e[:, 2]], axis=1)
    p = np.ascontiguousarray(p[np.argsort(p[:, 0], kind="stable")], dtype=np.int32)
    _, _, line = both(n, e, 4)
    _, _, shuffled = both(n, p, 4)
    assert line["rounds"] == line["begs_run"] and shuffled["rounds"] < line["rounds"] // 2


def test_library_exports_the_call_and_the_engine_has_the_method():
    lib = alga_amd.load_library()
    assert hasattr(lib, "alga_remove_short_parallel_paths_device")
    assert "alga_remove_short_parallel_paths_device" in alga_amd.engine.EXPORTS
    assert callable(getattr(alga_amd.Engine, "remove_short_parallel_paths"))
    hdr = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    assert int(re.search(r"#define\s+ALGA_MST_MAX_ROUNDS\s+(\d+)", hdr).group(1)) == alga_amd.engine.MST_MAX_ROUNDS
    # alga_mst_info as ctypes lays it out: 5 + 64 + 2 words of 8 bytes, 3 doubles
    assert C.sizeof(alga_amd.engine.MstInfo) == 8 * (5 + 64 + 2 + 3)
    for k in (b"k_mst_claim", b"k_mst_select", b"k_mst_run", b"k_mst_run_overflow"):
        assert k in open(alga_amd.library_path(), "rb").read()


def test_new_kernels_resources():
    """The compiler's resource report of mst_kernels.hip: no VGPR spill and no scratch in any kernel.  The three walk kernels keep one beg's
    state (5888 bytes) in LDS per wave: 27 of them fit into a CU's 160 KB, which the compiler reports as 7 waves per SIMD; k_mst_select_overflow
    needs 102 SGPRs, one step above what 8 waves per SIMD leave, and gets 7 too; the others 8."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "mst_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_mst_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_mst_[a-z_]+?)E[A-Z]", s)
        if not m:
            continue
        rep = {}
        for t in lines[i + 1:]:
            if "Function Name:" in t:
                break
            mm = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", t)
            if mm:
                rep[mm.group(1)] = mm.group(2)
        reps[m.group(1)] = rep
    assert sorted(reps) == ["k_mst_check", "k_mst_claim", "k_mst_claim_overflow", "k_mst_init", "k_mst_run", "k_mst_run_overflow", "k_mst_select",
                            "k_mst_select_overflow"], sorted(reps)
    for name, rep in reps.items():
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)
        assert int(rep["LDS Size [bytes/block]"]) == (5888 if name in ("k_mst_claim", "k_mst_select", "k_mst_run") else 0), (name, rep)
        assert int(rep["Occupancy [waves/SIMD]"]) >= 7, (name, rep)
