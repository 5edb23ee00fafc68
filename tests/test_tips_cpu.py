"""Dangling-branch removal without a GPU: the library exports the call, the Engine has the method, the compiler's resource report of the
new kernels, and the Python restatement (tests/tips_checker.py) on cases small enough to work out by hand."""
import os
import re
import subprocess

import numpy as np

import alga_amd
import tips_checker as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_call_and_the_engine_has_the_method():
    lib = alga_amd.load_library()
    assert hasattr(lib, "alga_remove_dangling_branches_device")
    assert "alga_remove_dangling_branches_device" in alga_amd.engine.EXPORTS
    assert callable(getattr(alga_amd.Engine, "remove_dangling_branches"))
    assert lib.alga_abi_version() == 7                                       # the addition is additive
    hdr = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    assert int(re.search(r"#define\s+ALGA_TIPS_MAX_PASSES\s+(\d+)", hdr).group(1)) == alga_amd.engine.TIPS_MAX_PASSES
    # alga_tips_info as ctypes lays it out: 3 + 1 (two int32) + 64 + 3 words of 8 bytes, 3 doubles
    import ctypes as C
    assert C.sizeof(alga_amd.engine.TipsInfo) == 8 * (3 + 1 + 64 + 3 + 3)
    for k in (b"k_tip_find", b"k_tip_find_overflow", b"k_tip_degrees", b"k_tip_apply"):
        assert k in open(alga_amd.library_path(), "rb").read()


def test_new_kernels_resources():
    """The compiler's resource report of tip_kernels.hip: no VGPR spill and no scratch in any kernel; full occupancy except k_tip_find, whose
    8 KB of LDS per wave (the short lists, one column per lane) allow 5 waves per SIMD."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "tip_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_tip_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_tip_[a-z_]+?)E[A-Z]", s)
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
    assert sorted(reps) == ["k_tip_apply", "k_tip_check", "k_tip_degrees", "k_tip_emit", "k_tip_find", "k_tip_find_overflow", "k_tip_flags", "k_tip_keys",
                            "k_tip_rev_edges", "k_tip_rev_keys"], sorted(reps)
    for name, rep in reps.items():
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)
        assert int(rep["Occupancy [waves/SIMD]"]) == (5 if name == "k_tip_find" else 8), (name, rep)


def _clip(edges, bound, n=None):
    e = np.array(edges, dtype=np.int32).reshape(-1, 3)
    n = n or int(e[:, :2].max()) + 1
    out, counts = T.remove_dangling_branches(n, e, bound)
    return [tuple(x) for x in out.tolist()], counts


def test_a_tip_goes_and_the_path_stays():
    # 0 -> 1 -> 2 -> 3 -> 4 with offsets of 200 (the path runs past the bound), the tip 1 -> 5
    path = [(0, 1, 200), (1, 2, 200), (2, 3, 200), (3, 4, 200)]
    out, counts = _clip(path + [(1, 5, 10)], 300)
    assert out == path and counts == [1, 0, 0, 0]
    # the same tip the other way round goes in the up pass
    out, counts = _clip(path + [(5, 3, 10)], 300)
    assert out == path and counts == [0, 1, 0, 0]
    # a tip longer than the bound stays
    out, counts = _clip(path + [(1, 5, 301)], 300)
    assert len(out) == 5 and counts == [0, 0]


def test_of_two_tips_the_larger_stays_and_the_smallest_offset_per_pair_is_kept():
    out, counts = _clip([(0, 1, 5), (0, 2, 5), (0, 2, 3), (0, 2, 9)], 100)
    assert out == [(0, 1, 5)] and counts == [1, 0, 0, 0]                     # ends (3, 2) < (5, 1): the last of the sorted ends stays
    out, counts = _clip([(0, 1, 5), (0, 2, 5)], 100)
    assert out == [(0, 2, 5)]


def test_par_is_overwritten_by_a_later_neighbour():
    # beg 0: the chain 1 -> 2 -> 3 ends at 3; 2 is a neighbour of 0 too and gets par = 0, so from the end 3 only 2 -> 3 and 0 -> 2 go;
    # 0 -> 4 (offset above the bound) is no end, so 0 drops none
    g = T.graph_from_edges(5, np.array([(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 2, 1), (0, 4, 50)], dtype=np.int32))
    T.retain_only_smallest_offset(g)
    removed, found = T.dangling_pass(g, 10)
    assert removed == 2 and found == [(0, 2), (2, 3)]
    assert T.edges_from_graph(g, sort=True).tolist() == [[0, 1, 1], [0, 4, 50], [1, 2, 1]]


def test_keep_emulates_the_reference_fault():
    e = np.array([(0, 1, 200), (1, 2, 200), (2, 3, 200), (1, 5, 10), (2, 6, 10)], dtype=np.int32)
    out, counts = T.remove_dangling_branches(7, e, 300)
    assert len(out) == 3 and counts == [2, 0, 0, 0]
    out, counts = T.remove_dangling_branches(7, e, 300, keep={(1, 5)})       # never removed
    assert len(out) == 4 and counts == [1, 0, 0, 0]
    out, counts = T.remove_dangling_branches(7, e, 300, keep=[{(1, 5)}])     # kept in pass 0 only: found again and removed in pass 2
    assert len(out) == 3 and counts == [1, 0, 1, 0, 0, 0]
