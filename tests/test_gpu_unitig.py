"""The unitig graph on the GPU (alga_unitigs_device, alga_write_unitig_gfa_device): every array equal to the Python definition
(tests/unitig_checker.py) on the reference's graph dumps, on the engine's own graphs before and after the triangle cut, on the
hand-written cases of tests/unitig_cases.py; a path long enough for more than 16 jump rounds; the 1 M read set; the GFA export of the
ragged rows; refusals; the command line; the compiler's resource report of the new kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import gen_reads
import gfa_writer as G
import oracle_lib as O
import unitig_cases as K
import unitig_checker as U
from alga_amd import workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("words", "word_off", "len", "path_node", "path_pos", "path_off", "edges")
COUNTS = ("edges_in", "edges_sym", "twins_added", "compactable", "cycles_cut", "isolated_skipped", "longest_nodes", "longest_bases", "total_bases",
          "total_nodes")


@pytest.fixture(scope="module", params=["jumping", "ruling_set"])
def eng(request):
    """every test twice: plain pointer jumping (what sets below 2^16 nodes get by default), and with the ruling set ranked first
    (option "unitig_ruling": what larger sets get)"""
    e = alga_amd.Engine(0)
    e.ruling = request.param == "ruling_set"
    e.set_option("unitig_ruling", 1 if e.ruling else 0)
    yield e
    e.close()


def _dev(eng, words, lens):
    import torch
    dev = torch.device("cuda", eng.device)
    w = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
    return w, torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)


def assert_same(got, want, what=""):
    assert got["n_pairs"] == want["n_pairs"], what
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    for k in COUNTS:
        assert got["info"][k] == want["info"][k], (what, k)


def equals_checker(eng, words, lens, edges, d_edges=None, shuffle_seed=None):
    """device == definition, with and without SKIP_ISOLATED (and for a shuffled edge order); returns the device result without the flag"""
    w, l = _dev(eng, words, lens)
    first = None
    for skip in (False, True):
        want = U.unitigs(words, lens, edges, skip_isolated=skip)
        u = eng.unitigs(w, l, d_edges[0] if d_edges else edges, n_edges=d_edges[1] if d_edges else None, skip_isolated=skip)
        got = u.to_host()
        assert_same(got, want, "skip=%s" % skip)
        if shuffle_seed is not None and len(edges):
            perm = np.random.default_rng(shuffle_seed).permutation(len(edges))
            assert_same(eng.unitigs(w, l, np.ascontiguousarray(edges[perm]), skip_isolated=skip).to_host(), want, "shuffled, skip=%s" % skip)
        first = first or got
    return first


@pytest.mark.parametrize("graph", K.GOLDEN_GRAPHS)
def test_reference_dump(eng, golden_dir, graph):
    words, lens, edges = K.golden(golden_dir, graph)
    got = equals_checker(eng, words, lens, edges, shuffle_seed=5)
    live, sym, oriented, longest = K.GOLDEN_TABLE[graph]
    assert (got["info"]["edges_sym"], 2 * got["n_pairs"], got["info"]["longest_nodes"]) == (sym, oriented, longest)


def _nodes(n, length, G_, seed, err=0.0, min_length=None):
    codes, lens = gen_reads.sample_reads(n, length, G_, seed, err, min_length)
    rc = np.zeros_like(codes)
    for i in range(n):
        rc[i, : lens[i]] = 3 - codes[i, : lens[i]][::-1]
    codes = np.stack([rc, codes], axis=1).reshape(2 * n, length)
    lens = np.repeat(lens, 2)
    return alga_amd.pack_reads(codes, lens), lens.astype(np.int32)


@pytest.mark.parametrize("n,length,G_,seed,err,minlen,lo,rs", [
    (3000, 100, 6000, 71, 0.0, None, 55, 77),        # error-free
    (3000, 150, 9000, 77, 0.02, None, 82, 116),      # 2 % errors: exact graph, then the supplement
    (2500, 150, 5000, 72, 0.0, 90, 70, 100),         # several read lengths, contained / prefix reads kept
    (3000, 100, 6000, 78, 0.0, None, 40, 60),        # l = 40
])
def test_engine_graphs_before_and_after_the_triangle_cut(eng, n, length, G_, seed, err, minlen, lo, rs):
    words, lens = _nodes(n, length, G_, seed, err, minlen)
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, lo, rs)
    if err > 0:
        live = lens[lens > 0]
        p = eng.pkb_params(float(live.mean()), err, min(2 * length // 3, 60))
        d, m = eng.pkb_supplement_device(w, l, d, m, p)
    e = alga_amd.engine.device_edges_to_numpy(d, m)
    assert m > 0
    equals_checker(eng, words, lens, e, d_edges=(d, m), shuffle_seed=seed)
    d2, m2, removed = eng.cut_triangles_device(len(lens), d, m, max(250, int(1.75 * length)))
    e2 = alga_amd.engine.device_edges_to_numpy(d2, m2)                       # grouped by src, NOT sorted by (src, dst)
    equals_checker(eng, words, lens, e2, d_edges=(d2, m2))


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("case", sorted(K.CASES))
def test_hand_written_case(eng, case, skip):
    c = K.CASES[case]
    words, lens = K.nodes_of(c["reads"])
    edges = np.array(c["edges"], dtype=np.int32).reshape(-1, 3)
    for e in (edges, np.ascontiguousarray(edges[::-1])):
        got = eng.unitigs(words, lens, e, skip_isolated=skip).to_host()
        K.assert_equals_expected(got, case, skip)
        assert_same(got, U.unitigs(words, lens, e, skip_isolated=skip))


def test_many_rings(eng):
    """rings of every length 3 .. 40 and their twin rings side by side, one chain between them: every cycle is cut at its own m"""
    reads, edges, k = [], [], 0
    for c in range(3, 41):
        for i in range(c):
            reads.append("ACGTACGT"[i % 4:] + "ACGTACGT"[: i % 4])
            edges.append((2 * (k + i) + 1, 2 * (k + (i + 1) % c) + 1, 1 + i % 3))
        k += c
    for i in range(30):
        reads.append(K.A8)
        if i:
            edges.append((2 * (k + i - 1) + 1, 2 * (k + i) + 1, 2))
    words, lens = K.nodes_of(reads)
    got = equals_checker(eng, words, lens, np.array(edges, dtype=np.int32), shuffle_seed=3)
    assert got["info"]["cycles_cut"] == 38 and got["n_pairs"] == 39


def test_long_path_runs_more_than_16_rounds(eng, tmp_path):
    """200 k error-free reads of one genome at the coverage and read length of f1_cfg1: after the triangle cut one path holds all
    157 551 surviving reads (confirmed with the CPU oracle's build and cut and the checker), so pointer jumping needs 18 rounds."""
    codes, _ = gen_reads.sample_reads(200000, 100, 400000, 91)
    fasta = str(tmp_path / "long.fasta")
    workload.write_fasta_fast(fasta, codes)
    nd = alga_amd.ingest_files(fasta)
    os.unlink(fasta)
    words, lens = nd["words"], nd["len"]
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, nd["min_overlap"], nd["rsoemo"])
    d2, m2, _ = eng.cut_triangles_device(len(lens), d, m, max(250, int(1.75 * nd["LEN"])))
    e2 = alga_amd.engine.device_edges_to_numpy(d2, m2)
    u = eng.unitigs(w, l, d2, n_edges=m2, skip_isolated=True)
    print("long path:", u.info)
    assert u.info["longest_nodes"] > 65536
    if not eng.ruling:
        assert u.info["rank_rounds"] > 16                                    # (the ruling set ranks a list 1/64 as long: fewer rounds)
    assert_same(u.to_host(), U.unitigs(words, lens, e2, skip_isolated=True))


def test_cfg2_1M(eng):
    import torch
    n_reads, read_len, genome, seed, _ = workload.CONFIGS["cfg2_1M_150bp"]
    wl = workload.device_build(n_reads, read_len, genome, seed, device="cuda:%d" % eng.device)
    w, l = wl["words"], wl["lens"]
    torch.cuda.synchronize()                                                 # the engine's own stream orders with no other
    d, m = eng.prefsuf_device(w, l, wl["min_overlap"], wl["rsoemo"])
    d2, m2, _ = eng.cut_triangles_device(int(l.shape[0]), d, m, max(250, int(1.75 * read_len)))
    e2 = alga_amd.engine.device_edges_to_numpy(d2, m2)
    assert (e2[:, 2] > 0).all()                                              # this set has no offset-0 edge
    u = eng.unitigs(w, l, d2, n_edges=m2, skip_isolated=True)
    print("cfg2:", u.info)
    got = u.to_host()
    words, lens = w.cpu().numpy().view(np.uint32), l.cpu().numpy()
    assert_same(got, U.unitigs(words, lens, e2, skip_isolated=True))
    # device-independent properties over all nodes
    pn, pp, po = got["path_node"].astype(np.int64), got["path_pos"].astype(np.int64), got["path_off"].astype(np.int64)
    has_edge = np.zeros(len(lens), dtype=bool)
    has_edge[e2[:, 0]] = True; has_edge[e2[:, 1]] = True
    has_edge |= has_edge.reshape(-1, 2)[:, ::-1].reshape(-1)                 # an edge at the twin counts (E* is symmetric)
    kept = np.nonzero((lens > 0) & has_edge)[0]
    both = np.sort(np.concatenate([pn, pn ^ 1]))
    assert len(both) == len(kept) and (both == kept).all()                   # every live node with an edge once ...
    allp = eng.unitigs(w, l, d2, n_edges=m2).to_host()["path_node"].astype(np.int64)
    assert (np.sort(np.concatenate([allp, allp ^ 1])) == np.nonzero(lens > 0)[0]).all()   # ... and without the flag every live node once
    inner = np.ones(len(pn), dtype=bool)
    inner[po[:-1]] = False
    assert (np.diff(pp)[inner[1:]] > 0).all()                                # pos strictly increasing along a path
    # read k equals its unitig's bases at pos (error-free set): compare 2-bit codes of every node against the unitig words
    wo = got["word_off"].astype(np.int64)
    pair_of_entry = np.repeat(np.arange(got["n_pairs"]), np.diff(po))
    uw = got["words"]
    for q in range(int(lens.max())):
        sel = lens[pn] > q
        j = pp[sel] + q
        at = wo[pair_of_entry[sel]] + (j >> 4)
        ucode = (uw[at] >> (2 * (j & 15)).astype(np.uint32)) & 3
        ncode = (words[pn[sel], q >> 4] >> np.uint32(2 * (q & 15))) & 3
        assert (ucode == ncode).all(), q
    e = got["edges"].astype(np.int64)
    key = (e[:, 0] << 32) | e[:, 1]
    assert (np.diff(key) > 0).all()
    ul = np.repeat(got["len"].astype(np.int64), 2)
    tw = np.stack([e[:, 1] ^ 1, e[:, 0] ^ 1, ul[e[:, 1]] - ul[e[:, 0]] + e[:, 2]], axis=1)
    tw = tw[np.lexsort((tw[:, 2], tw[:, 1], tw[:, 0]))]
    assert (tw == e).all()                                                   # twin-symmetric and sorted
    torch.cuda.synchronize()


def _unitig_gfa_want(want, sequences):
    P = want["n_pairs"]
    rows = U.padded_rows(want)
    words2 = np.zeros((2 * P, rows.shape[1]), dtype=np.uint32)
    words2[1::2] = rows
    return G.gfa_bytes(words2, np.repeat(want["len"], 2), want["edges"], twins=True, sequences=sequences)


@pytest.mark.parametrize("graph", ["f1_cfg1.graph", "f4_varlen.aftercut.graph", "f7_pkb.supplement.graph"])
def test_write_unitig_gfa(eng, golden_dir, tmp_path, graph):
    words, lens, edges = K.golden(golden_dir, graph)
    path = str(tmp_path / "u.gfa")
    try:
        eng.set_option("gfa_chunk_mb", 1)
        for skip in (False, True):
            want = U.unitigs(words, lens, edges, skip_isolated=skip)
            u = eng.unitigs(words, lens, edges, skip_isolated=skip)
            for seqs in (True, False):
                info = eng.write_unitig_gfa(path, u, sequences=seqs)
                text, winfo = _unitig_gfa_want(want, seqs)
                assert open(path, "rb").read() == text
                os.unlink(path)
                for k in ("segments", "links", "links_merged", "bytes"):
                    assert info[k] == winfo[k], k
    finally:
        eng.set_option("gfa_chunk_mb", 256)


def test_write_unitig_gfa_long_lines_across_chunks(eng, tmp_path):
    """segments of tens of kilobases and 1 MB chunks: chunk borders fall between long lines, a chunk is never smaller than twice the longest"""
    words, lens = _nodes(60000, 100, 3000000, 79)
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, 55, 77)
    e = alga_amd.engine.device_edges_to_numpy(d, m)
    want = U.unitigs(words, lens, e, skip_isolated=True)
    u = eng.unitigs(w, l, d, n_edges=m, skip_isolated=True)
    path = str(tmp_path / "u.gfa")
    try:
        eng.set_option("gfa_chunk_mb", 1)
        info = eng.write_unitig_gfa(path, u)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    text, winfo = _unitig_gfa_want(want, True)
    assert info["bytes"] > 2 << 20
    assert open(path, "rb").read() == text


def test_ordinary_gfa_unchanged_through_the_shared_accessor(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f1_cfg1.graph")
    path = str(tmp_path / "g.gfa")
    for twins in (True, False):
        eng.write_gfa(path, words, lens, edges, twins=twins)
        assert open(path, "rb").read() == G.gfa_bytes(words, lens, edges, twins=twins)[0]


@pytest.mark.parametrize("name", sorted(K.REFUSALS))
def test_refusals_write_nothing_and_leave_the_engine_usable(eng, golden_dir, name):
    words, lens, edges = K.golden(golden_dir, "f6_l40.graph")
    before = eng.unitigs(words, lens, edges)
    snap = before.to_host()
    bw, bl, be = K.refusal_nodes(name)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.unitigs(bw, bl, be)
    assert ei.value.code == -1
    assert_same(before.to_host(), snap)                                     # the previous result is untouched
    assert_same(eng.unitigs(words, lens, edges).to_host(), snap)


def test_odd_node_count_is_refused(eng):
    words, lens = K.nodes_of([K.A8, K.C8])
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.unitigs(words[:-1], lens[:-1], np.zeros((0, 3), np.int32))
    assert ei.value.code == -1


def test_second_call_and_other_calls_in_between(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f3_paired.graph")
    a = eng.unitigs(words, lens, edges).to_host()
    w, l = _dev(eng, words, lens)
    eng.write_gfa(str(tmp_path / "g.gfa"), w, l, edges)                      # another call on the engine in between
    eng.sort_edges_device(np_to_dev(eng, edges), len(edges), len(lens))
    b = eng.unitigs(words, lens, edges)
    assert_same(b.to_host(), a)
    info = eng.write_unitig_gfa(str(tmp_path / "u.gfa"), b)
    assert info["segments"] == a["n_pairs"]
    assert_same(b.to_host(), a)                                              # writing the file changes nothing


def np_to_dev(eng, edges):
    import torch
    return torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32)).to(torch.device("cuda", eng.device))


def test_empty_graph(eng):
    words, lens = K.nodes_of([K.A8, K.C8])
    got = eng.unitigs(words, lens, np.zeros((0, 3), np.int32)).to_host()
    assert_same(got, U.unitigs(words, lens, np.zeros((0, 3), np.int32)))
    assert got["n_pairs"] == 2
    assert eng.unitigs(words, lens, np.zeros((0, 3), np.int32), skip_isolated=True).n_pairs == 0


def test_ruling_option(golden_dir):
    """the same result either way; the default is plain jumping below 2^16 nodes (15 766 here)"""
    words, lens, edges = K.golden(golden_dir, "f1_cfg1.aftercut.graph")
    e = alga_amd.Engine(0)
    try:
        a = e.unitigs(words, lens, edges)
        info_a, host_a = a.info, a.to_host()
        e.set_option("unitig_ruling", 1)
        b = e.unitigs(words, lens, edges)
        assert_same(b.to_host(), host_a)
        assert info_a["rank_rounds"] == 13 and b.info["rank_rounds"] < 13     # 7 883 nodes on one path: 2^13 > 7 882
        with pytest.raises(alga_amd.AlgaError):
            e.set_option("unitig_ruling", 2)
    finally:
        e.close()


def test_cli_writes_unitigs(golden_dir, tmp_path):
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f1_cfg1")
    try:
        f1, _ = fx.inputs()
        out, gfa = str(tmp_path / "unitigs.gfa"), str(tmp_path / "reads.gfa")
        r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta", "--unitigs=" + out, "--gfa=" + gfa], cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "Unitigs written" in r.stderr
    finally:
        fx.cleanup()
    # what the checker makes of the reference's own graph after its triangle cut
    words, lens, edges = K.golden(golden_dir, "f1_cfg1.aftercut.graph")
    want = U.unitigs(words, lens, edges, skip_isolated=True)
    text = open(out, "rb").read()
    lines = text.split(b"\n")
    assert lines[0] == b"H\tVN:Z:1.0" and lines[-1] == b""
    segs = [x.split(b"\t") for x in lines if x.startswith(b"S\t")]
    assert len(segs) == want["n_pairs"] == 1
    assert text == _unitig_gfa_want(want, True)[0]
    for _, name, seq, ln in segs:
        assert set(seq) <= set(b"ACGT") and ln == b"LN:i:%d" % len(seq)
    # --gfa= is what it is without the option
    n, e = O.parse_graph(fx.ref_graph())
    assert open(gfa, "rb").read() == G.gfa_bytes(*K.golden(golden_dir, "f1_cfg1.graph")[:2], e)[0]


def test_new_kernels_resources():
    """The compiler's resource report of unitig_kernels.hip: no VGPR spill and no scratch in any kernel, full occupancy."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "unitig_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_unitig_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: (\S*k_ut_\S*)", s)
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
    assert len(reps) == 23, sorted(reps)
    for name, rep in reps.items():
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)
        assert int(rep["Occupancy [waves/SIMD]"]) == 8, (name, rep)
