"""GFA 1.0 export formatted on the GPU (alga_write_gfa_device): byte for byte against the Python statement of the format
(tests/gfa_writer.py) on the golden graphs, the engine's own graphs and the supplement's; chunked output; refusals; the command line."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import gen_reads
import gfa_writer as G
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _dev(eng, words, lens):
    import torch
    dev = torch.device("cuda", eng.device)
    w = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
    return w, torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)


def _nodes(n, length, G_, seed, err=0.0, min_length=None, both_strands=True):
    codes, lens = gen_reads.sample_reads(n, length, G_, seed, err, min_length)
    if both_strands:   # node 2k = reverse complement, 2k+1 = forward
        rc = np.zeros_like(codes)
        for i in range(n):
            rc[i, : lens[i]] = 3 - codes[i, : lens[i]][::-1]
        codes = np.stack([rc, codes], axis=1).reshape(2 * n, length)
        lens = np.repeat(lens, 2)
    return alga_amd.pack_reads(codes, lens), lens.astype(np.int32)


def _same(eng, tmp_path, words, lens, edges, twins=True, sequences=True, d_edges=None):
    """the engine's file == the Python writer's text; returns (text, info)"""
    path = str(tmp_path / "g.gfa")
    w, l = _dev(eng, words, lens)
    info = eng.write_gfa(path, w, l, d_edges[0] if d_edges else edges, n_edges=d_edges[1] if d_edges else None, twins=twins, sequences=sequences)
    got = open(path, "rb").read()
    os.unlink(path)
    want, winfo = G.gfa_bytes(words, lens, edges, twins=twins, sequences=sequences)
    assert got == want
    for k in ("segments", "links", "links_merged", "bytes"):
        assert info[k] == winfo[k], k
    return got, info


@pytest.mark.parametrize("name", ["f1_cfg1", "f3_paired", "f4_varlen", "f6_l40"])
def test_golden_graph_gfa(eng, golden_dir, tmp_path, name):
    fx = O.Fixture(golden_dir, name)
    try:
        f1, f2 = fx.inputs()
        lo, rs = fx.explicit_params()
        nd = O.ingest(f1, f2, min_overlap=lo, rsoemo=rs)
    finally:
        fx.cleanup()
    n, e = O.parse_graph(fx.ref_graph())
    assert n == nd["n"]
    text, info = _same(eng, tmp_path, nd["words"], nd["len"], e)
    # every link expanded into both of its edges: the dump's edges, and the twins the reduction's per-source caps dropped from it
    have = set(map(tuple, e.tolist()))
    lens = nd["len"].astype(np.int64)
    lacking = {(b ^ 1, a ^ 1, int(lens[b] - lens[a]) + o) for a, b, o in have} - have
    assert G.expand_links(text, nd["len"]) == have | lacking
    assert info["links"] + info["links_merged"] == len(e)
    _same(eng, tmp_path, nd["words"], nd["len"], e, sequences=False)
    _same(eng, tmp_path, nd["words"], nd["len"], e, twins=False)


@pytest.mark.parametrize("n,length,G_,seed,err,minlen,lo,rs", [
    (3000, 100, 6000, 71, 0.0, None, 55, 77),
    (2500, 150, 5000, 72, 0.0, 90, 70, 100),      # several read lengths, contained / prefix reads kept
    (2000, 250, 6000, 73, 0.003, 180, 125, 180),  # long rows (16 words), errors, several lengths
])
def test_engine_graph_gfa(eng, tmp_path, n, length, G_, seed, err, minlen, lo, rs):
    words, lens = _nodes(n, length, G_, seed, err, minlen)
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, lo, rs)
    e = alga_amd.engine.device_edges_to_numpy(d, m)
    assert m > 0
    for twins in (True, False):
        for seqs in (True, False):
            _same(eng, tmp_path, words, lens, e, twins=twins, sequences=seqs, d_edges=(d, m))


def test_plain_node_set_gfa(eng, tmp_path):
    """reads of one strand only (no twins), several lengths and removed nodes: the plain layout"""
    words, lens = _nodes(3000, 120, 4000, 74, 0.0, 80, both_strands=False)
    lens = lens.copy()
    lens[::17] = 0
    words = words.copy()
    words[::17] = 0
    e = eng.prefsuf_host(words, lens, 50, 70)
    assert len(e) > 0
    _same(eng, tmp_path, words, lens, e, twins=False)


def test_supplement_graph_gfa(eng, golden_dir, tmp_path):
    meta = json.load(open(os.path.join(golden_dir, "f7_pkb.json")))
    words, lens = O.load_nodes_bin(os.path.join(golden_dir, "f7_pkb.nodes.bin.gz"))
    with gzip.open(os.path.join(golden_dir, meta["pre_graph"]), "rb") as f:
        n, pre = O.parse_graph(f.read())
    import torch
    w, l = _dev(eng, words, lens)
    d_pre = torch.from_numpy(np.ascontiguousarray(pre, dtype=np.int32)).to(w.device)
    p = eng.pkb_params(meta["avg_len"], 0.02, meta["kmer_length_bucket"])
    d, m = eng.pkb_supplement_device(w, l, d_pre.data_ptr(), len(pre), p)
    e = alga_amd.engine.device_edges_to_numpy(d, m)
    with gzip.open(os.path.join(golden_dir, "f7_pkb.supplement.graph.gz"), "rb") as f:
        assert O.graph_bytes(n, e) == f.read()
    _same(eng, tmp_path, words, lens, e, d_edges=(d, m))


def test_chunked_output_is_identical(eng, tmp_path):
    words, lens = _nodes(200000, 150, 1000000, 75)
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, 82, 116)
    a, b = str(tmp_path / "a.gfa"), str(tmp_path / "b.gfa")
    try:
        info = eng.write_gfa(a, w, l, d, n_edges=m)
        assert info["bytes"] > 30 << 20                          # dozens of 1 MB chunks
        eng.set_option("gfa_chunk_mb", 1)
        info1 = eng.write_gfa(b, w, l, d, n_edges=m)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    ta, tb = open(a, "rb").read(), open(b, "rb").read()
    assert ta == tb and info == {**info1, "ms_format": info["ms_format"], "ms_total": info["ms_total"]}
    want, _ = G.gfa_bytes(words, lens, alga_amd.engine.device_edges_to_numpy(d, m))
    assert ta == want


def test_refusals_leave_no_file(eng, tmp_path):
    words, lens = _nodes(1500, 100, 3000, 76)
    e = eng.prefsuf_host(words, lens, 55, 77)
    assert len(e) > 10
    path = str(tmp_path / "x.gfa")
    bad_order = e.copy()
    bad_order[[3, 7]] = bad_order[[7, 3]]
    bad_id = e.copy()
    bad_id[5, 1] = len(lens)
    for ww, ll, ee in ((words, lens, bad_order), (words, lens, bad_id), (words[:-1], lens[:-1], e[e[:, 0] < len(lens) - 1][: 0])):
        w, l = _dev(eng, ww, ll)
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.write_gfa(path, w, l, ee, twins=True)
        assert ei.value.code == -1
        assert not os.path.exists(path)
    # an odd n is fine in the plain layout
    w, l = _dev(eng, words[:-1], lens[:-1])
    eng.write_gfa(path, w, l, np.zeros((0, 3), np.int32), twins=False)
    assert os.path.exists(path)
    os.unlink(path)
    # a directory that does not exist
    w, l = _dev(eng, words, lens)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.write_gfa(str(tmp_path / "no_such_dir" / "x.gfa"), w, l, e)
    assert ei.value.code == -6


def test_cli_writes_gfa(golden_dir, tmp_path):
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f1_cfg1")
    try:
        f1, _ = fx.inputs()
        nd = O.ingest(f1)
        out = str(tmp_path / "out.gfa")
        r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta", "--gfa=" + out], cwd=str(tmp_path), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        n, e = O.parse_graph(fx.ref_graph())
        want, _ = G.gfa_bytes(nd["words"], nd["len"], e)
        assert open(out, "rb").read() == want
        assert "GFA written" in r.stderr
    finally:
        fx.cleanup()
