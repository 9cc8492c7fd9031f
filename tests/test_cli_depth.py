"""SLAM --depth-out / --depth-min (tools/slam_main.cpp; include/kslam_depth.h): the usage names them, the threshold without the
file dies with its message, the file is the host twin's on the batches' concatenated arrays and the one kslam_stream_classify
writes for the same inputs (without --sam-file and with --just-align too, several batches), no other output moves by a byte, and
no file appears without the option."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from test_cli import _fixture_case, _run


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    for flag in (b"--depth-out arg", b"--depth-min arg (=1)"):
        assert flag in r.stdout


def test_the_threshold_needs_the_file(kslam, tmp_path):
    r = _run(["--db=db", "--depth-min", "3", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"option '--depth-min' needs '--depth-out'" in r.stderr, r.stderr
    r = _run(["--db=db", "--depth-out", "d.bg", "--depth-min", "x", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"depth-min" in r.stderr and not (tmp_path / "d.bg").exists()


def _library_files(kslam, tmp_path, case, per_batch, just_align, min_depth):
    """the same inputs through kslam_stream_classify with kslam_stream_set_depth, and through the Python loop into the host twin
    -> (the library's file, the twin's file, the number of batches)"""
    import variants_ref as V
    D = importlib.import_module("kslam_amd.db")
    DP = importlib.import_module("kslam_amd.depth")
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    db = D.Database.load(os.path.join(str(tmp_path), "db", "database"))
    c = kslam.Context()
    h1, h2 = kslam.HostBuffer(len(case["r1"]) + 64), kslam.HostBuffer(len(case["r2"]) + 64)
    try:
        h1.a[:len(case["r1"])] = np.frombuffer(case["r1"], dtype=np.uint8)
        h2.a[:len(case["r2"])] = np.frombuffer(case["r2"], dtype=np.uint8)
        bases_pp, lens_p = db.entry_pointers()
        c._chk(c._L.kslam_set_index(c._h, db.n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
        name = str(tmp_path / "lib.bg")
        fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        P = T.TailParams.default(paired=True)
        S.classify_stream_native(c, db, h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]), per_batch, P,
                                 taxdb=None if just_align else X.TaxDB(case["taxdb"]), depth_fd=fd, depth_min=min_depth)
        os.close(fd)
        got = []
        S.classify_stream(c, db, h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]), per_batch, P,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(ov), np.array(cg), np.array(rp), np.array(pr), np.array(reads.bases_off))))
    finally:
        c.close()
        h1.close()
        h2.close()
    ents = [bytes(e["bases"]) for e in case["entries"]]
    gbases = np.frombuffer(b"".join(ents), dtype=np.uint8)
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    whole = None
    for ov, cg, rp, pr, bases_off in got:
        roff = (bases_off - bases_off[0]).astype(np.uint64)
        part = {"name": "batch", "gbases": gbases, "goff": goff, "rbases": np.zeros(int(roff[-1]), dtype=np.uint8), "roff": roff,
                "pool": cg.astype(np.uint32), "ov": ov.astype(V.OVERLAP_DT), "rp": rp.astype(V.READ_PAIR_DT), "pr": pr.astype(V.PAIRED_OVERLAP_DT)}
        whole = part if whole is None else V.concat(whole, part)
    rows, _ = DP.tail_depth(whole["goff"], whole["ov"], whole["pool"], whole["roff"], whole["rp"], whole["pr"], min_depth)
    return open(name, "rb").read(), DP.report_bytes(db, rows), len(got)


@pytest.mark.gpu
def test_the_file_and_nothing_else_moves(kslam, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    DP = importlib.import_module("kslam_amd.depth")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "d.bg").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    _run(base + ["--depth-out", "d.bg", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    bg = (tmp_path / "d.bg").read_bytes()
    lib, twin, n_batches = _library_files(kslam, tmp_path, case, per_batch, False, 1)
    assert bg == twin and bg == lib and n_batches > 1              # several batches via --num-reads-at-once
    loci = [bytes(e["locusTag"]).decode() for e in case["entries"]]
    lengths = dict(zip(loci, (len(e["bases"]) for e in case["entries"])))
    rows = DP.parse_bedgraph(bg)
    assert len(rows) > 20 and all(0 <= s < t <= lengths[name] and v >= 1 for name, s, t, v in rows)
    assert rows == sorted(rows, key=lambda r: (loci.index(r[0]), r[1]))
    assert all(not (a[0] == b[0] and a[2] == b[1] and a[3] == b[3]) for a, b in zip(rows, rows[1:]))   # adjacent runs differ in depth
    # without --sam-file, with the threshold: the per-read file stays what it was; rows are dropped, never merged
    _run(["--db=db", "--output-file=n", "--depth-out=n.bg", "--depth-min", "2", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    assert (tmp_path / "n_PerRead").read_bytes() == plain["out_PerRead"] and (tmp_path / "n").read_bytes() == plain["out"]
    deep = DP.parse_bedgraph((tmp_path / "n.bg").read_bytes())
    assert deep == [r for r in rows if r[3] >= 2] and 0 < len(deep) < len(rows)
    # --just-align: the aligned set
    _run(["--db=db", "--just-align", "--depth-out=ja.bg", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    ja = (tmp_path / "ja.bg").read_bytes()
    lib, twin, _ = _library_files(kslam, tmp_path, case, per_batch, True, 1)
    assert ja == twin and ja == lib and len(ja) > 0
