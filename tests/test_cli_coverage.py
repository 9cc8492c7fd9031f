"""SLAM --coverage-out (tools/slam_main.cpp; include/kslam_coverage.h): the file is the report kslam_stream_classify writes for the
same inputs, with --just-align too; without the option no file appears and no other output moves by a byte."""
import importlib
import os

import pytest

from test_cli import _fixture_case, _run


def test_usage_names_the_option(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert b"--coverage-out arg" in r.stdout


def _library_report(kslam, tmp_path, case, per_batch, just_align):
    """the same inputs through kslam_stream_classify with kslam_stream_set_coverage"""
    import ctypes as C
    CV = importlib.import_module("kslam_amd.coverage")
    D = importlib.import_module("kslam_amd.db")
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    db = D.Database.load(os.path.join(str(tmp_path), "db", "database"))
    c = kslam.Context()
    h1, h2 = kslam.HostBuffer(len(case["r1"]) + 64), kslam.HostBuffer(len(case["r2"]) + 64)
    try:
        import numpy as np
        h1.a[:len(case["r1"])] = np.frombuffer(case["r1"], dtype=np.uint8)
        h2.a[:len(case["r2"])] = np.frombuffer(case["r2"], dtype=np.uint8)
        bases_pp, lens_p = db.entry_pointers()
        c._chk(c._L.kslam_set_index(c._h, db.n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
        name = str(tmp_path / "lib.cov")
        fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        sam_fd = os.open(str(tmp_path / "lib.sam"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        S.classify_stream_native(c, db, h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]), per_batch, T.TailParams.default(paired=True),
                                 taxdb=None if just_align else X.TaxDB(case["taxdb"]), sam_fd=sam_fd, coverage_fd=fd)
        os.close(fd)
        os.close(sam_fd)
        return open(name, "rb").read(), CV
    finally:
        c.close()
        h1.close()
        h2.close()


@pytest.mark.gpu
def test_the_report_and_nothing_else_moves(kslam, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "cov.tsv").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    _run(base + ["--coverage-out", "cov.tsv", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    report = (tmp_path / "cov.tsv").read_bytes()
    exp, CV = _library_report(kslam, tmp_path, case, per_batch, just_align=False)
    assert report == exp
    rows = CV.parse_report(report)
    assert rows and all(r["covered_bases"] > 0 and r["length"] == len(case["entries"][r["entry"]]["bases"]) for r in rows)
    assert [r["locus"].encode() for r in rows] == [case["entries"][r["entry"]]["locusTag"] for r in rows]
    # --just-align: the aligned set
    _run(["--db=db", "--just-align", "--sam-file", "ja.sam", "--coverage-out=ja.tsv", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    exp_ja, _ = _library_report(kslam, tmp_path, case, per_batch, just_align=True)
    assert (tmp_path / "ja.tsv").read_bytes() == exp_ja and len(CV.parse_report(exp_ja)) > 0
