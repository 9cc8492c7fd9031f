"""SLAM --qc-out / --qc-max-cycles (tools/slam_main.cpp; include/kslam_readqc.h): the usage names the options, bad arguments are
refused before anything runs, the file is what the plain-Python restatement (tests/readqc_ref.py) gives for the whole FASTQ
files, and no other output moves by a byte -- with the metagenomic outputs, with --just-align and no --sam-file, single-end, and
from BGZF input."""
import importlib

import pytest

from test_cli import _fixture_case, _run


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert b"--qc-out arg" in r.stdout and b"--qc-max-cycles arg (=512)" in r.stdout


@pytest.mark.parametrize("value", ["0x", "70000", "0", "-1", ""])
def test_bad_cycle_counts_are_refused(kslam, tmp_path, value):
    r = _run(["--db=db", "--qc-out", "qc.json", "--qc-max-cycles", value, "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"option '--qc-max-cycles' is invalid" in r.stderr, r.stderr
    assert not (tmp_path / "qc.json").exists()


def test_cycles_without_a_file_are_refused(kslam, tmp_path):
    r = _run(["--db=db", "--qc-max-cycles", "100", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"option '--qc-max-cycles' needs '--qc-out'" in r.stderr, r.stderr


@pytest.mark.gpu
def test_the_report_and_nothing_else_moves(kslam, tmp_path):
    import readqc_ref as R
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    RQ = importlib.import_module("kslam_amd.readqc")
    B = importlib.import_module("kslam_amd.bgzf")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    r1, r2 = case["r1"], case["r2"]
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "qc.json").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    _run(base + ["--qc-out", "qc.json", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    report = (tmp_path / "qc.json").read_bytes()
    assert report == R.text(R.of_fastq(r1, r2))
    doc = RQ.parse(report)
    assert doc["summary"]["total_reads"] == 2 * case["n_pairs"] and doc["max_cycles"] == 512 and doc["paired"] is True
    # --just-align, no --sam-file, another number of rows
    _run(["--db=db", "--just-align", "--num-reads-at-once", str(per_batch), "--qc-out=ja.json", "--qc-max-cycles", "90", "R1.fq", "R2.fq"], tmp_path)
    assert (tmp_path / "ja.json").read_bytes() == R.text(R.of_fastq(r1, r2, 90))
    # single-end, from a BGZF copy of the file
    c = kslam.Context()
    try:
        (tmp_path / "R1.fq.gz").write_bytes(B.compress(c, r1) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    finally:
        c.close()
    _run(["--db=db", "--output-file=se", "--num-reads-at-once", str(per_batch), "--qc-out", "se.json", "R1.fq.gz"], tmp_path)
    single = R.text(R.of_fastq(r1))
    assert (tmp_path / "se.json").read_bytes() == single and b'"read2"' not in single
    _run(["--db=db", "--output-file=se_off", "--num-reads-at-once", str(per_batch), "R1.fq"], tmp_path)
    for suffix in ("", "_abbreviated", "_PerRead"):
        assert (tmp_path / ("se" + suffix)).read_bytes() == (tmp_path / ("se_off" + suffix)).read_bytes(), suffix
