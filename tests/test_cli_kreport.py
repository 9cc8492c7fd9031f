"""SLAM --kraken-report (tools/slam_main.cpp; include/kslam_kreport.h): the usage names the option, the file is what the
plain-Python restatement (tests/kreport_ref.py) gives for that run's _PerRead ids, no other output moves by a byte, and the option
dies with its message next to --just-align."""
import importlib

import pytest

from test_cli import _fixture_case, _run


def test_usage_names_the_option(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert b"--kraken-report arg" in r.stdout


def test_just_align_is_refused(kslam, tmp_path):
    r = _run(["--db=db", "--just-align", "--kraken-report", "k.txt", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"option '--kraken-report' cannot be combined with '--just-align'" in r.stderr, r.stderr
    assert not (tmp_path / "k.txt").exists()


@pytest.mark.gpu
def test_the_report_and_nothing_else_moves(kslam, tmp_path):
    import kreport_ref as R
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    KR = importlib.import_module("kslam_amd.kreport")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "k.txt").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    _run(base + ["--kraken-report", "k.txt", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    report = (tmp_path / "k.txt").read_bytes()
    ids = [int(line.rsplit(b"\t", 1)[1]) for line in plain["out_PerRead"].split(b"\n") if line]
    total = (tmp_path / "R1.fq").read_bytes().count(b"\n") // 4
    assert len(ids) > 10 and total >= len(ids)
    assert report == R.text(case["taxdb"], ids, total)
    lines = KR.parse_report(report)
    assert [x for x in lines if x["code"] == "R"][0]["clade"] == sum(1 for i in ids if i)
    # --just-align: the message, and nothing runs
    r = _run(["--db=db", "--just-align", "--kraken-report=ja.txt", "R1.fq", "R2.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"--kraken-report" in r.stderr and b"--just-align" in r.stderr
