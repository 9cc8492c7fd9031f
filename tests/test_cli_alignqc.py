"""SLAM --align-qc-out / --align-qc-max-cycles (tools/slam_main.cpp; include/kslam_alignqc.h): the usage names both options, and
bad arguments are refused before anything runs (no log.txt of a run, no report)."""
import pytest

from test_cli import _run


def _nothing_ran(tmp_path):
    """the log holds the refusal alone (SLAM logs the error it dies of): no line of a run"""
    log = tmp_path / "log.txt"
    return not log.exists() or all(b"error: " in line for line in log.read_bytes().splitlines())


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert b"--align-qc-out arg" in r.stdout and b"--align-qc-max-cycles arg (=512)" in r.stdout


@pytest.mark.parametrize("value", ["0", "65537", "x", "-1", ""])
def test_bad_cycle_counts_are_refused(kslam, tmp_path, value):
    r = _run(["--db=db", "--align-qc-out", "aq.json", "--align-qc-max-cycles", value, "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"option '--align-qc-max-cycles' is invalid" in r.stderr, r.stderr
    assert not (tmp_path / "aq.json").exists() and _nothing_ran(tmp_path)


def test_cycles_without_a_file_are_refused(kslam, tmp_path):
    r = _run(["--db=db", "--align-qc-max-cycles", "100", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"option '--align-qc-max-cycles' needs '--align-qc-out'" in r.stderr, r.stderr
    assert _nothing_ran(tmp_path)
