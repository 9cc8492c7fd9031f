"""SLAM --consensus-out and its four dependent options (tools/slam_main.cpp; include/kslam_consensus.h): the usage names them, a
dependent option without the file and a value outside its range die with their messages, and the file of one run of the binary
equals the file written from the host twin's rows over the same batches (with --just-align, without --sam-file and single-end
too)."""
import importlib
import os

import pytest

from test_cli import _fixture_case, _run

DEPENDENT = (("--consensus-min-depth", "2"), ("--consensus-call-permille", "600"), ("--consensus-fill", "ref"), ("--consensus-min-covered", "10"))


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    for flag in (b"--consensus-out arg", b"--consensus-min-depth arg (=1)", b"--consensus-call-permille arg (=500)", b"--consensus-fill arg (=n)",
                 b"--consensus-min-covered arg (=1)"):
        assert flag in r.stdout


def test_the_dependent_options_need_the_file_and_their_ranges(kslam, tmp_path):
    for flag, value in DEPENDENT:
        r = _run(["--db=db", flag, value, "R1.fq"], tmp_path, check=False)
        assert r.returncode != 0 and ("option '%s' needs '--consensus-out'" % flag).encode() in r.stderr, r.stderr
    for flag, value in (("--consensus-min-depth", "0"), ("--consensus-min-depth", "x"), ("--consensus-call-permille", "499"),
                        ("--consensus-call-permille", "1000"), ("--consensus-fill", "N"), ("--consensus-fill", "reference"), ("--consensus-min-covered", "-1")):
        r = _run(["--db=db", "--consensus-out", "c.fa", flag, value, "R1.fq"], tmp_path, check=False)
        assert r.returncode != 0 and (b"the argument ('" + value.encode() + b"') for option '" + flag.encode() + b"' is invalid") in r.stderr, r.stderr
        assert not (tmp_path / "c.fa").exists()


@pytest.mark.gpu
def test_the_file_equals_the_twins(kslam, tmp_path):
    import ref_loop_case as RL
    import test_gpu_consensus as G
    D = importlib.import_module("kslam_amd.db")
    CN = importlib.import_module("kslam_amd.consensus")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    world = {"case": case, "db": D.Database.load(os.path.join(str(tmp_path), "db", "database"))}
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "c.fa").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    _run(base + ["--consensus-out", "c.fa", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n                     # no other output moves
    exp, rows, seqs, stats, n_batches = G.twin_file(kslam, CN, world, per_batch)
    assert (tmp_path / "c.fa").read_bytes() == exp and len(rows) > 0 and n_batches > 1
    # the four options, --just-align, no --sam-file
    params = (2, 600, CN.FILL_REF, 10)
    _run(["--db=db", "--just-align", "--consensus-out=ja.fa", "--num-reads-at-once", str(per_batch)] + [x for kv in DEPENDENT for x in kv] + ["R1.fq", "R2.fq"],
         tmp_path)
    strict = G.twin_file(kslam, CN, world, per_batch, params=params)[0]
    assert (tmp_path / "ja.fa").read_bytes() == strict and strict != exp
    # single-end
    _run(["--db=db", "--consensus-out=se.fa", "--output-file=se", "--num-reads-at-once", str(per_batch), "R1.fq"], tmp_path)
    assert (tmp_path / "se.fa").read_bytes() == G.twin_file(kslam, CN, world, per_batch, single=True)[0]
