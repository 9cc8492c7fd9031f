"""SLAM --indels-out / --indels-min-alt / --indels-min-depth (tools/slam_main.cpp; include/kslam_indels.h): a threshold without
the file dies with its message, the usage text stays the recorded one (the switches are not listed yet), the file is the one
kslam_stream_classify writes for the same inputs and the host twin's (on the stream test's world; without --sam-file, with
--just-align and single-end too), and no other output moves by a byte."""
import importlib
import os

import pytest

from test_cli import ROOT, _run
from test_gpu_indels_stream import ID, PER_BATCH, indel_world, planted_rows, stream_files, twin_file  # noqa: F401  (the fixtures and their helpers)


def test_a_threshold_needs_the_file(kslam, tmp_path):
    for flag in ("--indels-min-alt", "--indels-min-depth"):
        r = _run(["--db=db", flag, "3", "R1.fq"], tmp_path, check=False)
        assert r.returncode != 0 and ("option '%s' needs '--indels-out'" % flag).encode() in r.stderr, r.stderr
    r = _run(["--db=db", "--indels-out", "v.vcf", "--indels-min-alt", "x", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"indels-min-alt" in r.stderr and not (tmp_path / "v.vcf").exists()
    r = _run(["--db=db", "--indels-out"], tmp_path, check=False)
    assert r.returncode != 0


def test_usage_is_still_the_recorded_text(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert r.returncode == 1 and r.stdout == open(os.path.join(ROOT, "tests", "golden", "slam_help.txt"), "rb").read()
    assert b"indels" not in r.stdout


@pytest.mark.gpu
def test_the_file_and_nothing_else_moves(kslam, ID, indel_world, tmp_path):  # noqa: F811
    import indels_ref as R
    world = indel_world
    cwd = world["tmp"]                       # write_case left db/, R1.fq and R2.fq there
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(PER_BATCH)]
    _run(base + ["R1.fq", "R2.fq"], cwd)
    assert not (cwd / "i.vcf").exists()
    plain = {n: (cwd / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (cwd / "out.sam").read_bytes()
    _run(base + ["--indels-out", "i.vcf", "--indels-min-alt", "1", "--indels-min-depth", "0", "R1.fq", "R2.fq"], cwd)
    for n, b in plain.items():
        assert (cwd / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((cwd / "out.sam").read_bytes()) == cut(sam)
    exp, rows = twin_file(kslam, ID, world)
    assert (cwd / "i.vcf").read_bytes() == exp                 # the host twin's file, byte for byte
    # the defaults are 2 and 1; without --sam-file
    _run(["--db=db", "--output-file=n", "--indels-out=n.vcf", "--num-reads-at-once", str(PER_BATCH), "R1.fq", "R2.fq"], cwd)
    assert (cwd / "n_PerRead").read_bytes() == plain["out_PerRead"] and (cwd / "n").read_bytes() == plain["out"]
    default_rows = [r for r in R.fields(rows) if r[5] + r[6] >= 2 and r[7] >= 1]
    got = ID.parse(str(cwd / "n.vcf"))
    assert [(r["pos"] - 1, r["type"], r["len"], r["SAF"], r["SAR"], r["DP"]) for r in got] == \
        [(pos, "del" if kind == R.DEL else "ins", n, fwd, rev, dp) for e, pos, kind, n, s, fwd, rev, dp in default_rows]
    have = {(r["chrom"], r["pos"] - 1, r["type"], r["len"]) for r in got}
    locus = bytes(world["case"]["entries"][0]["locusTag"]).decode()
    for e, anchor, kind, n, s in planted_rows(world):
        assert (locus, anchor, "del" if kind == R.DEL else "ins", n) in have
    # together with the SNV table: neither moves the other
    _run(["--db=db", "--indels-out=b.vcf", "--variants-out=bv.vcf", "--num-reads-at-once", str(PER_BATCH), "R1.fq", "R2.fq"], cwd)
    _run(["--db=db", "--variants-out=v.vcf", "--num-reads-at-once", str(PER_BATCH), "R1.fq", "R2.fq"], cwd)
    assert (cwd / "b.vcf").read_bytes() == (cwd / "n.vcf").read_bytes() and (cwd / "bv.vcf").read_bytes() == (cwd / "v.vcf").read_bytes()
    # --just-align, and single-end: files of the same kind
    _run(["--db=db", "--just-align", "--indels-out=ja.vcf", "--num-reads-at-once", str(PER_BATCH), "R1.fq", "R2.fq"], cwd)
    assert len(ID.parse(str(cwd / "ja.vcf"))) > 0
    _run(["--db=db", "--indels-out=se.vcf", "--indels-min-alt", "1", "--indels-min-depth", "0", "--num-reads-at-once", str(PER_BATCH), "R1.fq"], cwd)
    assert (cwd / "se.vcf").read_bytes() == twin_file(kslam, ID, world, single=True)[0]
