"""SLAM --classified-out / --unclassified-out / --reads-out-bgzf (tools/slam_main.cpp; include/kslam_readsplit.h): the files are the
split of the inputs by the run's own _PerRead, the '#' naming rule holds, and no other output moves by a byte."""
import gzip
import importlib

import pytest

import bgzf_check
import readsplit_ref as R
from test_cli import _fixture_case, _run


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    for flag in (b"--classified-out arg", b"--unclassified-out arg", b"--reads-out-bgzf"):
        assert flag in r.stdout, flag


def test_two_inputs_need_the_hash(kslam, tmp_path):
    """a usage error before any work: no GPU context, no log of a run"""
    for opt in ("--classified-out", "--unclassified-out"):
        r = _run(["--db=db", opt, "reads.fq", "R1.fq", "R2.fq"], tmp_path, check=False)
        assert r.returncode == 1 and b"'#'" in r.stderr and opt.encode() in r.stderr and b"Usage\tSLAM" in r.stderr
    assert not (tmp_path / "reads.fq").exists() and not (tmp_path / "log.txt").exists()


def _classified(per_read, ids):
    number = {i: k for k, i in enumerate(ids)}
    return [number[line.split(b"\t")[0]] for line in per_read.split(b"\n") if line]


@pytest.mark.gpu
def test_the_four_files(kslam, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(int(z["a_per_batch"]))]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    plain_outputs = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    args = base + ["--classified-out", "c#.fq", "--unclassified-out=u_#_x.fq", "R1.fq", "R2.fq"]
    _run(args, tmp_path)
    # SAM (but for the @PG line's command line), XML, _abbreviated and _PerRead: identical to the run without the options
    for n, b in plain_outputs.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    sel = _classified(plain_outputs["out_PerRead"], case["ids"])
    assert 0 < len(sel) < case["n_pairs"]
    exp, _ = R.split(case["r1"], case["r2"], sel)
    names = ["c1.fq", "c2.fq", "u_1_x.fq", "u_2_x.fq"]
    assert [(tmp_path / n).read_bytes() for n in names] == exp
    assert not (tmp_path / "c#.fq").exists()
    # BGZF, one kind only
    _run(base + ["--classified-out", "z#.fq.gz", "--reads-out-bgzf", "R1.fq", "R2.fq"], tmp_path)
    for k in (1, 2):
        blob = (tmp_path / ("z%d.fq.gz" % k)).read_bytes()
        assert bgzf_check.check(blob) == exp[k - 1] and gzip.decompress(blob) == exp[k - 1]
    for n, b in plain_outputs.items():
        assert (tmp_path / n).read_bytes() == b, n


@pytest.mark.gpu
def test_single_end_takes_the_name_as_it_stands(kslam, synth, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    case = RL.make_case(synth, n_pairs=300, seed=6202, paired=False)
    RL.write_case(case, tmp_path, D)
    _run(["--db=db", "--just-align", "--sam-file", "s.sam", "--classified-out", "al#.fq", "--unclassified-out", "rest.fq", "R1.fq"], tmp_path)
    c, u = (tmp_path / "al#.fq").read_bytes(), (tmp_path / "rest.fq").read_bytes()
    aligned = set()
    for line in (tmp_path / "s.sam").read_bytes().split(b"\n"):
        f = line.split(b"\t")
        if line and not line.startswith(b"@") and f[2] != b"*":
            aligned.add(f[0])
    sel = [k for k, i in enumerate(case["ids"]) if i in aligned]
    exp, _ = R.split(case["r1"], None, sel)
    assert 0 < len(sel) and [c, None, u, None] == exp
