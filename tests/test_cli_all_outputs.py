"""SLAM with every output option at once (tools/slam_main.cpp: one table of output files): each file is byte for byte the one a
run with that option alone writes, and <out>, <out>_abbreviated and <out>_PerRead do not move; the usage text is the recorded one
(tests/golden/slam_help.txt).  Fixture "a" of tests/test_cli.py in three batches."""
import importlib
import os

import pytest

from test_cli import ROOT, _fixture_case, _run

# an option group and the files it writes (R1FILE and R2FILE: '#' becomes 1 and 2)
OPTIONS = {
    "coverage": (["--coverage-out", "cov.tsv"], ["cov.tsv"]),
    "kreport": (["--kraken-report", "kreport.txt"], ["kreport.txt"]),
    "consensus": (["--consensus-out", "consensus.fa"], ["consensus.fa"]),
    "variants": (["--variants-out", "variants.vcf"], ["variants.vcf"]),
    "depth": (["--depth-out", "depth.bedgraph"], ["depth.bedgraph"]),
    "genes": (["--genes-out", "genes.tsv"], ["genes.tsv"]),
    "qc": (["--qc-out", "qc.json"], ["qc.json"]),
    "align_qc": (["--align-qc-out", "align_qc.json"], ["align_qc.json"]),
    "classified": (["--classified-out", "c#.fq"], ["c1.fq", "c2.fq"]),
    "unclassified": (["--unclassified-out", "u#.fq"], ["u1.fq", "u2.fq"]),
    "extract": (["--extract-include-children", "--extract-out", "x#.fq"], ["x1.fq", "x2.fq"]),   # + --extract-taxid, chosen from the run
}
MAIN = ["out", "out_abbreviated", "out_PerRead"]


def test_usage_is_the_recorded_text(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert r.returncode == 1 and r.stdout == open(os.path.join(ROOT, "tests", "golden", "slam_help.txt"), "rb").read()


@pytest.mark.gpu
def test_every_output_at_once_is_each_output_alone(kslam, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case("a")
    per_batch = -(-case["n_pairs"] // 3)

    def run(tag, options):
        d = tmp_path / tag
        d.mkdir()
        RL.write_case(case, d, D)
        _run(["--db=db", "--output-file=out", "--num-reads-at-once", str(per_batch)] + options + ["R1.fq", "R2.fq"], d)
        return d

    alone = {name: run(name, OPTIONS[name][0]) for name in OPTIONS if name != "extract"}
    main = {f: (alone["coverage"] / f).read_bytes() for f in MAIN}
    ids = [int(x.rsplit(b"\t", 1)[1]) for x in main["out_PerRead"].split(b"\n") if x]
    assert len(ids) > 10
    taxid = ["--extract-taxid", str(max(set(i for i in ids if i), key=ids.count))]
    alone["extract"] = run("extract", taxid + OPTIONS["extract"][0])
    both = run("all", taxid + [o for name in OPTIONS for o in OPTIONS[name][0]])
    assert ("Processed\t%d\t reads" % case["n_pairs"]) in (both / "log.txt").read_text()
    for name, (_, files) in OPTIONS.items():
        for f in files:
            got = (both / f).read_bytes()
            assert got == (alone[name] / f).read_bytes() and len(got) > 0, f
    for d in list(alone.values()) + [both]:
        for f in MAIN:
            assert (d / f).read_bytes() == main[f], (d.name, f)
