"""SLAM --extract-taxid / --extract-out (tools/slam_main.cpp; include/kslam_taxreads.h): the usage names the options, every
refusal fires with its message before a file is written, and on the fixture the '#' files are what the plain-Python restatement
(tests/taxreads_ref.py) selects from R1.fq / R2.fq by that run's _PerRead ids, while no other output moves by a byte."""
import importlib

import pytest

from test_cli import _fixture_case, _run

OPTIONS = [b"--extract-taxid arg", b"--extract-out arg", b"--extract-include-children", b"--extract-include-parents", b"--extract-exclude"]


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    for o in OPTIONS:
        assert o in r.stdout, o


REFUSALS = [
    (["--extract-taxid", "562"], b"option '--extract-taxid' needs '--extract-out'"),
    (["--extract-out", "x#.fq"], b"option '--extract-out' needs '--extract-taxid'"),
    (["--extract-include-children"], b"option '--extract-include-children' needs '--extract-taxid'"),
    (["--extract-include-parents"], b"option '--extract-include-parents' needs '--extract-taxid'"),
    (["--extract-exclude", "--extract-out", "x#.fq"], b"needs '--extract-taxid'"),
    (["--extract-taxid", "0", "--extract-out", "x#.fq"], b"the argument ('0') for option '--extract-taxid' is invalid"),
    (["--extract-taxid", "562,0", "--extract-out", "x#.fq"], b"for option '--extract-taxid' is invalid"),
    (["--extract-taxid", "56x", "--extract-out", "x#.fq"], b"the argument ('56x') for option '--extract-taxid' is invalid"),
    (["--extract-taxid", "562,,7", "--extract-out", "x#.fq"], b"for option '--extract-taxid' is invalid"),
    (["--extract-taxid", "-5", "--extract-out", "x#.fq"], b"for option '--extract-taxid' is invalid"),
    (["--extract-taxid", "562", "--extract-out", "x#.fq", "--just-align"], b"option '--extract-taxid' cannot be combined with '--just-align'"),
    (["--extract-out", "x#.fq", "--just-align"], b"option '--extract-out' cannot be combined with '--just-align'"),
    (["--extract-taxid", "562", "--extract-taxid", "7,9", "--extract-out", "x.fq"], b"the argument of '--extract-out' must contain a '#' (replaced by 1 and 2)"),
]


@pytest.mark.parametrize("args,message", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_refusals_write_no_file(kslam, tmp_path, args, message):
    r = _run(["--db=db", "--output-file=out"] + args + ["R1.fq", "R2.fq"], tmp_path, check=False)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    left = sorted(p.name for p in tmp_path.iterdir() if p.name != "log.txt")
    assert left == [], left


def _names(fastq):
    lines = fastq.split(b"\n")
    return [lines[4 * k][1:].split(b"/")[0] for k in range(len(lines) // 4)]


@pytest.mark.gpu
def test_the_extracted_reads_and_nothing_else_moves(kslam, tmp_path):
    import kreport_ref as K
    import ref_loop_case as RL
    import taxreads_ref as R
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    r1, r2 = (tmp_path / "R1.fq").read_bytes(), (tmp_path / "R2.fq").read_bytes()
    number = {name: k for k, name in enumerate(_names(r1))}
    lines = [x for x in plain["out_PerRead"].split(b"\n") if x]
    records = [number[x.split(b"\t")[0]] for x in lines]
    ids = [int(x.rsplit(b"\t", 1)[1]) for x in lines]
    assert len(ids) > 10 and len(number) >= len(ids)
    # a species-level id of this run: the species above the most frequent id (or that id itself when it is a species already)
    tree = K.Tree(case["taxdb"])
    species = [i for i in set(ids) if i and tree.rank.get(i) == b"species"] or \
              [tree.parent[i] for i in set(ids) if i in tree.node and tree.rank.get(tree.parent.get(i)) == b"species"]
    assert species
    chosen = max(species, key=lambda s: sum(R.matched(case["taxdb"], [s], R.CHILDREN, ids)))
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    for flags, mode in ((["--extract-include-children"], R.CHILDREN), (["--extract-include-children", "--extract-exclude"], R.CHILDREN | R.EXCLUDE)):
        _run(base + ["--extract-taxid", str(chosen), "--extract-out", "x#.fq"] + flags + ["R1.fq", "R2.fq"], tmp_path)
        exp, n_exp = R.select(case["taxdb"], [chosen], mode, r1, r2, records, ids)
        assert n_exp[0] > 0 and n_exp[1] > 0
        assert [(tmp_path / "x1.fq").read_bytes(), (tmp_path / "x2.fq").read_bytes()] == exp, flags
        for n, b in plain.items():
            assert (tmp_path / n).read_bytes() == b, n
        assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
