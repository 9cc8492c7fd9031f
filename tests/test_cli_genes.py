"""SLAM --genes-out (tools/slam_main.cpp; include/kslam_genes.h): the file is the writer applied to the host twin's rows on the
final arrays of the same inputs, with --just-align, without --sam-file and single-end too; without the option no file appears
and no other output moves by a byte."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import genes_ref as R
from test_cli import _fixture_case, _run


def test_usage_names_the_option(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    assert b"--genes-out arg" in r.stdout


def _twin_table(kslam, tmp_path, case, per_batch, single=False):
    """the same inputs through the Python loop: every batch's final arrays, concatenated, through kslam_tail_genes and the writer"""
    GN = importlib.import_module("kslam_amd.genes")
    D = importlib.import_module("kslam_amd.db")
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    db = D.Database.load(os.path.join(str(tmp_path), "db", "database"))
    c = kslam.Context()
    h1, h2 = kslam.HostBuffer(len(case["r1"]) + 64), kslam.HostBuffer(len(case["r2"]) + 64)
    got = []
    try:
        h1.a[:len(case["r1"])] = np.frombuffer(case["r1"], dtype=np.uint8)
        h2.a[:len(case["r2"])] = np.frombuffer(case["r2"], dtype=np.uint8)
        bases_pp, lens_p = db.entry_pointers()
        c._chk(c._L.kslam_set_index(c._h, db.n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
        S.classify_stream(c, db, h1.ptr, len(case["r1"]), None if single else h2.ptr, 0 if single else len(case["r2"]), per_batch,
                          T.TailParams.default(paired=not single),
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(rp), np.array(pr))))
    finally:
        c.close()
        h1.close()
        h2.close()
    rp, at = [], 0
    for r, p in got:
        r = r.astype(R.READ_PAIR_DT)
        r["first"] += at
        at += len(p)
        rp.append(r)
    rows, st = GN.tail_genes(db, np.concatenate(rp), np.concatenate([p.astype(R.PAIRED_OVERLAP_DT) for _, p in got]))
    return GN.table_bytes(db, rows), rows, GN


@pytest.mark.gpu
def test_the_table_and_nothing_else_moves(kslam, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "genes.tsv").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    _run(base + ["--genes-out", "genes.tsv", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    table = (tmp_path / "genes.tsv").read_bytes()
    exp, rows, GN = _twin_table(kslam, tmp_path, case, per_batch)
    assert table == exp and len(rows) > 0
    lines = GN.parse(table)
    assert [r["gene"] for r in lines] == rows["gene"].tolist() and all(r["alignments"] > 0 and r["overlap_bases"] > 0 for r in lines)
    assert [r["locus"].encode() for r in lines] == [case["entries"][r["entry"]]["locusTag"] for r in lines]
    # --just-align, and without --sam-file: the same final read pairs, the same table
    _run(["--db=db", "--just-align", "--sam-file", "ja.sam", "--genes-out=ja.tsv", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    assert (tmp_path / "ja.tsv").read_bytes() == exp
    _run(["--db=db", "--just-align", "--genes-out=bare.tsv", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    assert (tmp_path / "bare.tsv").read_bytes() == exp
    _run(["--db=db", "--output-file=nosam", "--genes-out=nosam.tsv", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    assert (tmp_path / "nosam.tsv").read_bytes() == exp and (tmp_path / "nosam_PerRead").read_bytes() == plain["out_PerRead"]
    # single-end
    _run(["--db=db", "--output-file=se", "--genes-out=se.tsv", "--num-reads-at-once", str(per_batch), "R1.fq"], tmp_path)
    exp_se, rows_se, _ = _twin_table(kslam, tmp_path, case, per_batch, single=True)
    assert (tmp_path / "se.tsv").read_bytes() == exp_se and len(rows_se) > 0
