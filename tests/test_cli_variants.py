"""SLAM --variants-out / --variants-min-alt / --variants-min-depth (tools/slam_main.cpp; include/kslam_variants.h): the usage
names them, a threshold without the file dies with its message, the file is the one kslam_stream_classify writes for the same
inputs (without --sam-file and with --just-align too), and no other output moves by a byte."""
import importlib
import os

import pytest

from test_cli import _fixture_case, _run


def test_usage_names_the_options(kslam, tmp_path):
    r = _run(["--help"], tmp_path, check=False)
    for flag in (b"--variants-out arg", b"--variants-min-alt arg (=2)", b"--variants-min-depth arg (=1)"):
        assert flag in r.stdout


def test_a_threshold_needs_the_file(kslam, tmp_path):
    for flag in ("--variants-min-alt", "--variants-min-depth"):
        r = _run(["--db=db", flag, "3", "R1.fq"], tmp_path, check=False)
        assert r.returncode != 0 and ("option '%s' needs '--variants-out'" % flag).encode() in r.stderr, r.stderr
    r = _run(["--db=db", "--variants-out", "v.vcf", "--variants-min-alt", "x", "R1.fq"], tmp_path, check=False)
    assert r.returncode != 0 and b"variants-min-alt" in r.stderr and not (tmp_path / "v.vcf").exists()


def _library_file(kslam, tmp_path, case, per_batch, just_align, min_alt, min_depth):
    """the same inputs through kslam_stream_classify with kslam_stream_set_variants"""
    import ctypes as C
    import numpy as np
    D = importlib.import_module("kslam_amd.db")
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    db = D.Database.load(os.path.join(str(tmp_path), "db", "database"))
    c = kslam.Context()
    h1, h2 = kslam.HostBuffer(len(case["r1"]) + 64), kslam.HostBuffer(len(case["r2"]) + 64)
    try:
        h1.a[:len(case["r1"])] = np.frombuffer(case["r1"], dtype=np.uint8)
        h2.a[:len(case["r2"])] = np.frombuffer(case["r2"], dtype=np.uint8)
        bases_pp, lens_p = db.entry_pointers()
        c._chk(c._L.kslam_set_index(c._h, db.n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
        name = str(tmp_path / "lib.vcf")
        fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        S.classify_stream_native(c, db, h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]), per_batch, T.TailParams.default(paired=True),
                                 taxdb=None if just_align else X.TaxDB(case["taxdb"]), variants_fd=fd, variants_min_alt=min_alt,
                                 variants_min_depth=min_depth)
        os.close(fd)
        return open(name, "rb").read()
    finally:
        c.close()
        h1.close()
        h2.close()


@pytest.mark.gpu
def test_the_file_and_nothing_else_moves(kslam, tmp_path):
    import ref_loop_case as RL
    import variants_ref as R
    D = importlib.import_module("kslam_amd.db")
    VR = importlib.import_module("kslam_amd.variants")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    per_batch = int(z["a_per_batch"])
    base = ["--db=db", "--sam-file", "out.sam", "--output-file=out", "--num-reads-at-once", str(per_batch)]
    _run(base + ["R1.fq", "R2.fq"], tmp_path)
    assert not (tmp_path / "v.vcf").exists()
    plain = {n: (tmp_path / n).read_bytes() for n in ("out", "out_abbreviated", "out_PerRead")}
    sam = (tmp_path / "out.sam").read_bytes()
    _run(base + ["--variants-out", "v.vcf", "R1.fq", "R2.fq"], tmp_path)
    for n, b in plain.items():
        assert (tmp_path / n).read_bytes() == b, n
    cut = lambda t: [x for x in t.split(b"\n") if not x.startswith(b"@PG")]   # noqa: E731
    assert cut((tmp_path / "out.sam").read_bytes()) == cut(sam)
    vcf = (tmp_path / "v.vcf").read_bytes()
    assert vcf == _library_file(kslam, tmp_path, case, per_batch, False, 2, 1)
    loci = [bytes(e["locusTag"]) for e in case["entries"]]
    rows = R.read_vcf(vcf, loci, [len(e["bases"]) for e in case["entries"]])
    assert rows and all(fwd + rev >= 2 for *_, fwd, rev, depth in rows)
    assert [(r["chrom"].encode(), r["pos"]) for r in VR.parse_vcf(vcf)[1]] == [(loci[e], pos + 1) for e, pos, *_ in rows]
    # without --sam-file, with the thresholds: the per-read file stays what it was
    _run(["--db=db", "--output-file=n", "--variants-out=n.vcf", "--variants-min-alt", "1", "--variants-min-depth", "3", "--num-reads-at-once",
          str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    assert (tmp_path / "n_PerRead").read_bytes() == plain["out_PerRead"] and (tmp_path / "n").read_bytes() == plain["out"]
    loose = (tmp_path / "n.vcf").read_bytes()
    assert loose == _library_file(kslam, tmp_path, case, per_batch, False, 1, 3)
    loose_rows = R.read_vcf(loose, loci, [len(e["bases"]) for e in case["entries"]])
    assert all(depth >= 3 for *_, depth in loose_rows) and {r for r in rows if r[6] >= 3} <= set(loose_rows) and len(loose_rows) > len(rows)
    # --just-align: the aligned set
    _run(["--db=db", "--just-align", "--variants-out=ja.vcf", "--num-reads-at-once", str(per_batch), "R1.fq", "R2.fq"], tmp_path)
    ja = (tmp_path / "ja.vcf").read_bytes()
    assert ja == _library_file(kslam, tmp_path, case, per_batch, True, 2, 1) and len(R.read_vcf(ja, loci, [len(e["bases"]) for e in case["entries"]])) > 0
