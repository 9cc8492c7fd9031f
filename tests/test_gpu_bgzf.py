"""include/kslam_bgzf.h on the GPU: kslam_bgzf_compress at its edges (member seams, stored members, long and overlapping
matches, the window edge, several launch rounds), its ratio on the reference loop's own SAM files, and the executable's
--sam-bgzf against the golden files and against itself under the host formatter and other lane counts."""
import gzip
import importlib
import os
import subprocess

import numpy as np
import pytest

import bgzf_check as B
from test_cli import SLAM, _fixture_case, _run

pytestmark = pytest.mark.gpu
M = B.MAX_INPUT


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def Z(kslam):
    return importlib.import_module("kslam_amd.bgzf")


def _roundtrip(Z, ctx, x):
    z = Z.compress(ctx, x)
    blob = z + Z.EOF
    assert B.check(blob) == x
    assert gzip.decompress(blob) == x
    assert Z.compress(ctx, x) == z, "a second call gave other bytes"
    return z


def test_eof_marker_is_the_headers(Z):
    assert Z.EOF == B.EOF_MARKER


def test_edge_inputs(Z, ctx):
    rnd = np.random.default_rng(11)
    text = np.load(os.path.join(os.path.dirname(__file__), "golden", "slam_loop.npz"))["a_sam"].tobytes()
    assert Z.compress(ctx, b"") == b""
    for n in (1, M - 1, M, M + 1, 3 * M + 17):
        x = (text * (n // len(text) + 1))[:n]
        z = _roundtrip(Z, ctx, x)
        assert len(B.members(z + Z.EOF)) == (n + M - 1) // M + 1
    # random bytes: every member stored, so the size is exact
    x = rnd.integers(0, 256, 4 << 20, dtype=np.uint8).tobytes()
    z = _roundtrip(Z, ctx, x)
    k = (len(x) + M - 1) // M
    assert len(z) == len(x) + 26 * k + 5 * k
    assert all(m[2] == 0 for m in B.members(z + Z.EOF)[:-1])
    # zeros: distance-1, overlapping, length-258 matches
    z = _roundtrip(Z, ctx, bytes(8 << 20))
    assert len(z) < (8 << 20) // 50
    assert all(m[2] == 1 for m in B.members(z + Z.EOF)[:-1])
    # a random pattern repeated at the window's size and one byte over it
    for p in (32768, 32769):
        pat = rnd.integers(0, 256, p, dtype=np.uint8).tobytes()
        _roundtrip(Z, ctx, (pat * 8)[:5 * M + 3])
    _roundtrip(Z, ctx, bytes(range(256)) * 3)


def test_multi_round_input(Z, ctx):
    """256 MiB: more members than one launch round holds"""
    rnd = np.random.default_rng(5)
    text = np.load(os.path.join(os.path.dirname(__file__), "golden", "slam_loop.npz"))["b_sam"]
    n = 256 << 20
    x = np.resize(text, n)
    x[rnd.integers(0, n, 1 << 16)] = rnd.integers(0, 256, 1 << 16, dtype=np.uint8)   # no two members alike
    x = x.tobytes()
    z = Z.compress(ctx, x)
    assert B.check(z + Z.EOF) == x
    assert Z.compress(ctx, x) == z


@pytest.mark.parametrize("tag", ["a", "b"])
def test_ratio_floor(Z, ctx, tag):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "slam_loop.npz"))
    x = z[tag + "_sam"].tobytes()
    c = _roundtrip(Z, ctx, x)
    assert len(x) / len(c) >= 3.0, len(x) / len(c)


def _run_env(args, cwd, env):
    r = subprocess.run([SLAM] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr.decode()


def _cl(args):
    return (SLAM + " " + " ".join(args)).encode()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_binary_sam_bgzf_equals_the_reference_loop(kslam, tmp_path, tag):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case(tag)
    R.write_case(case, tmp_path, D)
    tail = ["--num-reads-at-once", str(int(z[tag + "_per_batch"]))] + ([] if bool(z[tag + "_pseudo"]) else ["--no-pseudo-assembly"])
    args = ["--db=db", "--sam-file", "out.sam.gz", "--output-file=out", "--sam-bgzf"] + tail + ["R1.fq", "R2.fq"]
    _run(args, tmp_path)
    blob = (tmp_path / "out.sam.gz").read_bytes()
    exp = z[tag + "_sam"].tobytes().replace(b'CL:"SLAM --db db R1.fq R2.fq"', b'CL:"' + _cl(args) + b'"')
    assert B.check(blob) == exp
    plain = ["--db=db", "--sam-file", "p.sam", "--output-file=p"] + tail + ["R1.fq", "R2.fq"]
    _run(plain, tmp_path)
    for suffix in ("", "_abbreviated", "_PerRead"):
        assert (tmp_path / ("out" + suffix)).read_bytes() == (tmp_path / ("p" + suffix)).read_bytes(), suffix
    # the same file from the host formatter and from one or three lanes
    for env in ({"KSLAM_HOST_SAM_TEXT": "1"}, {"KSLAM_LANES": "1"}, {"KSLAM_LANES": "3"}):
        _run_env(args, tmp_path, env)
        assert (tmp_path / "out.sam.gz").read_bytes() == blob, env


def test_binary_sam_bgzf_single_end_and_just_align(kslam, synth, tmp_path):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    single = R.make_case(synth, n_pairs=400, seed=6202, paired=False)
    R.write_case(single, tmp_path, D)
    for mode in (["--output-file", "o"], ["--just-align"]):
        args = ["--db", "db", "--sam-file", "s.sam.gz", "--sam-bgzf", "--num-reads-at-once", "150"] + mode + ["R1.fq"]
        plain = ["--db", "db", "--sam-file", "s.sam", "--num-reads-at-once", "150"] + mode + ["R1.fq"]
        _run(args, tmp_path)
        _run(plain, tmp_path)
        got = B.check((tmp_path / "s.sam.gz").read_bytes())
        assert got == (tmp_path / "s.sam").read_bytes().replace(_cl(plain), _cl(args))
        _run_env(args, tmp_path, {"KSLAM_HOST_SAM_TEXT": "1"})
        assert B.check((tmp_path / "s.sam.gz").read_bytes()) == got
