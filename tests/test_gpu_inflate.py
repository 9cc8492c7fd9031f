"""include/kslam_inflate.h on the GPU: kslam_bgzf_inflate on every case of tests/inflate_cases.py (all three block types, many
blocks per member, long codes, the window edge, overlapping copies), at the workgroup and launch-round seams, on the project's
own BGZF writer, on corrupt members, and the executable reading BGZF input."""
import gzip
import importlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import inflate_cases as Cs
from test_cli import SLAM, _fixture_case, _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def Z(kslam):
    return importlib.import_module("kslam_amd.inflate")


@pytest.fixture(scope="module")
def valid():
    return Cs.valid_cases()


def test_every_valid_case(Z, ctx, valid):
    assert Z.inflate(ctx, b"") == b"" and Z.inflate(ctx, Cs.EOF_MARKER) == b""
    wrong = []
    for name, (blob, text) in valid.items():
        got = Z.inflate(ctx, blob + Cs.EOF_MARKER)
        if got != text or Z.inflate(ctx, blob) != got:          # a second call, and without the EOF marker
            wrong.append(name)
    assert not wrong


def test_member_counts_around_a_workgroup(Z, ctx):
    W = Z.WAVES_PER_WORKGROUP
    assert W >= 2
    for n in (1, W - 1, W, W + 1, 2 * W + 1):
        texts = [Cs.fastq_text(700 + 131 * k, seed=20 + k) for k in range(n)]     # no two members alike, odd lengths
        blob = b"".join(Cs.member(Cs.deflate_raw(t), t) for t in texts)
        assert Z.scan(blob) == (n, sum(map(len, texts)))
        assert Z.inflate(ctx, blob) == b"".join(texts), n
    # empty members between the others, as in cat a.gz b.gz
    one = Cs.member(Cs.deflate_raw(texts[0]), texts[0])
    assert Z.inflate(ctx, Cs.EOF_MARKER + one + Cs.EOF_MARKER + Cs.EOF_MARKER + one + Cs.EOF_MARKER) == texts[0] * 2


_ROUND_CHILD = r'''
import importlib, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
from conftest import load_kslam
import inflate_cases as Cs
K = load_kslam(); Z = importlib.import_module("kslam_amd.inflate")
texts = [Cs.fastq_text(5000 + 313 * k, seed=40 + k) for k in range(9)]
blob = b"".join(Cs.member(Cs.deflate_raw(t), t) for t in texts)
ctx = K.Context()
assert Z.inflate(ctx, blob) == b"".join(texts)
bad = bytearray(blob)                      # the CRC of member 6: behind a round seam for rounds of 1 and 4
at = sum(len(Cs.member(Cs.deflate_raw(t), t)) for t in texts[:7]) - 8
bad[at] ^= 1
try:
    Z.inflate(ctx, bytes(bad)); print("NOT_REFUSED")
except K.KslamError as e:
    assert e.status == 1 and "member 6 " in str(e) and "CRC mismatch" in str(e), str(e)
assert Z.inflate(ctx, blob) == b"".join(texts)
ctx.close()
print("ROUNDS_OK", os.environ.get("KSLAM_INFLATE_ROUND"))
'''


@pytest.mark.parametrize("round_size", ["1", "4", None])
def test_nine_members_across_round_seams(tmp_path, round_size):
    """KSLAM_INFLATE_ROUND is read once per process: every setting gets a process of its own"""
    script = tmp_path / "child.py"
    script.write_text(_ROUND_CHILD % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if k != "KSLAM_INFLATE_ROUND"}
    if round_size is not None:
        env["KSLAM_INFLATE_ROUND"] = round_size
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ROUNDS_OK %s" % round_size in r.stdout and "NOT_REFUSED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_round_trip_of_the_projects_own_writer(kslam, Z, ctx):
    B = importlib.import_module("kslam_amd.bgzf")
    rnd = np.random.default_rng(11)
    M = Cs.CHUNK
    sam = np.load(os.path.join(ROOT, "tests", "golden", "slam_loop.npz"))["a_sam"].tobytes()
    cases = [sam, (sam * 4)[:3 * M + 17], bytes(2 * M + 5), rnd.integers(0, 256, 2 * M + 9, dtype=np.uint8).tobytes(), bytes(range(256)) * 3, b"x"]
    for p in (32768, 32769):              # a random pattern repeated at the window's size and one byte over it
        pat = rnd.integers(0, 256, p, dtype=np.uint8).tobytes()
        cases.append((pat * 8)[:5 * M + 3])
    for x in cases:
        z = B.compress(ctx, x)
        assert Z.scan(z + B.EOF) == ((len(x) + M - 1) // M + 1, len(x))
        assert Z.inflate(ctx, z + B.EOF) == x, len(x)


def _fastq_like(n_bytes, seed):
    """FASTQ-like text by numpy (16 MiB of it through Python's random would take longer than the test may)"""
    rnd = np.random.default_rng(seed)
    L = 150
    rows = n_bytes // (14 + 2 * L) + 1
    rec = np.empty((rows, 10 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(rows)
    for d in range(8):
        rec[:, 8 - d] = ord("0") + (idx // 10 ** d) % 10
    rec[:, 9] = ord("\n")
    rec[:, 10:10 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rnd.integers(0, 4, (rows, L))]
    rec[:, 10 + L:13 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 13 + L:13 + 2 * L] = np.frombuffer(b"FFFFFFF:,#", dtype=np.uint8)[rnd.integers(0, 10, (rows, L))]
    rec[:, 13 + 2 * L] = ord("\n")
    return rec.tobytes()[:n_bytes]


def test_sixteen_mebibytes_of_fastq_at_level_6(Z, ctx):
    text = _fastq_like(16 << 20, seed=8)
    blob = Cs.bgzf(text) + Cs.EOF_MARKER
    n, t = Z.scan(blob)
    assert t == len(text) and 250 <= n <= 270
    assert Z.inflate(ctx, blob) == text


def test_corrupt_members_are_refused_and_the_context_goes_on(kslam, Z, ctx, valid):
    good_blob, good_text = valid["fastq_level6"]
    for name, (blob, index, kind) in Cs.corrupt_cases().items():
        with pytest.raises(kslam.KslamError) as e:
            Z.inflate(ctx, blob)
        assert e.value.status == 1 and "member %d " % index in str(e.value) and str(e.value).endswith(": " + kind), (name, str(e.value))
    assert Z.inflate(ctx, good_blob) == good_text


# ---- the executable ----
def _cl(args):
    return (SLAM + " " + " ".join(args)).encode()


def _four_files(d, out, sam, args):
    files = [(d / (out + s)).read_bytes() for s in ("", "_abbreviated", "_PerRead")]
    return files + [(d / sam).read_bytes().replace(_cl(args), b"CL")]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_binary_reads_bgzf_input(kslam, tmp_path, tag):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case(tag)
    R.write_case(case, tmp_path, D)
    for r in ("R1", "R2"):
        text = (tmp_path / (r + ".fq")).read_bytes()
        (tmp_path / (r + ".fq.gz")).write_bytes(Cs.bgzf(text) + Cs.EOF_MARKER)
        assert gzip.decompress((tmp_path / (r + ".fq.gz")).read_bytes()) == text
    tail = ["--num-reads-at-once", str(int(z[tag + "_per_batch"]))] + ([] if bool(z[tag + "_pseudo"]) else ["--no-pseudo-assembly"])
    plain = ["--db=db", "--sam-file", "p.sam", "--output-file=p"] + tail + ["R1.fq", "R2.fq"]
    _run(plain, tmp_path)
    exp = _four_files(tmp_path, "p", "p.sam", plain)
    assert exp[3] == z[tag + "_sam"].tobytes().replace(b"SLAM --db db R1.fq R2.fq", b"CL")
    for k, (r1, r2) in enumerate((("R1.fq.gz", "R2.fq"), ("R1.fq.gz", "R2.fq.gz"), ("R1.fq", "R2.fq.gz"))):
        out = "o%d" % k
        args = ["--db=db", "--sam-file", out + ".sam", "--output-file=" + out] + tail + [r1, r2]
        _run(args, tmp_path)
        assert _four_files(tmp_path, out, out + ".sam", args) == exp, (r1, r2)


def test_binary_single_end_bgzf_and_plain_gzip(kslam, synth, tmp_path):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    single = R.make_case(synth, n_pairs=400, seed=6202, paired=False)
    R.write_case(single, tmp_path, D)
    text = (tmp_path / "R1.fq").read_bytes()
    (tmp_path / "R1.fq.gz").write_bytes(Cs.bgzf(text, level=9) + Cs.EOF_MARKER)
    (tmp_path / "plain.fq.gz").write_bytes(gzip.compress(text))
    plain = ["--db", "db", "--sam-file", "p.sam", "--output-file", "p", "--num-reads-at-once", "150", "R1.fq"]
    args = ["--db", "db", "--sam-file", "o.sam", "--output-file", "o", "--num-reads-at-once", "150", "R1.fq.gz"]
    _run(plain, tmp_path)
    _run(args, tmp_path)
    assert _four_files(tmp_path, "o", "o.sam", args) == _four_files(tmp_path, "p", "p.sam", plain)
    r = _run(["--db", "db", "--output-file", "q", "plain.fq.gz"], tmp_path, check=False)
    assert r.returncode != 0 and b"plain gzip" in r.stderr and b"bgzip" in r.stderr and b"plain.fq.gz" in r.stderr
