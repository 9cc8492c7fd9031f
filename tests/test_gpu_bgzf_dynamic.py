"""KSLAM_BGZF_DEFLATE_DYNAMIC (include/kslam_bgzf.h) on the GPU: kslam_bgzf_compress byte for byte against the restatement
(tests/deflate_ref.py) at every seam of the member compressor, the code builder alone against the restatement's on histograms
on both sides of its length limits, every reader on what is written, dynamic never larger than fixed, the switch itself, and
the executable's --sam-deflate dynamic against its own fixed-mode files."""
import gzip
import importlib
import subprocess

import numpy as np
import pytest

import bgzf_check as B
import deflate_cases as C
import deflate_ref as D
import inflate_ref as I
from test_cli import SLAM, _fixture_case, _run
from test_gpu_bgzf import _cl, _run_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Z(kslam):
    return importlib.import_module("kslam_amd.bgzf")


@pytest.fixture(scope="module")
def ctx(kslam, Z):
    c = kslam.Context()
    Z.set_deflate(c, Z.DEFLATE_DYNAMIC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixed_ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


def test_the_constants_are_the_headers(Z):
    assert (Z.DEFLATE_FIXED, Z.DEFLATE_DYNAMIC) == (D.FIXED, D.DYNAMIC) == (0, 1)


@pytest.mark.parametrize("name", sorted(C.INPUTS))
def test_bytes_equal_the_restatement(Z, ctx, fixed_ctx, kslam, name):
    x = C.data(name)
    exp = C.expected(name, D.DYNAMIC)
    z = Z.compress(ctx, x)
    at = 0
    for k, (m, rep) in enumerate(exp):   # member by member, so that a failure names the member and its form
        assert z[at:at + len(m)] == m, (name, k, rep.btype, rep.stored_bytes, rep.fixed_bytes, rep.dynamic_bytes)
        at += len(m)
    assert at == len(z)
    assert Z.compress(ctx, x) == z, "a second call gave other bytes"
    # readers: gzip, and the device inflater
    assert gzip.decompress(z + Z.EOF) == x
    assert importlib.import_module("kslam_amd.inflate").inflate(ctx, z + Z.EOF) == x
    # every dynamic-mode member is at most as large as its fixed-mode twin
    f = Z.compress(fixed_ctx, x)
    assert f == b"".join(m for m, _ in C.expected(name, D.FIXED))
    sizes = lambda blob: [size for _, size in I.members(blob)]
    assert len(sizes(z)) == len(sizes(f)) and all(a <= b for a, b in zip(sizes(z), sizes(f)))
    if name == "random_200000":   # every member stored: the size is exact
        k = (len(x) + C.M - 1) // C.M
        assert len(z) == len(x) + 26 * k + 5 * k


@pytest.mark.parametrize("tag", ["a", "b"])
def test_dynamic_is_smaller_on_the_golden_text(Z, ctx, fixed_ctx, tag):
    x = C.golden_text(tag)
    z, f = Z.compress(ctx, x), Z.compress(fixed_ctx, x)
    assert gzip.decompress(z + Z.EOF) == x and I.inflate(z)[0] == x
    assert len(z) < len(f), (len(z), len(f))
    assert all(a[1] <= b[1] for a, b in zip(I.members(z), I.members(f)))
    print("%s_sam: %d bytes, fixed %d (%.2f x), dynamic %d (%.2f x)" % (tag, len(x), len(f), len(x) / len(f), len(z), len(x) / len(z)))


@pytest.mark.parametrize("name", sorted(C.HISTOGRAMS))
def test_code_lengths_hook_equals_the_restatement(kslam, fixed_ctx, name):
    counts, limit = C.HISTOGRAMS[name]
    got = fixed_ctx.debug_bgzf_code_lengths(counts, limit)
    assert got == D.code_lengths(counts, limit)
    assert fixed_ctx.debug_bgzf_code_lengths(counts, limit) == got


def test_code_lengths_hook_refuses_what_it_cannot_build(kslam, fixed_ctx):
    L = kslam.lib()
    one = np.ones(300, dtype=np.uint32)
    out = np.zeros(300, dtype=np.uint8)
    for n, limit in ((1, 15), (287, 15), (20, 4), (19, 0), (19, 16)):
        assert L.kslam_debug_bgzf_code_lengths(fixed_ctx._h, one.ctypes.data, n, limit, out.ctypes.data) == kslam.KSLAM_ERR_ARG, (n, limit)
    big = np.full(4, 1 << 30, dtype=np.uint32)
    assert L.kslam_debug_bgzf_code_lengths(fixed_ctx._h, big.ctypes.data, 4, 15, out.ctypes.data) == kslam.KSLAM_ERR_ARG
    assert L.kslam_debug_bgzf_code_lengths(fixed_ctx._h, None, 4, 15, out.ctypes.data) == kslam.KSLAM_ERR_ARG


def test_the_switch(kslam, Z):
    c = kslam.Context()
    try:
        x = C.data("text_member_plus_1")
        assert Z.get_deflate(c) == Z.DEFLATE_FIXED
        fixed = Z.compress(c, x)
        Z.set_deflate(c, Z.DEFLATE_DYNAMIC)
        assert Z.get_deflate(c) == Z.DEFLATE_DYNAMIC
        assert Z.compress(c, x) == D.compress(x, D.DYNAMIC)
        for bad in (2, -1, 7):
            assert Z.lib().kslam_set_bgzf_deflate(c._h, bad) == kslam.KSLAM_ERR_ARG
            assert Z.get_deflate(c) == Z.DEFLATE_DYNAMIC
        Z.set_deflate(c, Z.DEFLATE_FIXED)
        assert Z.get_deflate(c) == Z.DEFLATE_FIXED
        again = Z.compress(c, x)
        assert again == fixed == D.compress(x, D.FIXED) and B.check(again + Z.EOF) == x
    finally:
        c.close()


@pytest.mark.parametrize("form", ["bgzf", "bam_seq"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_binary_sam_deflate_dynamic(kslam, tmp_path, tag, form):
    """SLAM --sam-deflate dynamic on the reference loop's cases: the file inflates to what the fixed-mode file (which the
    existing tests pin to the reference loop's own SAM file) inflates to, is smaller, is the same from the host formatter and
    from one or three lanes, and leaves the other output files alone"""
    import ref_loop_case as R
    Dm = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case(tag)
    R.write_case(case, tmp_path, Dm)
    tail = ["--num-reads-at-once", str(int(z[tag + "_per_batch"]))] + ([] if bool(z[tag + "_pseudo"]) else ["--no-pseudo-assembly"])
    flags = ["--sam-bgzf"] if form == "bgzf" else ["--sam-bam", "--sam-seq"]
    fixed = ["--db=db", "--sam-file", "f.out", "--output-file=f"] + flags + tail + ["R1.fq", "R2.fq"]
    args = ["--db=db", "--sam-file", "d.out", "--output-file=d"] + flags + ["--sam-deflate", "dynamic"] + tail + ["R1.fq", "R2.fq"]
    _run(fixed, tmp_path)
    _run(args, tmp_path)
    f_blob, blob = (tmp_path / "f.out").read_bytes(), (tmp_path / "d.out").read_bytes()
    assert blob.endswith(Z_EOF) and len(blob) < len(f_blob)
    text, reps = I.inflate(blob)
    assert any(r.types == [2] for r in reps) and all(len(r.types) == 1 for r in reps)
    assert gzip.decompress(blob) == text
    if form == "bgzf":
        assert text.replace(_cl(args), b"CL") == B.check(f_blob).replace(_cl(fixed), b"CL")
    else:
        import samseq_check as S
        (head, body), (f_head, f_body) = S.decode(text), S.decode(B.check(f_blob))
        assert head.replace(_cl(args), b"CL") == f_head.replace(_cl(fixed), b"CL") and body == f_body
    for suffix in ("", "_abbreviated", "_PerRead"):
        assert (tmp_path / ("d" + suffix)).read_bytes() == (tmp_path / ("f" + suffix)).read_bytes(), suffix
    for env in ({"KSLAM_HOST_SAM_TEXT": "1"}, {"KSLAM_LANES": "1"}, {"KSLAM_LANES": "3"}):
        _run_env(args, tmp_path, env)
        assert (tmp_path / "d.out").read_bytes() == blob, env


Z_EOF = B.EOF_MARKER


def test_binary_refuses_sam_deflate_without_a_compressed_mode(kslam, tmp_path):
    for extra in (["--sam-deflate", "dynamic"], ["--sam-deflate", "fixed"], ["--sam-bgzf", "--sam-deflate", "best"]):
        r = subprocess.run([SLAM, "--db", "db", "--sam-file", "o.sam"] + extra + ["R1.fq"], cwd=str(tmp_path), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and b"sam-deflate" in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.sam").exists()
