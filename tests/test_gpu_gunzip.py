"""include/kslam_gunzip.h on the GPU: kslam_gunzip_inflate on every case of tests/gunzip_cases.py -- text equal to the original,
the figures of kslam_gunzip_last_stats equal to the restatement's (tests/gunzip_ref.py) -- in rounds of several sizes, on every
refusal, on 16 MiB of FASTQ-like text, and the executable reading plain gzip with --gunzip."""
import gzip
import importlib

import pytest

import gunzip_cases as Gc
import gunzip_ref as G
import inflate_cases as Cs
from test_cli import SLAM, _fixture_case, _run

pytestmark = pytest.mark.gpu
KIB = 1024
FIGURES = ("members", "chunks", "starts_found", "starts_live", "starts_dropped", "text_len")


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def Z(kslam):
    return importlib.import_module("kslam_amd.gunzip")


@pytest.fixture(scope="module")
def valid():
    return Gc.valid_cases()


@pytest.fixture(scope="module")
def restated(valid):
    """name -> the figures the restatement gives; every distinct file is walked once"""
    seen, out = {}, {}
    for name, (blob, _, chunk) in valid.items():
        if blob not in seen:
            seen[blob] = (G.walk(blob), G.Finder(blob))
        out[name] = G.plan(blob, chunk, *seen[blob]).stats
    return out


def _figures(Z, ctx):
    s = Z.stats(ctx)
    return {k: s[k] for k in FIGURES}


def test_every_valid_case_text_and_figures(Z, ctx, valid, restated):
    Z.set_round(ctx, 0)
    wrong = []
    for name, (blob, text, chunk) in valid.items():
        Z.set_chunk(ctx, chunk)
        got = Z.inflate(ctx, blob)
        if got != text or _figures(Z, ctx) != restated[name]:
            wrong.append((name, len(got), _figures(Z, ctx), restated[name]))
    Z.set_chunk(ctx, 0)
    assert not wrong, wrong
    assert Z.inflate(ctx, b"") == b"" and Z.stats(ctx)["chunks"] == 0


def test_bgzf_through_this_path_equals_the_bgzf_path(kslam, Z, ctx, valid):
    I = importlib.import_module("kslam_amd.inflate")
    blob, text, chunk = valid["bgzf"]
    Z.set_chunk(ctx, chunk)
    assert Z.inflate(ctx, blob) == I.inflate(ctx, blob) == text
    Z.set_chunk(ctx, 0)


@pytest.mark.parametrize("name", ["level6", "far_sources"])
def test_rounds_of_every_size_give_the_same(Z, ctx, valid, restated, name):
    """one chunk's worth of symbols (every stretch a round of its own: the window is carried across each seam), three, the default"""
    blob, text, chunk = valid[name]
    Z.set_chunk(ctx, chunk)
    rounds = []
    for symbols in (chunk, 3 * chunk, 0):
        Z.set_round(ctx, symbols)
        assert Z.inflate(ctx, blob) == text, symbols
        assert _figures(Z, ctx) == restated[name], symbols
        rounds.append(Z.stats(ctx)["rounds"])
    Z.set_chunk(ctx, 0)
    assert rounds[0] == restated[name]["starts_live"] + 1 and rounds[0] >= rounds[1] > rounds[2] == 1
    with pytest.raises(Exception):
        Z.set_round(ctx, KIB)          # less than one chunk's worth
    with pytest.raises(Exception):
        Z.set_chunk(ctx, 1022)


def test_refusals_are_named_and_the_context_goes_on(kslam, Z, ctx, valid):
    Z.set_round(ctx, 0)
    for name, (blob, chunk, member, kind) in Gc.refusals().items():
        if kind is None:
            with pytest.raises(G.GunzipError) as r:
                G.walk(blob)
            kind = r.value.kind
        Z.set_chunk(ctx, chunk)
        with pytest.raises(kslam.KslamError) as e:
            Z.inflate(ctx, blob)
        assert e.value.status == 1 and "member %d " % member in str(e.value) and str(e.value).endswith(": " + kind), (name, str(e.value))
    blob, text, chunk = valid["two_members"]
    Z.set_chunk(ctx, chunk)
    assert Z.inflate(ctx, blob) == text
    Z.set_chunk(ctx, 0)


def test_sixteen_mebibytes_of_fastq_at_level_6(Z, ctx):
    text = Gc.fastq_like(16 << 20, seed=8)
    blob = Gc.gz(text)
    Z.set_chunk(ctx, 64 * KIB)
    Z.set_round(ctx, 0)
    got = Z.inflate(ctx, blob)
    s = Z.stats(ctx)
    Z.set_chunk(ctx, 0)
    print({k: (round(v, 3) if isinstance(v, float) else v) for k, v in s.items()})
    assert got == text
    assert s["starts_dropped"] == 0 and s["starts_live"] >= 0.9 * (s["chunks"] - 1) and s["members"] == 1


# ---- the executable ----
def _four_files(d, out, sam, args):
    """the three report files and the SAM file, the command line in its header aside"""
    files = [(d / (out + s)).read_bytes() for s in ("", "_abbreviated", "_PerRead")]
    return files + [(d / sam).read_bytes().replace((SLAM + " " + " ".join(args)).encode(), b"CL")]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_binary_reads_plain_gzip_with_the_switch(kslam, tmp_path, tag):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case(tag)
    R.write_case(case, tmp_path, D)
    for r in ("R1", "R2"):
        text = (tmp_path / (r + ".fq")).read_bytes()
        (tmp_path / (r + ".plain.gz")).write_bytes(gzip.compress(text[:len(text) // 2]) + gzip.compress(text[len(text) // 2:], 9))   # cat a.gz b.gz
        (tmp_path / (r + ".bgzf.gz")).write_bytes(Cs.bgzf(text) + Cs.EOF_MARKER)
    tail = ["--num-reads-at-once", str(int(z[tag + "_per_batch"]))] + ([] if bool(z[tag + "_pseudo"]) else ["--no-pseudo-assembly"])
    plain = ["--db=db", "--sam-file", "p.sam", "--output-file=p"] + tail + ["R1.fq", "R2.fq"]
    _run(plain, tmp_path)
    exp = _four_files(tmp_path, "p", "p.sam", plain)
    for k, (r1, r2) in enumerate((("R1.plain.gz", "R2.bgzf.gz"), ("R1.fq", "R2.plain.gz"))):
        out = "o%d" % k
        args = ["--gunzip", "--db=db", "--sam-file", out + ".sam", "--output-file=" + out] + tail + [r1, r2]
        _run(args, tmp_path)
        assert _four_files(tmp_path, out, out + ".sam", args) == exp, (r1, r2)
        r = _run(args[1:], tmp_path, check=False)            # without the switch: refused as before
        assert r.returncode != 0 and b"plain gzip" in r.stderr and b"bgzip" in r.stderr and (r1 if "plain" in r1 else r2).encode() in r.stderr
