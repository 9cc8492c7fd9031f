"""include/kslam_gunzip.h without a GPU: the yardstick itself.  tests/gunzip_ref.py's serial walk gives gzip.decompress's text
on every case of tests/gunzip_cases.py, every case holds the seam it is named for -- proven from the restatement's report,
not assumed -- and every refusal is refused by Python's gzip too and named by the restatement as the cases say."""
import gzip
import zlib

import pytest

import gunzip_cases as Gc
import gunzip_ref as G
import inflate_ref as R

KIB = 1024


@pytest.fixture(scope="module")
def valid():
    return Gc.valid_cases()


@pytest.fixture(scope="module")
def walks(valid):
    """blob -> Walk and Finder, computed once per distinct file"""
    out = {}
    for blob, _, _ in valid.values():
        if blob not in out:
            out[blob] = (G.walk(blob), G.Finder(blob))
    return out


@pytest.fixture(scope="module")
def plans(valid, walks):
    return {name: G.plan(blob, chunk, *walks[blob]) for name, (blob, _, chunk) in valid.items()}


def test_every_case_is_what_gzip_makes_of_it(valid, walks):
    assert len(valid) == 16 + 18
    for name, (blob, text, chunk) in valid.items():
        assert gzip.decompress(blob) == text, name
        assert bytes(walks[blob][0].text) == text, name
        assert chunk % 4 == 0 and chunk >= 1024
    assert G.plan(b"", 1024).stats["chunks"] == 0 and gzip.decompress(b"") == b""


def test_levels_have_a_live_start_in_every_chunk_that_can_have_one(valid, walks, plans):
    """Blocks of this text lie 25 to 30 KB of compressed bytes apart, so every 32 KiB chunk holds a block header.  The
    LAST block is final (BFINAL = 1) and therefore never a start: the chunks from the one with its header on have none."""
    for level in (1, 6, 9):
        name = "level%d" % level
        blob, text, chunk = valid[name]
        w, pl = walks[blob][0], plans[name]
        assert chunk == 32 * KIB and len(text) == 1500000 and {b[3] for b in w.blocks} == {2}
        gaps = [b[0] - a[0] for a, b in zip(w.blocks, w.blocks[1:])]
        assert max(gaps) < 8 * 31 * KIB
        last_chunk = w.blocks[-1][0] // (8 * chunk)
        assert last_chunk >= pl.stats["chunks"] - 2
        assert sorted(pl.found) == list(range(1, last_chunk)), name
        assert pl.stats["starts_dropped"] == 0 and pl.stats["starts_live"] == last_chunk - 1
    # the same file in chunks of 4 KiB and 1 KiB: most chunks have no start and belong to their predecessor
    for name, chunk in (("level6_chunk4k", 4 * KIB), ("level6_chunk1k", KIB)):
        pl = plans[name]
        assert valid[name][0] == valid["level6"][0] and valid[name][2] == chunk
        assert pl.stats["starts_live"] == len(walks[valid[name][0]][0].blocks) - 2 and pl.stats["starts_dropped"] == 0
        assert pl.stats["chunks"] > 8 * pl.stats["starts_found"]
    assert plans["shorter_than_a_chunk"].stats["chunks"] == 1 and plans["shorter_than_a_chunk"].stats["starts_found"] == 0


def test_the_false_start_is_found_and_dropped(valid, walks, plans):
    blob, text, chunk = valid["false_start"]
    w, pl = walks[blob][0], plans["false_start"]
    assert {b[3] for b in w.blocks} == {0} and len(w.blocks) == 2            # stored blocks only: no true start anywhere
    assert pl.found[1] == 8 * (16 * KIB + 7)                                 # the inner stream's first bit
    assert G.is_start(blob, pl.found[1]) and pl.found[1] not in {b[0] for b in w.blocks}
    assert pl.stats["starts_found"] >= 1 and pl.stats["starts_dropped"] == pl.stats["starts_found"] and pl.stats["starts_live"] == 0
    inner = zlib.decompressobj(-15)
    assert len(inner.decompress(text[16 * KIB + 7 - 15:])) == 300000 and inner.eof      # a real stream: the wave on it decodes for long


def test_far_sources_reach_one_two_and_three_stretches_back(valid, walks, plans):
    blob, text, chunk = valid["far_sources"]
    w, pl = walks[blob][0], plans["far_sources"]
    rep = G.symbols(w, pl)
    assert {1, 2, 3} <= rep.far_spans_back
    lengths = pl.span_lengths(len(text))
    assert min(lengths[1:-1]) < G.WINDOW < max(lengths[1:-1])               # a live stretch between two live starts shorter than the window
    assert rep.marker_copied and rep.rle_over_markers
    assert pl.stats["starts_live"] >= 8 and pl.stats["starts_dropped"] == 0
    assert max(m[1] for m in w.matches) < 32768                             # zlib stops short of the full window; the edge cases reach it


def test_hand_built_edges(valid, walks, plans):
    for name, before in (("edge_32768", 0), ("edge_32768_second_member", 7000)):
        blob, text, chunk = valid[name]
        w, pl = walks[blob][0], plans[name]
        rep = G.symbols(w, pl)
        assert len(pl.spans) == 2 and pl.spans[1][1] == before + 32768, name     # the match's block is a live start ...
        assert rep.first_tokens[1] == (32768, 258)                               # ... and the match its first token
        assert w.members[-1][1] == before                                        # exactly 32 768 bytes of its member before it
        assert pl.stats["starts_live"] == 1 and pl.stats["starts_dropped"] == 0


def test_member_cases(valid, walks, plans):
    n = {"two_members": 2, "five_members": 5, "empty_member_between": 4, "header_fields": 2, "zero_padding": 2}
    for name, members in n.items():
        assert plans[name].stats["members"] == members, name
    w = walks[valid["empty_member_between"][0]][0]
    assert [m[2] - m[1] for m in w.members][1::2] == [0, 0]
    blob = valid["header_fields"][0]
    assert blob[3] == 4 | 8 | 16 | 2 and G.header(blob) == 10 + 2 + 42 + 15 + 7 + 2
    blob = valid["zero_padding"][0]
    assert blob.endswith(bytes(700)) and walks[blob][0].members[-1][3] + 8 == len(blob) - 700
    blob, text, chunk = valid["bgzf"]
    assert R.inflate(blob)[0] == text and plans["bgzf"].stats["members"] == len(R.members(blob)) == 4
    # the seam at a multiple of 4 KiB falls on each of the 8 trailer bytes and the 10 header bytes of the second member
    seen = set()
    for j in range(18):
        blob, text, chunk = valid["straddle_%02d" % j]
        w = walks[blob][0]
        trailer, second = w.members[0][3], w.members[1][0]
        assert second == trailer + 8 and G.header(blob, second) == second + 10
        seam = (trailer + chunk - 1) // chunk * chunk if j else trailer
        assert seam % chunk == 0 and trailer <= seam < second + 10
        seen.add(seam - trailer)
    assert seen == set(range(18))


def test_refusals_are_gzips_too_and_named_by_the_restatement():
    bad = Gc.refusals()
    assert len(bad) == 11
    for name, (blob, chunk, member, kind) in bad.items():
        with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
            if name == "reserved_flag":      # the one point where the library is stricter than Python (RFC 1952: must be zero)
                raise gzip.BadGzipFile(name)
            gzip.decompress(blob)
        with pytest.raises(G.GunzipError) as e:
            G.walk(blob)
        assert e.value.member == member, name
        if kind is not None:
            assert e.value.kind == kind, name
        else:
            assert e.value.kind in R.KINDS, name
    assert G.walk(bad["garbage_behind_a_member"][0][:-7]).members[-1][3] + 8 == len(bad["garbage_behind_a_member"][0]) - 7
