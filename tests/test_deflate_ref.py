"""tests/deflate_ref.py, the restatement of csrc/bgzf.hip that the GPU tests compare bytes with, pinned on the CPU: what
it writes, zlib, gzip and tests/inflate_ref.py read back; its fixed mode is strict BGZF as tests/bgzf_check.py defines it;
its code builder gives complete, limited, monotone and -- where plain Huffman fits -- optimal codes; and the cases hold
the seams they are named for."""
import gzip
import heapq
import zlib
from fractions import Fraction

import pytest

import bgzf_check as B
import deflate_cases as C
import deflate_ref as D
import inflate_ref as I


@pytest.mark.parametrize("mode", [D.FIXED, D.DYNAMIC])
@pytest.mark.parametrize("name", sorted(C.INPUTS))
def test_every_reader_returns_the_input(name, mode):
    x, ms = C.data(name), C.expected(name, mode)
    assert len(ms) == (len(x) + C.M - 1) // C.M
    blob = b"".join(m for m, _ in ms)
    assert b"".join(zlib.decompress(m[18:-8], -15) for m, _ in ms) == x
    assert gzip.decompress(blob + B.EOF_MARKER) == x
    text, reps = I.inflate(blob)
    assert text == x
    for (m, rep), seen in zip(ms, reps):
        assert seen.types == [rep.btype]
        assert rep.btype == 2 or mode == D.FIXED or rep.dynamic_bytes >= rep.fixed_bytes or rep.stored_bytes < rep.dynamic_bytes
        assert len(m) == 26 + {0: rep.stored_bytes, 1: rep.fixed_bytes, 2: rep.dynamic_bytes}[rep.btype]
        assert len(m) - 26 == min(rep.stored_bytes, rep.fixed_bytes, rep.dynamic_bytes if mode == D.DYNAMIC else rep.fixed_bytes)
        if rep.btype == 2:
            assert (seen.max_ll_len, seen.max_d_len, seen.repeat_crossed) == (rep.max_ll_len, rep.max_d_len, rep.repeat_crossed)
    if mode == D.FIXED:
        assert B.check(blob + B.EOF_MARKER) == x
        assert D.compress(x) == blob


def test_the_cases_hold_their_seams():
    dyn = {name: C.expected(name, D.DYNAMIC) for name in C.INPUTS}
    assert dyn["empty"] == []
    # the first tile can have no match; the second can
    assert all(dyn[n][0][1].n_matches == 0 for n in ("one_byte", "text_255", "text_256", "random_3000", "ff_200"))
    assert dyn["text_3_members_17"][0][1].n_matches > 1000
    # no match: two forced distance lengths of 1, HDIST = 2
    for n in ("random_3000", "text_255"):
        rep = dyn[n][0][1]
        assert (rep.hdist, rep.max_d_len, rep.hlit) == (2, 1, 257)
    assert dyn["random_3000"][0][1].btype == 0 and dyn["text_255"][0][1].btype == 2
    assert [r.btype for _, r in dyn["random_200000"]] == [0, 0, 0, 0]
    assert sum(len(m) for m, _ in dyn["random_200000"]) == 200000 + 4 * 31
    # where the fixed code wins: the header costs more than it saves
    assert [r.btype for _, r in dyn["all_bytes_x3"]] == [1] and [r.btype for _, r in dyn["one_byte"]] == [1]
    # a 16, a 17 and an 18 in one header
    assert {16, 17, 18} <= set(dyn["text_member"][0][1].cl_symbols) and dyn["text_member"][0][1].btype == 2
    # a repeat from the literal/length lengths into the distance lengths, in a member that is written dynamic
    rep = dyn["ff_200"][0][1]
    assert rep.btype == 2 and rep.repeat_crossed
    assert I.inflate(dyn["ff_200"][0][0])[1][0].repeat_crossed
    # the window edge: distance 32 768 is used, 32 769 is not
    assert max(r.max_distance for r in I.inflate(b"".join(m for m, _ in dyn["pattern_32768"]))[1]) == 32768
    far = b"".join(m for m, _ in dyn["pattern_32769"])
    assert max(r.max_distance for r in I.inflate(far)[1]) < 32768 and len(far) > 0.99 * len(C.data("pattern_32769"))
    # dynamic never loses, and wins on the text
    for name in C.INPUTS:
        for (m, _), (f, _) in zip(dyn[name], C.expected(name, D.FIXED)):
            assert len(m) <= len(f)
    for tag in "ab":
        x = C.golden_text(tag)[:C.M]
        assert len(D.compress(x, D.DYNAMIC)) < len(D.compress(x, D.FIXED))


def _huffman_cost(counts):
    h = [c for c in counts if c]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def _huffman_depth(counts):
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))   # on equal weight the shallower first: the least deepest leaf
    return h[0][1] if h else 0


@pytest.mark.parametrize("name", sorted(C.HISTOGRAMS))
def test_code_lengths(name):
    counts, limit = C.HISTOGRAMS[name]
    lens = D.code_lengths(counts, limit)
    assert len(lens) == len(counts)
    assert sum(Fraction(1, 1 << l) for l in lens if l) == 1, "the Kraft sum is exactly 1"
    assert max(lens) <= limit
    used = [s for s, c in enumerate(counts) if c]
    assert all(lens[s] for s in used)
    if len(used) >= 2:
        assert all(lens[s] == 0 for s in range(len(counts)) if not counts[s])
    else:   # the lowest-numbered unused symbols fill up to two, each code one bit
        forced = [s for s in range(len(counts)) if not counts[s]][:2 - len(used)]
        assert sorted(s for s, l in enumerate(lens) if l) == sorted(used + forced) and max(lens) == 1
    for a in used:
        for b in used:
            assert not (counts[a] > counts[b] and lens[a] > lens[b]), "a higher count has a longer code"
    if len(used) >= 2 and _huffman_depth(counts) <= limit:
        assert sum(counts[s] * lens[s] for s in used) == _huffman_cost(counts)
    codes = D.canonical_codes(lens)
    words = sorted(format(codes[s], "0%db" % lens[s])[::-1] for s in range(len(lens)) if lens[s])
    assert all(not b.startswith(a) for a, b in zip(words, words[1:])), "prefix-free"


def test_the_histograms_sit_on_both_sides_of_the_limit():
    deep = {n: _huffman_depth(C.HISTOGRAMS[n][0]) for n in C.HISTOGRAMS}
    assert (deep["fib_8"], deep["fib_16"], deep["fib_17"], deep["fib_22"], deep["fib_30"]) == (7, 15, 16, 21, 29)
    assert (deep["cl_fib_6"], deep["cl_fib_7"], deep["cl_fib_8"], deep["cl_fib_9"], deep["cl_fib_19"]) == (5, 6, 7, 8, 18)
    assert max(D.code_lengths(*C.HISTOGRAMS["fib_16"])) == 15 == max(D.code_lengths(*C.HISTOGRAMS["fib_17"]))
    assert deep["steep_286"] > 15 and deep["ties_286"] <= 15 and deep["equal_286"] == 9
