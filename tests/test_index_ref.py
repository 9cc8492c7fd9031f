"""tests/index_ref.py held to the oracle and to values written out by hand, and tests/index_seams.py held to its seams (CPU).

The restatement of the index build is what tests/test_gpu_index_build.py demands of the device bit for bit, so it is
checked here three ways: against the oracle's getKMers + sortKMers on every index of index_seams, against records, buckets
and base codes worked out by hand, and -- so that no family silently misses the seam it was built for -- against the list
of preconditions below.  A count the inputs do not reach is mended in index_seams, not here.
"""
import numpy as np
import pytest

import filter_ref as F
import index_ref as R
import index_seams as S
import sort_ref as SR

G, RC = R.FROM_GENBANK, R.REVCOMP


def _rows(recs):
    return [(int(r["kmer"]), int(r["meta"]), int(r["offset"])) for r in recs]


# ---- against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_records_and_order_equal_the_oracle(oracle, name):
    entries = list(S.index(name))
    got = R.records(entries)
    exp = oracle.extract_kmers(entries, True, R.GAP)
    assert len(got) == len(exp) == int(R.kmers_per_entry(entries).sum())
    for f in ("kmer", "meta", "offset"):                       # extraction order and every field
        bad = np.flatnonzero(got[f] != exp[f])
        assert len(bad) == 0, (name, f, bad[:5], got[bad[:5]], exp[bad[:5]])
    mine, theirs = S.sorted_records(name), oracle.sort_kmers(exp)
    # sortKMers orders by (kmer ascending, meta descending) and no further: those two columns must agree as they stand ...
    assert np.array_equal(mine["kmer"], theirs["kmer"]) and np.array_equal(mine["meta"], theirs["meta"]), name
    # ... and within a tie of both the offsets agree as a multiset (the restatement's are in extraction order, ascending)
    def canon(s):
        return s[np.lexsort((s["offset"], ~s["meta"], s["kmer"]))]
    assert canon(mine).tobytes() == canon(theirs).tobytes(), name
    same = (mine["kmer"][1:] == mine["kmer"][:-1]) & (mine["meta"][1:] == mine["meta"][:-1])
    assert (mine["offset"][1:][same] > mine["offset"][:-1][same]).all(), name


def test_reverse_complement_agrees_with_the_filter_restatement():
    rng = np.random.default_rng(5)
    ws = [S.rand(rng, R.K) for _ in range(200)]
    fwd = R.records(ws)
    back = R.records([S.revcomp(w) for w in ws])
    assert np.array_equal(fwd["kmer"], back["kmer"])                                   # either strand, one canonical k-mer
    assert ((fwd["meta"] ^ back["meta"]) == RC).all()                                  # (no palindrome among them)
    assert np.array_equal(F.revcomp64(F.revcomp64(fwd["kmer"])), fwd["kmer"])
    assert (fwd["kmer"] <= F.revcomp64(fwd["kmer"])).all()


# ---- by hand -----------------------------------------------------------------------------------------------------------------
HAND = [b"C" * 32, b"G" * 32, b"A" * 48, S.LAST_BUCKET_PALINDROME, b"T" * 33, b"ACGT" * 8, b"c" * 40, b"ACGT" * 7 + b"ACG"]
C32, GC, ACGT = 0x5555555555555555, 0xFFFFFFFF55555555, 0x1E1E1E1E1E1E1E1E


def test_records_by_hand():
    assert _rows(R.records(HAND)) == [
        (C32, G | 0, 0),                      # C*32 < its reverse complement G*32: forward
        (C32, G | RC | 1, 0),                 # G*32: the other strand of the same k-mer
        (0, G | 2, 0), (0, G | 2, 16),        # poly-A: k-mer 0, forward, every 16th offset; 48 bases hold two
        (GC, G | RC | 3, 0),                  # G*16 + C*16 is its own reverse complement: the rc branch, bit 30 set
        (0, G | RC | 4, 0),                   # poly-T: k-mer 0 on the other strand; 33 bases hold one k-mer
        (ACGT, G | RC | 5, 0),                # (ACGT)*8, a palindrome again: A 0, C 1, G 3, T 2 -> 0x1E per four bases
        (0, G | 6, 0),                        # lower case is code 0: k-mer 0, forward; 40 bases hold one k-mer
    ]                                         # and 31 bases hold none


def test_order_and_buckets_by_hand():
    b = R.build(HAND)
    assert _rows(b["records"]) == [
        (0, G | RC | 4, 0), (0, G | 6, 0), (0, G | 2, 0), (0, G | 2, 16),        # meta descending; equal metas keep their order
        (ACGT, G | RC | 5, 0), (C32, G | RC | 1, 0), (C32, G | 0, 0), (GC, G | RC | 3, 0)]
    assert (b["bucket_bits"], b["filter_bits"], b["n_genome_kmers"], b["n_entries"], b["n_bases"]) == (8, 20, 8, 8, 280)
    t = b["bucket"]
    assert len(t) == 257 and t[0] == 0 and (t[1:0x1F] == 4).all() and (t[0x1F:0x56] == 5).all() and (t[0x56:0x100] == 7).all()
    assert t[256] == 8
    assert np.array_equal(b["offsets"], [0, 32, 64, 112, 144, 177, 209, 249, 280])
    assert len(b["filter"]) == (1 << 20) // 32
    assert F.is_member(b["filter"], np.array([ACGT, C32, GC], dtype=np.uint64), 20).all()
    assert int(sum(bin(int(w)).count("1") for w in b["filter"][b["filter"] != 0])) <= 12      # three keys, four bits each: k-mer 0 is not in it


def test_bucket_and_filter_sizes_by_hand():
    assert [R.bucket_bits(m) for m in (0, 1023, 1024, 2047, 2048, 1 << 20, 1 << 40)] == [8, 8, 9, 9, 10, 19, 27]
    assert R.bucket_bits(5, exact=20) == 20 and R.bucket_bits(5, exact=3) == 8 and R.bucket_bits(5, exact=40) == 28
    assert [R.filter_bits(m) for m in (0, 87381, 87382)] == [20, 20, 21]
    assert [R.filter_bits(100, env) for env in (0, -1, 5, 20, 21, 28, 99)] == [0, 0, 20, 20, 21, 28, 36]


def test_base_codes_by_hand():
    got = R.base_codes([b"ACGTU", b"acgtu", b"Nn-@[R"])
    assert got.tolist() == [8, 9, 10, 11, 0, 0, 1, 2, 3, 0, 4, 4, 4, 4, 4, 4]
    # the kernels undo it as 3 - code where bit 3 is set (stage.h: codes_of_dword): A <-> T, C <-> G, nothing else moves
    comp = np.where(got & 8, 3 - (got & 7), got & 7)
    assert comp.tolist() == [3, 2, 1, 0, 0, 0, 1, 2, 3, 0, 4, 4, 4, 4, 4, 4]


def test_first_difference_names_the_table():
    a = R.build(HAND)
    assert R.first_difference(a, a) is None
    b = dict(a, bucket=a["bucket"].copy())
    b["bucket"][200] += 1
    assert R.first_difference(b, a)[:4] == ("bucket", 200, 8, 7)
    assert R.first_difference(dict(a, filter_bits=21), a)[0] == "filter_bits"
    assert R.first_difference(dict(a, keys=a["keys"][:-1]), a)[:2] == ("keys", "length")


# ---- the preconditions of tests/test_gpu_index_build.py ------------------------------------------------------------------------
def test_lengths_and_start_residues():
    entries = S.index("lengths")
    lens = [len(e) for e in entries]
    assert set(S.NAMED_LENGTHS) <= set(lens)
    assert R.kmers_per_entry([b"A" * 2064])[0] == 128 and R.kmers_per_entry([b"A" * 2080])[0] == 129
    assert S.n_segments([b"A" * S.NAMED_LENGTHS[-2]]) == 64 and S.n_segments([b"A" * S.NAMED_LENGTHS[-1]]) == 65
    off = R.offsets(entries)[:-1].astype(np.int64)
    lens = np.array(lens)
    assert set((off % 4).tolist()) == {0, 1, 2, 3} and set((off % 16).tolist()) == set(range(16))
    assert set((off[lens >= R.K] % 16).tolist()) == set(range(16))             # ... of entries that have k-mers
    assert set((off[lens >= 2064] % 4).tolist()) == {0, 1, 2, 3}               # ... of entries of more than one segment
    assert sum(lens) < 400_000


def test_record_counts():
    for m in S.M_VALUES:
        assert len(S.sorted_records("m/%d" % m)) == m
    assert SR.SORT_TILE == 4096


@pytest.mark.parametrize("n", S.ID_COUNTS)
def test_id_groups_differ_in_every_meta_pass(n):
    entries = S.index("ids/%d" % n)
    assert len(entries) == n
    if n > 257:
        assert all(48 <= len(e) <= 64 for i, e in enumerate(entries) if i not in S.PLANT_AT)
    s = S.sorted_records("ids/%d" % n)
    meta_passes = SR.index_passes(n)[:-8]
    assert len(meta_passes) == {1: 1, 128: 1, 129: 2, 257: 2, 32768: 2, 32769: 3}[n]
    ident = s["meta"] & np.uint32(0x3FFFFFFF)
    w = np.ascontiguousarray(s).view(np.uint32).reshape(-1, 4)
    if n >= 129:
        for p in meta_passes:
            assert R.groups_differing(s, SR.digit(w, p)) >= 10, (n, p)
            id_field = (ident >> np.uint32(p[1])) & np.uint32(0xFF if p[4] == 0 else 0x7F)
            if (int(ident.max()) >> p[1]) != 0:                  # the pass holds id bits that are in use: those differ too
                assert R.groups_differing(s, id_field) >= 10, (n, p)
    only_revcomp = R.groups_differing(s, s["meta"]) - R.groups_differing(s, ident)
    assert only_revcomp >= 10, (n, only_revcomp)
    planted = [e for e in S.PLANT_AT if e < n]
    lo, hi = R.key_groups(s)
    full = sum(1 for a, b in zip(lo, hi) if set(planted) <= set(ident[a:b].tolist()))
    assert full >= S.N_PLANTED                                   # the same 32-mers in every planted entry
    both = sum(1 for a, b in zip(lo, hi) if len(planted) > 1 and set(planted) <= set(ident[a:b].tolist())
               and len(set((s["meta"][a:b] & np.uint32(RC)).tolist())) == 2)
    assert both >= S.N_PLANTED or len(planted) == 1              # ... on both strands


def test_ratio_switches():
    for k, on in ((63, False), (64, True)):
        e = S.index("uniform/%d" % k)
        nk = R.kmers_per_entry(e)
        assert (nk == k).all()
        assert (int(nk.sum()) // len(e) >= 64) == on              # api_index.hip: meta_digits_in_runs = n && m / n >= 64
        # equal keys in different entries, on both strands: otherwise no table shows what the meta pass did
        s = S.sorted_records("uniform/%d" % k)
        (meta_pass,) = SR.index_passes(len(e))[:-8]
        assert R.groups_differing(s, SR.digit(np.ascontiguousarray(s).view(np.uint32).reshape(-1, 4), meta_pass)) >= 10
        assert R.groups_differing(s, s["meta"] & np.uint32(0x3FFFFFFF)) >= 10 and R.groups_differing(s, s["meta"] & np.uint32(RC)) >= 10
    a, b = S.index("segments/4n"), S.index("segments/4n+1")
    assert S.n_segments(a) == 4 * len(a) and S.n_segments(b) == 4 * len(b) + 1        # extract.hip: n_segs <= 4 * n_seqs
    for n in (1, 129, 257):                                      # the id seams with the run histogram on, 32 768 with it off
        assert len(S.sorted_records("ids/%d" % n)) // n >= 64
    assert len(S.sorted_records("ids/32769")) // 32769 < 64


def test_content():
    s = S.sorted_records("content")
    zero = s[s["kmer"] == 0]
    assert (zero["meta"] & np.uint32(RC) != 0).sum() > 20 and (zero["meta"] & np.uint32(RC) == 0).sum() > 20    # k-mer 0, both strands
    run, ascending = R.longest_equal_record_run(s)
    assert run > 4096 and ascending
    t = R.build(list(S.index("content")), bucket_exact=8, sorted_recs=s)["bucket"]
    assert t[1] > t[0] and t[256] > t[255]                        # bucket 0 and the last bucket hold keys
    assert (s["kmer"] == GC).any() and GC >> 56 == 0xFF
    rc = F.revcomp64(s["kmer"])
    assert ((rc == s["kmer"]) & (s["kmer"] != 0)).sum() >= 20     # palindromes ...
    assert (s["meta"][rc == s["kmer"]] & np.uint32(RC) != 0).all()      # ... all on the rc branch
    e = S.index("content")
    assert e[1] == e[5]                                           # an entry present twice
    junk = e[3]
    # N and lower case on both sides of a k-mer boundary
    assert any(junk[16 * i - 1:16 * i + 1] == b"NN" for i in range(1, 70)) and any(junk[16 * i - 1:16 * i + 1].islower() for i in range(1, 70))


def test_empty_bucket_runs_and_filter_blocks():
    big = "bucket_bits/%d" % S.BIG_BUCKET_BITS
    seen = 0
    for name in S.NAMES:
        if big not in S.routes_of(name):
            continue
        s = S.sorted_records(name)
        assert len(s) <= 1 << 15                                  # the setting is well above log2 m
        if len(s):
            assert R.longest_empty_bucket_run(S.expected(name, big)["bucket"]) > 256, name
            seen += 1
    assert seen >= 5
    blocks = {name: R.filter_block_words(S.sorted_records(name)["kmer"], 20) for name in S.NAMES if "filter_bits/20" in S.routes_of(name)}
    assert all(len(b) == 4 for b in blocks.values())
    assert (blocks["sparse"] == 0).any() and (blocks["sparse"] > 0).any()         # a block that receives no word, next to one that does
    assert sum(1 for b in blocks.values() if (b > 256).all()) >= 5                # blocks of more than 256 words (a workgroup's stride)
    assert (R.filter_block_words(S.sorted_records("content")["kmer"], 28) == 0).sum() > 256


def test_empty_and_filter_resize():
    assert len(S.index("empty/no_entries")) == 0
    assert len(S.index("empty/short_only")) > 0 and len(S.sorted_records("empty/short_only")) == 0
    b = S.expected("empty/short_only", "default")
    assert not b["bucket"].any() and not b["filter"].any() and len(b["filter"]) == 1 << 15
    assert S.expected("ids/32769", "default")["filter_bits"] == 21 and S.expected("m/255", "default")["filter_bits"] == 20
    assert S.DEVICE_FIRST_OFFSET % 4 != 0


def test_every_route_runs_somewhere_and_reads_exist():
    used = {r for _n, r in S.CASES}
    assert used == set(S.ROUTES)
    for name in S.NAMES:
        reads = S.reads_of(name)
        assert 1 <= len(reads) <= 9 and all(len(r) >= R.K for r in reads)
