"""The host restatement tests/join_ref.py held to recorded truth, and every seam of tests/join_seams.py shown to be
where its case's name says (no GPU).

The restatement is what tests/test_gpu_join_seams.py compares the kernels of k-slam_amd/csrc/join.hip with, so it is
compared here with the reference's own recorded answers (tests/golden/join_vectors.npz) and with the oracle.  The seam
checks import the constants from join_seams.py, where each names the line of join.hip it mirrors: when such a constant
moves, the check fails here instead of the seam test quietly testing something else.
"""
import os

import numpy as np
import pytest

import join_ref as R
import join_seams as S
from join_cases import make_join_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _split(sorted_recs):
    """the reference's one sorted list -> (genome records, read records), each still ascending by k-mer"""
    gb = (sorted_recs["meta"] >> np.uint32(31)) == 1
    g, r = np.zeros(int(gb.sum()), dtype=R.KMER_DT), np.zeros(int((~gb).sum()), dtype=R.KMER_DT)
    for f in ("kmer", "meta", "offset"):
        g[f], r[f] = sorted_recs[f][gb], sorted_recs[f][~gb]
    return g, r


def _layout_for(g, read_len):
    n_reads, lmax = len(read_len), int(max(read_len.max(), 1)) if len(read_len) else 1
    n_entries = int((g["meta"] & np.uint32(R.ID_MASK)).max()) + 1 if len(g) else 1
    gmax = int(g["offset"].max()) if len(g) else 0
    return (max(1, (n_reads - 1).bit_length()), max(1, (n_entries - 1).bit_length()), (gmax + 2 * lmax).bit_length(), lmax)


def _as_tuples(keys, layout):
    return [R.unpack(k, layout) for k in keys.tolist()]


def _check_against(g, r, read_len, raw, deduped, ties):
    lay = _layout_for(g, read_len)
    keys = R.join(g, r, read_len, lay)
    got = sorted(_as_tuples(keys, lay))
    exp = sorted(zip(raw["read"].tolist(), raw["entry"].tolist(), raw["rel"].tolist(), raw["revcomp"].tolist()))
    assert got == exp
    _s, keep, rows = R.unique_rows(keys, lay, 0)
    assert len(rows) == len(deduped) and int(keep.sum()) == len(deduped)
    for f in ("read", "entry", "rel"):
        assert (rows[f] == deduped[f]).all(), f
    amb = np.array([(int(a), int(b), int(c)) in ties for a, b, c in zip(deduped["read"], deduped["entry"], deduped["rel"])], dtype=bool)
    assert ((rows["revcomp"] == deduped["revcomp"]) | amb).all()
    for f in ("score", "ref_begin", "ref_end", "query_begin", "query_end", "cigar_len", "cigar_off", "pad", "pad2"):
        assert not rows[f].any(), f
    return int(amb.sum())


def test_restatement_equals_the_recorded_reference():
    z = np.load(os.path.join(GOLD, "join_vectors.npz"))
    g, r = _split(z["sorted"])
    read_len = np.diff(z["reads_off"].astype(np.int64)).astype(np.uint32)
    ties = {tuple(int(v) for v in t) for t in z["ties"]}
    assert 0 < _check_against(g, r, read_len, z["raw"], z["deduped"], ties) < 10


def _oracle_sets():
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    unit = acgt[rng.integers(0, 4, 16)]
    g0 = np.concatenate([acgt[rng.integers(0, 4, 300)], np.tile(unit, 30), acgt[rng.integers(0, 4, 300)]]).tobytes()
    tandem = ([g0], [g0[250:400], g0[330:480], g0[300:460], g0[700:820], bytes(np.tile(unit, 9))])
    g1, g2 = (acgt[rng.integers(0, 4, 900)].tobytes() for _ in range(2))
    fwd = [g1[10:160], g2[300:420], g1[700:900]]
    revcomp = ([g1, g2], fwd + [s.translate(comp)[::-1] for s in fwd] + [g2[5:100].translate(comp)[::-1]])
    return {"tandem": tandem, "revcomp": revcomp}


@pytest.mark.parametrize("which", ["tandem", "revcomp", "join_case"])
def test_restatement_equals_the_oracle(oracle, which):
    genomes, reads = (make_join_case(3, n_reads=40)[::-1]) if which == "join_case" else _oracle_sets()[which]
    srt = oracle.sort_kmers(np.concatenate([oracle.extract_kmers(reads, False, 1), oracle.extract_kmers(genomes, True, 16)]))
    read_len = np.array([len(s) for s in reads], dtype=np.uint32)
    raw = oracle.scan_overlaps(srt, read_len)
    deduped, n_raw = oracle.find_overlaps(srt, read_len)
    assert n_raw == len(raw) and len(raw) > 50
    if which == "tandem":
        assert len(deduped) < len(raw)
    if which == "revcomp":
        assert set(raw["revcomp"].tolist()) == {0, 1}
    g, r = _split(srt)
    _check_against(g, r, read_len, raw, deduped, set())       # (the oracle orders revComp as this project does: no ties)


def test_bucket_table():
    keys = np.array([0, 1, 1 << 56, (1 << 56) + 5, 3 << 56, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    t = R.bucket_table(keys, 8)
    assert len(t) == 257 and t[0] == 0 and t[1] == 2 and t[2] == 4 and t[3] == 4 and t[4] == 5 and t[255] == 5 and t[256] == 6
    assert (R.bucket_table(np.zeros(0, dtype=np.uint64), 8) == 0).all()


def test_unique_is_against_the_last_kept():
    lay = (4, 4, 10, 100)
    keys = np.array(sorted(R.pack(1, 1, rel, 0, lay) for rel in (0, 2, 4, 5, 6, 9)), dtype=np.uint64)
    assert R.unique_flags(keys, lay).tolist() == [True, False, True, False, False, True]        # 0, 4 (not 2), 9
    assert not R.has_big_group(np.repeat(keys[:1], 64), lay) and R.has_big_group(np.repeat(keys[:1], 65), lay)


# ---- every named seam is present in its case --------------------------------------------------------------------------
JOIN = {c["name"]: c for c in S.join_cases() + S.merge_cases()}


def test_case_names_are_unique_and_sizes_small():
    assert len(JOIN) == len(S.join_cases()) + len(S.merge_cases())
    for c in JOIN.values():
        assert len(c["genome"]) <= 20000 and len(c["reads"]) <= 20000, c["name"]
        assert int(R.run_counts(c["genome"], c["reads"]).sum()) <= 2_000_000, c["name"]
        if len(c["genome"]) > 1:
            assert (c["genome"]["kmer"][1:] >= c["genome"]["kmer"][:-1]).all(), c["name"]
        gb = min(c["sorted_top_bits"], c["bucket_bits"])
        top = c["reads"]["kmer"] >> np.uint64(64 - gb)
        assert (top[1:] >= top[:-1]).all(), c["name"]


def test_record_count_seams():
    T = S.JOIN_TILE
    assert [len(JOIN["n_r=%d" % n]["reads"]) for n in (1, S.JB - 1, S.JB, S.JB + 1, T - 1, T, T + 1, 2 * T + 1)] == [1, 255, 256, 257, 1023, 1024, 1025, 2049]
    for n_g in (0, 1, 2):
        assert len(JOIN["n_g=%d" % n_g]["genome"]) == n_g
    assert R.run_counts(JOIN["no_hit"]["genome"], JOIN["no_hit"]["reads"]).sum() == 0
    assert R.run_counts(JOIN["n_r=2049"]["genome"], JOIN["n_r=2049"]["reads"]).sum() > 1000


def test_bucket_seams():
    seen_first, seen_last = set(), set()
    for c in S.bucket_cases():
        sizes = S.bucket_sizes(c)
        assert {S.SMALL_BUCKET, S.SMALL_BUCKET + 1, 8, 9}.issubset(set(sizes.tolist())), c["name"]
        assert set(c["want_sizes"]).issubset(set(sizes.tolist())), c["name"]
        assert (sizes[0], sizes[-1]) == c["first_last"], c["name"]
        seen_first.add(int(sizes[0]))
        seen_last.add(int(sizes[-1]))
        nz = np.flatnonzero(sizes)
        assert np.diff(nz).max() > len(sizes) // 4, c["name"]                 # a long stretch of empty buckets
        # per non-empty bucket: a read key below, above, on the first and on the last key
        table = R.bucket_table(c["genome"]["kmer"], c["bucket_bits"]).astype(np.int64)
        gk, rk = c["genome"]["kmer"], set(c["reads"]["kmer"].tolist())
        for b in nz.tolist():
            first, last = int(gk[table[b]]), int(gk[table[b + 1] - 1])
            assert {first - 1, first, last, last + 1}.issubset(rk), (c["name"], b)
            if first != last and sizes[b] > 1:
                assert first + 2 in rk, (c["name"], b)
            if first == last:
                assert sizes[b] == table[b + 1] - table[b]                    # a run that fills the bucket
    assert {S.SMALL_BUCKET, S.SMALL_BUCKET + 1}.issubset(seen_first) and {S.SMALL_BUCKET, S.SMALL_BUCKET - 1}.issubset(seen_last)


def test_edge_key_seams():
    c = JOIN["key_zero"]
    assert (c["genome"]["kmer"] == 0).sum() == 3 and (c["reads"]["kmer"] == 0).sum() == 5
    assert (R.run_counts(c["genome"], c["reads"])[c["reads"]["kmer"] == 0] == 0).all()
    parities = set()
    for c in S.edge_key_cases()[1:]:
        gk = c["genome"]["kmer"]
        assert gk[-1] == S.ALL_ONES and (gk == S.ALL_ONES).sum() == c["ones"], c["name"]
        hits = R.run_counts(c["genome"], c["reads"])[c["reads"]["kmer"] == S.ALL_ONES]
        assert len(hits) >= 3 and (hits == c["ones"]).all(), c["name"]
        parities.add((c["ones"], len(gk) & 1))
    assert parities == {(o, p) for o in (1, 2, 5) for p in (0, 1)}


def test_run_length_and_block_total_seams():
    c = JOIN["run_lengths"]
    assert set(c["run_lengths"]) == {1, S.RUN_STEPS, S.RUN_STEPS + 1, S.RUN_STEPS + 2, S.BIG, S.BIG + 1, 5000}
    assert set(c["run_lengths"]).issubset(set(R.run_counts(c["genome"], c["reads"]).tolist()))
    want = {"flat_4096": S.FLAT_MAX, "per_thread_4097": S.FLAT_MAX + 1}
    for c in S.block_total_cases():
        tot, lng = S.tile_totals(c), S.tile_long_runs(c)
        assert len(tot) == 2 and tot[0] == c["tile0_total"] and lng[0] == c["tile0_long_runs"], c["name"]
        short = c["name"].split("/")[1]
        if short in want:
            assert tot[0] == want[short] and lng[0] == 0
    c = JOIN["block_total/queue_overflow"]
    assert S.tile_long_runs(c)[0] == 70 > S.BIGQ and S.tile_totals(c)[0] > S.FLAT_MAX
    assert (R.run_counts(c["genome"], c["reads"])[:S.JOIN_TILE] > S.BIG).sum() == 70
    c = JOIN["block_total/one_run_of_5000"]
    cnt = R.run_counts(c["genome"], c["reads"])[:S.JOIN_TILE]
    assert sorted(cnt.tolist())[-2:] == [0, 5000] and 5000 > S.FLAT_MAX


def test_strand_offset_seams():
    c = JOIN["strand_offset"]
    lay = c["layout"]
    t = _as_tuples(R.join(c["genome"], c["reads"], c["read_len"], lay), lay)
    relb = [x[2] + lay[3] for x in t]
    assert (min(relb), max(relb)) == c["rel_extremes"] == (0, (1 << lay[2]) - 1)
    assert max(x[0] for x in t) == c["top_ids"][0] == (1 << lay[0]) - 1 and max(x[1] for x in t) == c["top_ids"][1] == (1 << lay[1]) - 1
    g_rc, r_rc = (c["genome"]["meta"] >> np.uint32(30)) & 1, (c["reads"]["meta"] >> np.uint32(30)) & 1
    for k in set(c["genome"]["kmer"].tolist()):
        assert set(g_rc[c["genome"]["kmer"] == k].tolist()) == {0, 1} and set(r_rc[c["reads"]["kmer"] == k].tolist()) == {0, 1}
    ids = c["reads"]["meta"] & np.uint32(R.ID_MASK)
    L = c["read_len"][ids]
    assert (c["reads"]["offset"] == 0).any() and (c["reads"]["offset"] == L - R.K).any() and len(set(L.tolist())) >= 3
    assert {x[3] for x in t} == {0, 1}


def test_merge_seams():
    for c in S.sorted_bits_cases():
        stb = c["sorted_top_bits"]
        k = c["reads"]["kmer"]
        assert not (k[1:] >= k[:-1]).all(), c["name"]                         # shuffled below the sorted bits
        assert ((k >> np.uint64(64 - stb))[1:] >= (k >> np.uint64(64 - stb))[:-1]).all()
    pairs = {(c["sorted_top_bits"], c["bucket_bits"]) for c in S.sorted_bits_cases()}
    assert {s for s, _b in pairs} == {8, 16, 24} and any(s < b for s, b in pairs) and any(s >= b for s, b in pairs)
    seen = set()
    for c in S.range_cases():
        (lo, hi), = S.merge_ranges(c)
        assert hi - lo == c["range_len"] and lo == c["range_start"], c["name"]
        seen.add((hi - lo, lo & 1))
    assert seen == {(n, p) for n in (0, 1, S.MP - 1, S.MP, S.MP + 1, 2 * S.MP + 1) for p in (0, 1)}
    seen = set()
    for c in S.piece_cases():
        assert c["piece_run"] in S.piece_index_of_runs(c), c["name"]
        seen.add(c["piece_run"])
    assert seen == {(s, r) for s in (S.MP - 2, S.MP - 1, S.MP) for r in (1, 2, 3, 4, 5, 6, S.MP + 4)}
    seen = set()
    for c in S.column_end_cases():
        gk = c["genome"]["kmer"]
        assert (gk == gk[-1]).sum() == c["end_run"] and int(gk[-1]) in set(c["reads"]["kmer"].tolist()), c["name"]
        seen.add((len(gk) & 1, len(gk) < S.MP))
    assert seen == {(0, True), (1, True), (0, False), (1, False)}
    c = JOIN["wide_tile"]
    assert len(c["reads"]) == S.JOIN_TILE and S.merge_ranges(c) == [(0, len(c["genome"]))] and len(c["genome"]) > 2 * S.MP


# ---- the unique cases -----------------------------------------------------------------------------------------------
def test_unique_case_seams():
    cases = S.unique_sorted_cases()
    names = [n for n, _l, _k in cases]
    assert len(set(names)) == len(names)
    assert {lay[2] for _n, lay, _k in cases} == {15, 20, 27} and max(sum(lay[:3]) + 1 for _n, lay, _k in cases) == 63
    for name, lay, keys in cases:
        assert (keys[1:] >= keys[:-1]).all() and int(keys.max()) >> (sum(lay[:3]) + 1) == 0, name
        short = name.split("/")[1]
        w = S.keep_flags_by_wave(keys, lay)
        relb = (keys >> np.uint64(1)) & np.uint64((1 << lay[2]) - 1)
        if short in ("n=1", "n=255", "n=256", "n=257"):
            assert len(keys) == int(short[2:])
        if short == "chain_by_2":
            assert len(keys) == 1000 > 3 * S.GROUP_BLOCK and w.sum() == 500          # 0, 4, 8, ...: every second one
        if short == "chain_by_1":
            assert len(keys) == 1000 and w.sum() == 334                                # 0, 3, 6, ...
        if short == "step2_then_gap3":
            assert w.reshape(-1)[:len(keys)].tolist()[:6] == [True, False, True, False, True, False]
        if short == "two_2s_then_gap3":
            assert w.reshape(-1)[:6].tolist() == [True, False, True, True, False, True]   # 0 (2) 4 7 (9) 11
        if short == "equal_rel_across_groups":
            assert w.sum() == 4 and len(keys) == 12
        if short == "identical_200":
            assert len(keys) == 200 and w.sum() == 1 and not w[1].any() and not w[2].any()
        if short == "survivor_in_lane_63":
            assert not w[1].any() and not w[2].any() and w[3].tolist() == [False] * 63 + [True] and w.sum() == 2
        if short == "rel_field_edges":
            assert relb.min() == 0 and relb.max() == (1 << lay[2]) - 1
    for step in (0, 1, 2, 3, 4):
        assert "rel15/step%d" % step in names


def test_grouped_case_seams():
    cases = S.unique_grouped_cases()
    names = [n for n, _l, _k in cases]
    assert len(set(names)) == len(names)
    G, B = S.GROUP_CAP, S.GROUP_BLOCK
    for name, lay, keys in cases:
        short = name.split("/")[1]
        hi = keys >> np.uint64(lay[2] + 1)
        assert (hi[1:] >= hi[:-1]).all(), name
        gs = S.group_sizes(keys, lay)
        sizes = [s for _a, s in gs]
        assert R.has_big_group(keys, lay, G) == (max(sizes) > G) == (short in ("size_65", "g65_lane255")), name
        if max(sizes) >= 3 and not short.startswith("zero_group_of_3"):
            assert not (keys[1:] >= keys[:-1]).all(), name                     # the low bits really are shuffled
        if short == "sizes_1_2_3_63_64":
            assert {1, 2, 3, G - 1, G}.issubset(set(sizes))
        if short in ("size_65", "g65_lane255"):
            assert G + 1 in sizes
        if short == "g64_lane0":
            assert gs[0] == (0, G)
        if short == "g64_lane0_block1":
            assert (B, G) in gs
        if short in ("g64_lane255", "g64_lane255_is_the_end"):
            assert (B - 1, G) in gs and (short == "g64_lane255" or len(keys) == B - 1 + G)
        if short == "g65_lane255":
            assert (B - 1, G + 1) in gs
        if short == "g64_straddles":
            a = [a for a, s in gs if s == G][0]
            assert a < B < a + G
        if short.startswith("n_mod_256="):
            assert len(keys) % B == int(short.split("=")[1]) and len(keys) > B and sizes[-1] > 1
        if short.startswith("zero_group_of_"):
            assert len(gs) == 1 and len(keys) == int(short.rsplit("_", 1)[1]) and int(hi[0]) == 0
    shorts = {n.split("/")[1] for n in names}
    assert {"zero_group_of_3", "zero_group_of_64", "n_mod_256=0", "n_mod_256=1", "n_mod_256=255"}.issubset(shorts)
