"""The cases of tests/merge_seams.py on the CPU: cutting a batch-global table into shards and merging them again gives the table
back byte for byte (merge_ref), the counts and the export restated plainly equal what the construction implies, the plain merge
agrees with kslam_amd.dist.reassemble on every field but cigar_off and on the ops every row addresses, every case keeps the
preconditions the kernels rely on, and -- without a broken kernel on a GPU -- the case list can SEE each plausible mistake of
csrc/merge.hip: a restatement of the kernels in their own terms (the walk in steps of 256 rows, a thread a 16-byte piece, the
shard lookup over row bases) equals the reference on every case, and each deliberately wrong variant of it differs on the cases
named beside it."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_seams as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.all_cases()
EVERY = CASES["X"] + CASES["M"]                    # S is the head of X
BY_NAME = {c["name"]: c for c in EVERY}
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def _name(case):
    return case["name"]


def _src(name):
    with open(os.path.join(ROOT, "k-slam_amd", "csrc", name)) as f:
        return f.read()


def test_the_sizes_the_cases_are_built_around_are_the_kernels():
    merge, common, api = _src("merge.hip"), _src("common.h"), _src("api_multi.hip")
    assert re.search(r"MERGE_MAX_SHARDS = %d;" % S.MAX_SHARDS, common)
    assert "base += %d" % S.WALK in merge and "dim3(1), dim3(%d), 0, s, d_rows, n, d_out2" % S.WALK in merge
    assert "const uint64_t i = g / %d;" % S.PIECES in merge and "(%d * n + %d) / %d" % (S.PIECES, S.BLOCK - 1, S.BLOCK) in merge
    assert "(n_rows + %d) / %d" % (S.BLOCK - 1, S.BLOCK) in merge
    assert api.count("(1ull << 31)") >= 4 and S.MAX_PAIRS == 1 << 31
    assert S.OVERLAP_DT.itemsize == 16 * S.PIECES and S.OVERLAP_DT.fields["cigar_len"][1] == 32 and S.OVERLAP_DT.fields["cigar_off"][1] == 40


def test_the_case_list_names_every_seam_once_and_loads_quickly():
    import time
    t0 = time.perf_counter()
    again = S.all_cases()
    assert time.perf_counter() - t0 < 1.0
    names = [c["name"] for c in EVERY]
    assert len(set(names)) == len(names)
    assert [c["name"] for c in CASES["S"]] == names[:len(CASES["S"])]
    for fam in "SXM":
        for a, b in zip(CASES[fam], again[fam]):          # generated from seeds: the same bytes every time
            assert a["rows"].tobytes() == b["rows"].tobytes() and a["pool"].tobytes() == b["pool"].tobytes(), a["name"]
    for n in (0, 1, 2, 255, 256, 257):
        for n_r1 in {0, 1, n - 1, n} & set(range(n + 1)):
            assert S.counts_of(BY_NAME["n%d_r1_%d" % (n, n_r1)])[:2] == (n, n_r1)
    assert BY_NAME["n0_pairs0"]["bounds"] == [(5, 5)]
    for d in S.WALK_DISTANCES:
        for r1 in (0, 1):
            c = BY_NAME["walk_d%d_r1cig%d" % (d, r1)]
            n, n_r1, n_cig, c1 = S.counts_of(c)
            lens = c["rows"]["cigar_len"][n_r1:]
            assert int(np.flatnonzero(lens)[0]) == d and (c1 > 0) == bool(r1) and n == n_r1 + d + 5
    for n_r1 in S.EXPORT_SPLITS:
        assert S.counts_of(BY_NAME["x_r1_%d_of_200" % n_r1])[:2] == (200, n_r1)
    c = BY_NAME["x_read_ids_to_2p32"]
    assert c["n_pairs"] == (1 << 31) - 1 and int(c["rows"]["read"].max()) == (1 << 32) - 3
    r1, r2, _, _, pb1, pb2 = S.exported(BY_NAME["x_high_word_bases"])
    assert (pb1, pb2) == ((1 << 32) - 3, (1 << 33) + (1 << 32) - 1)
    for part, base in ((r1, pb1), (r2, pb2)):             # offsets on both sides of the carry, and rows without a CIGAR
        off = part["cigar_off"][part["cigar_len"] > 0].astype(np.uint64)
        assert ((off >> np.uint64(32)) == np.uint64(base >> 32)).any() and ((off >> np.uint64(32)) == np.uint64((base >> 32) + 1)).any()
        assert (part["cigar_len"] == 0).any()
    assert sorted(len(BY_NAME[k]["bounds"]) for k in ("m1", "m2", "m3", "m255", "m256")) == [1, 2, 3, 255, 256]
    starts = np.cumsum([s[2] for s in S.gathered(BY_NAME["m_rows_255_256_257_512"])[2]])[:-1].tolist()
    assert starts == [255, 256, 257, 512]
    assert set(np.unique(BY_NAME["m_cigar_0_1_300"]["rows"]["cigar_len"]).tolist()) == {0, 1, 300}
    for name in S.EQUIVALENCE:
        assert sum(1 for s in S.gathered(BY_NAME[name])[2] if s[2] > 1) >= 3, name
    assert len(EVERY) < 200 and max(len(c["rows"]) for c in EVERY) <= 3000


@pytest.mark.parametrize("case", EVERY, ids=_name)
def test_cutting_into_shards_and_merging_gives_the_table_back(case):
    parts = S.split_batch(case["rows"], case["pool"], case["bounds"], case["n_pairs"])
    assert sum(len(r) for r, _ in parts) == len(case["rows"]), "a row outside every shard's pair range"
    rows, pool = S.merge_ref(S.shards_of(case), case["bounds"], case["n_pairs"])
    assert rows.tobytes() == case["rows"].tobytes() and pool.tobytes() == case["pool"].tobytes()
    for s, (r, p) in enumerate(S.shards_of(case)):
        lo, hi = case["bounds"][s]
        n, n_r1, n_cig, c1 = S.counts_ref(r, hi - lo)
        assert (n, n_r1, n_cig + case["junk"].get(s, 0), c1) == S.counts_of(case, s)
        assert n_cig + case["junk"].get(s, 0) == len(p)


@pytest.mark.parametrize("case", CASES["X"], ids=_name)
def test_export_restated_plainly_is_the_table_cut_at_the_split(case):
    (rows, pool), (lo, hi) = S.shards_of(case)[0], case["bounds"][0]
    e1, e2, p1, p2, pb1, pb2 = S.exported(case)
    g1, g2, q1, q2 = S.export_ref(rows, pool, hi - lo, lo, case["n_pairs"], pb1, pb2)
    assert g1.tobytes() == e1.tobytes() and g2.tobytes() == e2.tobytes()
    assert q1.tobytes() == p1.tobytes() and q2.tobytes() == p2.tobytes()
    both = np.concatenate([e1, e2])
    assert (both["cigar_off"][both["cigar_len"] == 0] == 0).all()


@pytest.mark.parametrize("case", EVERY, ids=_name)
def test_plain_merge_agrees_with_dist_reassemble(kslam, case):
    kd = importlib.import_module("kslam_amd.dist")
    parts = S.shards_of(case)
    host, hpool = kd.reassemble(parts, case["bounds"], case["n_pairs"], S.OVERLAP_DT)
    rows, pool = S.merge_ref(parts, case["bounds"], case["n_pairs"])
    assert len(host) == len(rows)
    for f in ("read",) + S.PASS_THROUGH:
        assert (host[f] == rows[f]).all(), f
    lens = rows["cigar_len"].astype(np.int64)
    assert S.row_ops(hpool, host["cigar_off"].astype(np.int64), lens).tobytes() == S.row_ops(pool, rows["cigar_off"].astype(np.int64), lens).tobytes()
    assert (host["cigar_off"][lens == 0] == 0).all()


def test_reassemble_leaves_the_pool_in_shard_order(kslam):
    """why dist.reassemble cannot be the byte oracle, and why its output must not be adopted and exported again (the
    precondition at the top of csrc/merge.hip): its rows go [all R1 | all R2] while the pools stay shard after shard, so the
    offsets do not grow with the row number, and the walk from the split would take a later row's offset for n_cigar_r1"""
    kd = importlib.import_module("kslam_amd.dist")
    case = BY_NAME["m3"]
    host, _ = kd.reassemble(S.shards_of(case), case["bounds"], case["n_pairs"], S.OVERLAP_DT)
    off = host["cigar_off"][host["cigar_len"] > 0].astype(np.int64)
    assert (np.diff(off) < 0).any()
    n_r1 = int((host["read"] < case["n_pairs"]).sum())
    assert model_counts(host, case["n_pairs"], int(host["cigar_len"].sum()))[:2] == (len(host), n_r1)
    assert model_counts(host, case["n_pairs"], int(host["cigar_len"].sum()))[3] != int(host["cigar_len"][:n_r1].sum())


@pytest.mark.parametrize("case", EVERY, ids=_name)
def test_every_case_keeps_the_documented_preconditions(case):
    rows, n_pairs = case["rows"], case["n_pairs"]
    assert 0 <= n_pairs < S.MAX_PAIRS and 1 <= len(case["bounds"]) <= S.MAX_SHARDS and len(rows) <= 3000
    key = np.stack([rows["read"].astype(np.int64), rows["entry"].astype(np.int64), rows["rel"].astype(np.int64)])
    d = np.diff(key, axis=1)
    assert ((d[0] > 0) | ((d[0] == 0) & ((d[1] > 0) | ((d[1] == 0) & (d[2] > 0))))).all(), "sorted by (read, entry, rel), no two rows alike"
    assert (rows["read"].astype(np.int64) < 2 * n_pairs).all() and (rows["pad"] == 0).all() and (rows["pad2"] == 0).all()
    for f in ("rel", "ref_begin"):
        assert len(np.unique(rows[f])) == len(rows), "a row-unique pattern in pieces 0 and 1"
    assert len(np.unique(case["pool"])) == len(case["pool"]) and not (case["pool"] == S.JUNK_WORD).any()
    prev = 0
    for (lo, hi), (r, p) in zip(case["bounds"], S.shards_of(case)):
        assert prev <= lo <= hi <= n_pairs and hi - lo < S.MAX_PAIRS
        prev = hi
        assert (np.diff(r["read"].astype(np.int64)) >= 0).all(), "sorted by local read id: the R1 rows first"
        assert (r["read"].astype(np.int64) < 2 * (hi - lo)).all()
        has = r["cigar_len"] > 0
        off, ln = r["cigar_off"][has].astype(np.int64), r["cigar_len"][has].astype(np.int64)
        assert (off[1:] == off[:-1] + ln[:-1]).all() and (len(off) == 0 or off[0] == 0), "offsets grow with the row number"
        assert (r["cigar_off"][~has] == 0).all() and int(ln.sum()) <= len(p)


# ---- the kernels restated in their own terms, with the mistakes one could make in them -----------------------------------------
NONE = M64


def model_counts(rows, n_local_pairs, n_cigar, fault=None):
    """k_shard_split + k_shard_first_cigar + what the API makes of ~0"""
    read, ln, off = rows["read"].tolist(), rows["cigar_len"].tolist(), rows["cigar_off"].tolist()
    n = len(read)
    lo, hi = 0, n
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if read[mid] < n_local_pairs:
            lo = mid + 1
        else:
            hi = mid
    first = NONE
    if n and n_cigar:
        base = lo
        while base < n:
            seen = [off[i] for i in range(base, min(base + S.WALK, n)) if ln[i]]
            if seen:
                first = min(seen)
                break
            if fault == "walk_stops_after_one_step":
                break
            base += S.WALK
    if first == NONE:
        first = 0 if fault == "none_found_read_as_0" else n_cigar
    return n, lo, n_cigar, first


def model_export(rows, n_local_pairs, pair_lo, n_total, pb1, pb2, n_r1, c1, fault=None):
    """k_export_rows, a thread a piece -> {(side, piece index there): the four words}"""
    pieces = np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 4).tolist()
    out = {}
    for g, v in enumerate(pieces):
        i = g // 3
        part = g - 3 * i
        r1 = i < n_r1
        if part == 0:
            v[0] = (pair_lo + v[0] if r1 else n_total + pair_lo + (v[0] - n_local_pairs)) & M32
        elif part == 2:
            off = v[2] | (v[3] << 32)
            noff = 0
            if v[0] or fault == "rebases_rows_without_cigar":
                noff = (pb1 + off if r1 else pb2 + (off - (0 if fault == "forgets_n_cigar_r1" else c1))) & M64
            if fault == "offset_cut_to_32_bits":
                noff &= M32
            v[2], v[3] = noff & M32, noff >> 32
        to_r1 = (g // S.WAVE * S.WAVE < 3 * n_r1) if fault == "routes_by_wave" else r1
        out[("r1", g) if to_r1 else ("r2", g - 3 * n_r1)] = v
    return out


def wanted_export(case):
    e1, e2 = S.exported(case)[:2]
    out = {}
    for side, part in (("r1", e1), ("r2", e2)):
        for g, v in enumerate(np.ascontiguousarray(part).view(np.uint32).reshape(-1, 4).tolist()):
            out[(side, g)] = v
    return out


def model_merge(rows, pool, shards, n_pairs, fault=None):
    """k_merge_plan + k_merge_rows + the scan + k_merge_cigars on the gathered buffers"""
    n_sh, n = len(shards), len(rows)
    row_base, pool_base, a, b = [], [], 0, 0
    for lo, hi, n_rows, n_cig in shards:
        row_base.append(a)
        pool_base.append(b)
        a, b = a + n_rows, b + n_cig
    read, ln, off = rows["read"].tolist(), rows["cigar_len"].tolist(), rows["cigar_off"].tolist()
    n_r1 = []
    for s, (plo, phi, n_rows, _) in enumerate(shards):
        lo, hi = 0, n_rows
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            if read[row_base[s] + mid] < phi - plo:
                lo = mid + 1
            else:
                hi = mid
        n_r1.append(lo)
    out_r1, out_r2, a = [], [], 0
    for s in range(n_sh):
        out_r1.append(a)
        a += n_r1[s]
    for s in range(n_sh):
        out_r2.append(a)
        a += shards[s][2] - n_r1[s]
    out = np.zeros(n, dtype=S.OVERLAP_DT)
    src = [0] * n
    for i in range(n):
        s = 0
        while s + 1 < n_sh and i >= row_base[s + 1]:
            s += 1
        if fault == "first_shard_of_equal_row_bases":
            while s > 0 and row_base[s - 1] == row_base[s]:
                s -= 1
        plo, phi = shards[s][:2]
        n_loc, k = phi - plo, i - row_base[s]
        r2 = read[i] >= n_loc
        pos = out_r2[s] + (k - n_r1[s]) if r2 else out_r1[s] + k
        if not 0 <= pos < n:
            return None, None                                   # a store outside the output
        out[pos] = rows[i]
        out["read"][pos] = (n_pairs + plo + (read[i] - n_loc) if r2 else plo + read[i]) & M32
        src[pos] = pool_base[s] + off[i] if ln[i] or fault == "rebases_rows_without_cigar" else 0
    lens = out["cigar_len"].tolist()
    pool_out = np.zeros(sum(lens), dtype=np.uint32)
    at = 0
    for i in range(n):
        out["cigar_off"][i] = src[i]
        if lens[i]:
            pool_out[at:at + lens[i]] = pool[src[i]:src[i] + lens[i]]
            out["cigar_off"][i] = at
        at += lens[i]
    return out, pool_out


def _counts_differ(case, fault):
    (rows, pool), (lo, hi) = S.shards_of(case)[0], case["bounds"][0]
    return model_counts(rows, hi - lo, len(pool), fault) != S.counts_of(case)


def _export_differs(case, fault):
    (rows, pool), (lo, hi) = S.shards_of(case)[0], case["bounds"][0]
    _, n_r1, _, c1 = S.counts_of(case)
    pb1, pb2 = S.exported(case)[4:]
    return model_export(rows, hi - lo, lo, case["n_pairs"], pb1, pb2, n_r1, c1, fault) != wanted_export(case)


def _merge_differs(case, fault):
    rows, pool, shards = S.gathered(case)
    out, pool_out = model_merge(rows, pool, shards, case["n_pairs"], fault)
    return out is None or out.tobytes() != case["rows"].tobytes() or pool_out.tobytes() != case["pool"].tobytes()


@pytest.mark.parametrize("case", CASES["X"], ids=_name)
def test_split_and_export_restated_as_the_kernels_do_them_give_the_table(case):
    assert not _counts_differ(case, None)
    assert not _export_differs(case, None)


@pytest.mark.parametrize("case", CASES["M"], ids=_name)
def test_merge_restated_as_the_kernels_do_it_gives_the_table(case):
    assert not _merge_differs(case, None)


# the mistake -> (where it is made, the cases that must see it, the cases that must NOT: the seam is where the names say)
FAULTS = {
    "forgets_n_cigar_r1": (_export_differs, "X", ["x_r1_22_of_200", "walk_d0_r1cig1", "walk_d1000_r1cig1", "x_high_word_bases"],
                           ["x_r1_0_of_200", "walk_d0_r1cig0"]),
    "walk_stops_after_one_step": (_counts_differ, "S", ["walk_d%d_r1cig%d" % (d, r) for d in S.WALK_DISTANCES if d >= S.WALK for r in (0, 1)]
                                  + ["walk_last_step_1_row"],
                                  ["walk_d%d_r1cig%d" % (d, r) for d in S.WALK_DISTANCES if d < S.WALK for r in (0, 1)]),
    "none_found_read_as_0": (_counts_differ, "S", ["walk_none_r2_300", "walk_none_r2_256", "walk_none_r2_1", "n1_r1_1", "n257_r1_257"],
                             ["no_cigar_anywhere", "walk_d1000_r1cig1"]),
    "first_shard_of_equal_row_bases": (_merge_differs, "M", ["m3_empty_front_norows", "m3_empty_middle_norows", "m3_empty_front_norange",
                                                             "m3_empty_middle_norange", "m3_100_empty_front", "m3_100_empty_middle",
                                                             "m255", "m256"], ["m3", "m3_empty_end_norows", "m3_100_empty_end"]),
    "rebases_rows_without_cigar": (_export_differs, "X", ["x_r1_85_of_200", "x_high_word_bases", "no_cigar_anywhere"], []),
    "offset_cut_to_32_bits": (_export_differs, "X", ["x_high_word_bases", "x_high_word_bases_read_ids_to_2p32", "x_r1_only_high_word",
                                                     "x_r2_only_high_word"], ["x_r1_85_of_200", "x_read_ids_to_2p32"]),
    "routes_by_wave": (_export_differs, "X", ["x_r1_1_of_200", "x_r1_21_of_200", "x_r1_22_of_200", "x_r1_85_of_200", "x_r1_86_of_200",
                                              "x_r1_171_of_200", "n2_r1_1", "n256_r1_255"],
                       ["x_r1_0_of_200", "x_r1_200_of_200", "n256_r1_256", "n257_r1_256"]),   # 3 * 256 is a multiple of the wave
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_each_plausible_mistake_is_seen_by_the_cases_named_for_it(fault):
    differs, fam, must, must_not = FAULTS[fault]
    seen = [c["name"] for c in CASES[fam] if differs(c, fault)]
    assert must, fault
    for name in must:
        assert name in seen, "%s: case %s does not tell the wrong variant from the construction (seen by: %s)" % (fault, name, seen)
    for name in must_not:
        assert name not in seen, "%s: case %s sees it, so the seam is not where its name says" % (fault, name)


def test_rows_without_cigar_rebased_in_the_merge_is_seen_too():
    seen = [c["name"] for c in CASES["M"] if _merge_differs(c, "rebases_rows_without_cigar")]
    for name in ("m2", "m3", "m_cigar_0_1_300", "m_junk_on_rows_without_cigar", "m256"):
        assert name in seen, "case %s does not see cigar_off re-based on rows without a CIGAR (seen by: %s)" % (name, seen)
    assert "m1" not in seen                                # one shard: its pool base is 0


def test_refusals_are_refusals_by_the_documented_rules():
    for name, shards, n_pairs, null, _ in S.refusals():
        bad = not 1 <= len(shards) <= S.MAX_SHARDS
        for k, (lo, hi, n_rows, n_cig) in enumerate(shards):
            bad |= hi < lo or hi > n_pairs or (k > 0 and lo < shards[k - 1][1])
        rows, ops = sum(s[2] for s in shards), sum(s[3] for s in shards)
        bad |= bool(rows and {"rows_in", "rows_out"} & set(null)) or bool(ops and {"pool_in", "pool_out"} & set(null))
        assert bad, name
