"""Case builders for the seams of the device tail front (k-slam_amd/csrc/pairs.hip): overlap records built row by row, so
that a read pair has exactly 256 or 257 rows, a group exactly 96 or 97 alignment pairs, an entry exactly 4000 or 4001 spans, a
stretch of reads without rows is exactly 63, 64 or 65 long.  Pure numpy: tests/test_tail_seams.py holds every case to the
host tail and the oracle's restatement on the CPU and recomputes the count each case claims; tests/test_gpu_tail_seams.py
runs the same cases through the device.

A case is a dict: name, ov (OVERLAP_DT, sorted by read, entry, rel), n_reads, read_lens, paired, score_threshold,
score_fraction, stages, claim {measure: exact value} and, for the pseudo-assembly hand-back, pseudo_cap (KSLAM_PSEUDO_CAP)
and on_device (whether the device keeps stage 4)."""
import numpy as np

# copies of the thresholds in csrc/pairs.hip (test_tail_seams.py compares them with the source text)
PAIR_BIG = 256
SCREEN_BIG = 96
PSEUDO_CAP = 4000
PSEUDO_CAP_GLOBAL = 1 << 18
GAP = 64              # k_row_starts: cur - prev > 64 goes to the side list
CHAIN_SLACK = 20      # a span starting more than reach - 20 starts a chain
LADDER_STEP = 1000    # a percentile step above this sets the limit
READ_LEN = 100
INT32_MAX = 2 ** 31 - 1

OVERLAP_DT = np.dtype([("read", "<u4"), ("entry", "<u4"), ("rel", "<i4"), ("revcomp", "u1"), ("pad", "u1"), ("score", "<u2"),
                       ("ref_begin", "<i4"), ("ref_end", "<i4"), ("query_begin", "<i4"), ("query_end", "<i4"),
                       ("cigar_len", "<u4"), ("pad2", "<u4"), ("cigar_off", "<u8")])


def insert_limit_ref(values):
    """getMaxAllowedInsertSize as host/tail.cpp: max_allowed_insert computes it, on int32 insert sizes"""
    sz = np.sort(np.asarray(values, dtype=np.int32))
    n = len(sz)
    if n == 0:
        return 0xFFFFFFFF
    lad = [int(sz[int(np.floor(n * i / 100.0))]) for i in range(100)]
    limit = 0
    for i in range(99):
        if lad[i + 1] - lad[i] > LADDER_STEP:
            limit = lad[i]
            break
    lq, uq = int(sz[int(np.floor(n * 0.25))]), int(sz[int(np.floor(n * 0.75))])
    hi = uq + 2 * (uq - lq)
    if limit:
        hi = limit
    if hi == 0:
        hi = INT32_MAX
    kept = sz[(sz >= 0) & (sz <= hi)]
    k = len(kept)
    sq = (kept.astype(np.uint32) * kept.astype(np.uint32)).view(np.int32)      # the product wraps as the reference's int does
    s = float(np.add.accumulate(kept.astype(np.float64))[-1]) if k else 0.0   # sequential, in sorted order
    q = float(np.add.accumulate(sq.astype(np.float64))[-1]) if k else 0.0
    with np.errstate(all="ignore"):
        mean = np.float64(s) / np.float64(k)
        r = np.floor(mean + 6 * np.sqrt(np.float64(q) / np.float64(k) - mean * mean))
    return 0xFFFFFFFF if np.isnan(r) else int(r) & 0xFFFFFFFF


class Rows:
    """overlap rows, column chunks at a time; done() sorts them by (read, entry, rel), ties in the order they were added"""

    def __init__(self):
        self.cols = []

    def add(self, read, entry, rel, revcomp, score, ref_begin=None, ref_end=None):
        read, entry, rel, revcomp, score = np.broadcast_arrays(np.asarray(read, dtype=np.int64), np.asarray(entry, dtype=np.int64),
                                                               np.asarray(rel, dtype=np.int64), np.asarray(revcomp, dtype=np.int64),
                                                               np.asarray(score, dtype=np.int64))
        rb = rel if ref_begin is None else np.broadcast_to(np.asarray(ref_begin, dtype=np.int64), rel.shape)
        re = rb + READ_LEN - 1 if ref_end is None else np.broadcast_to(np.asarray(ref_end, dtype=np.int64), rel.shape)
        self.cols.append([np.ravel(x) for x in (read, entry, rel, revcomp, score, rb, re)])

    def pair(self, u, mid, entry, rel1, insert, s1=100, s2=90):
        """a forward mate-1 row and a reverse mate-2 row behind it: one alignment pair of this insert size"""
        rel1, insert = np.asarray(rel1, dtype=np.int64), np.asarray(insert, dtype=np.int64)
        self.add(u, entry, rel1, 0, s1)
        self.add(np.asarray(u, dtype=np.int64) + mid, entry, rel1 + insert - READ_LEN, 1, s2)

    def done(self):
        a = np.zeros(sum(len(c[0]) for c in self.cols), dtype=OVERLAP_DT)
        if len(a):
            for k, f in enumerate(("read", "entry", "rel", "revcomp", "score", "ref_begin", "ref_end")):
                col = np.concatenate([c[k] for c in self.cols])
                assert col.min() >= np.iinfo(OVERLAP_DT[f]).min and col.max() <= np.iinfo(OVERLAP_DT[f]).max, f
                a[f] = col
            a["query_end"] = READ_LEN - 1
            a = a[np.lexsort((a["rel"], a["entry"], a["read"]))]
        return a


class Case(dict):
    """a case; its arrays ("ov", "read_lens") are built when first asked for, so that listing the cases stays cheap"""

    def __missing__(self, key):
        if key == "ov":
            rows = self["rows"]() if callable(self["rows"]) else self["rows"]
            ov = rows.done()
            assert len(ov) == 0 or int(ov["read"].max()) < self["n_reads"]
            self["ov"] = ov
        elif key == "read_lens":
            self["read_lens"] = np.full(self["n_reads"], READ_LEN, dtype=np.uint32)
        else:
            raise KeyError(key)
        return dict.__getitem__(self, key)


def _case(name, rows, n_reads, claim, paired=True, thr=0, frac=0.95, stages=3, pseudo_cap=None, on_device=True):
    """rows: a Rows, or a function that returns one (large batches)"""
    return Case(name=name, rows=rows, n_reads=n_reads, paired=paired, score_threshold=thr, score_fraction=frac, stages=stages,
                claim=claim, pseudo_cap=pseudo_cap, on_device=on_device)


# ---- A: the first-row table ------------------------------------------------------------------------------------------------
def _rows_on(reads_with_rows, mid):
    r = np.asarray(sorted(reads_with_rows), dtype=np.int64)
    R = Rows()
    m2 = r >= mid
    R.add(r, 3, np.where(m2, 1200, 1000), m2.astype(np.int64), 150 + r % 50)
    return R


def _with_stretches(n_reads, stretches):
    """reads that have rows: every read with r % 30 == 20 outside the open intervals (prev, cur), and the intervals' ends"""
    have = set(range(20, n_reads, 30))
    for prev, cur in stretches:
        have -= set(range(prev + 1, cur))
        have |= {x for x in (prev, cur) if 0 <= x < n_reads}
    return have


def cases_a():
    out = []
    n, mid = 400, 200
    for g in (GAP - 1, GAP, GAP + 1):
        for where, (prev, cur) in (("before_first", (-1, g)), ("inside_mate1", (10, 11 + g)), ("across_mid", (170, 171 + g)),
                                   ("after_last", (n - 1 - g, n))):
            out.append(_case("A-gap%d-%s" % (g, where), _rows_on(_with_stretches(n, [(prev, cur)]), mid), n,
                             {"longest_empty_stretch": g, "long_stretches": int(g + 1 > GAP)}))
    out.append(_case("A-gaps-300-600", _rows_on(_with_stretches(1400, [(50, 351), (500, 1101)]), 700), 1400,
                     {"longest_empty_stretch": 600, "long_stretches": 2}))
    out.append(_case("A-70-long-stretches", _rows_on(range(0, 4621, 66), 2311), 4622,
                     {"longest_empty_stretch": 65, "long_stretches": 70, "gap_cap": 4622 // 64 + 2}))
    out.append(_case("A-mate1-only", _rows_on(range(0, 20, 3), 20), 40, {"rows_mate1": 7, "rows_mate2": 0}))
    out.append(_case("A-mate2-only", _rows_on(range(20, 40, 3), 20), 40, {"rows_mate1": 0, "rows_mate2": 7}))
    out.append(_case("A-single-row", _rows_on([7], 20), 40, {"n_rows": 1, "longest_empty_stretch": 32}))
    out.append(_case("A-no-rows-40-reads", Rows(), 40, {"n_rows": 0, "longest_empty_stretch": 40, "long_stretches": 0}))
    out.append(_case("A-no-rows-200-reads", Rows(), 200, {"n_rows": 0, "longest_empty_stretch": 200, "long_stretches": 1}))
    R = Rows()
    R.pair(0, 1, 4, 1000, 300)
    out.append(_case("A-two-reads", R, 2, {"n_rows": 2, "n_units": 1}))
    return out


# ---- B: the pairing hand-over ----------------------------------------------------------------------------------------------
def _big_pair(R, u, mid, n1, n2, layout, heads=None):
    """n1 rows of mate 1 and n2 of mate 2 for unit u; scores 100 .. 200 in steps of 25"""
    k1, k2 = np.arange(n1), np.arange(n2)
    if layout == "one_entry":
        e1, e2, d1, d2 = np.full(n1, 5), np.full(n2, 5), k1, k2
    elif layout == "one_per_entry":       # mate 1 on the even entries, mate 2 on the odd ones: interleaved, nothing pairs
        e1, e2, d1, d2 = 2 * k1, 2 * k2 + 1, k1 * 0, k2 * 0
    elif layout == "heads":               # exactly `heads` entries
        e1, e2, d1, d2 = k1 % heads, k2 % heads, k1 // heads, k2 // heads
    else:                                 # "mixed": entries 0, 3, .. both mates, 1, 4, .. mate 1 only, 2, 5, .. mate 2 only, in pairs of rows
        e1 = np.array([e for e in range(3 * (n1 + 2)) if e % 3 != 2 for _ in (0, 1)][:n1], dtype=np.int64)
        e2 = np.array([e for e in range(3 * (n2 + 2)) if e % 3 != 1 for _ in (0, 1)][:n2], dtype=np.int64)
        d1, d2 = k1 % 2, k2 % 2
    R.add(u, e1, 1000 + 7 * d1, d1 % 3 == 2, 100 + 25 * (k1 % 5))
    R.add(u + mid, e2, 1203 + 7 * d2, d2 % 3 != 2, 100 + 25 * ((k2 + 2) % 5))


def _small_pairs(R, units, mid, s1=300, s2=290):
    units = np.asarray(list(units), dtype=np.int64)
    if len(units):
        R.pair(units, mid, 9, 2000 + units % 7, 280 + units % 41, s1, s2)


def cases_b():
    out = []
    for n1, n2 in ((128, 127), (128, 128), (257, 0), (0, 257), (1, 256), (128, 129)):
        for layout in ("one_entry", "one_per_entry", "mixed"):
            R, mid = Rows(), 8
            _small_pairs(R, (0, 1, 5, 7), mid)
            _big_pair(R, 3, mid, n1, n2, layout)
            claim = {"rows_largest_pair": n1 + n2, "rows_mate1_largest": n1, "rows_mate2_largest": n2, "n_big_pairs": int(n1 + n2 > PAIR_BIG)}
            if layout == "one_entry":
                claim["heads_largest_pair"] = 1
            if layout == "one_per_entry":
                claim["heads_largest_pair"] = n1 + n2
            out.append(_case("B-%d+%d-%s" % (n1, n2, layout), R, 2 * mid, claim, stages=1 if layout == "mixed" else 3))
    for h in (64, 65, 128, 129):
        R, mid = Rows(), 4
        _small_pairs(R, (0, 2), mid)
        _big_pair(R, 1, mid, 128, 129, "heads", h)
        out.append(_case("B-257-rows-%d-heads" % h, R, 2 * mid, {"rows_largest_pair": 257, "heads_largest_pair": h, "n_big_pairs": 1}))
    for thr, kept_big in ((250, 0), (150, 154)):
        R, mid = Rows(), 6
        _small_pairs(R, (0, 2, 5), mid)
        _big_pair(R, 3, mid, 128, 129, "heads", 65)
        out.append(_case("B-257-rows-threshold-%d" % thr, R, 2 * mid, {"rows_largest_pair": 257, "kept_rows": 6 + kept_big,
                                                                         "n_groups_out": 3 + int(kept_big > 0)}, thr=thr))
    # big pairs as unit 0, the last unit and units 255 / 256 (the edge of k_pair's 256-thread block)
    R, mid = Rows(), 600
    for u, lay in ((0, "mixed"), (255, "one_entry"), (256, "one_per_entry"), (599, "mixed")):
        _big_pair(R, u, mid, 128, 129, lay)
    _small_pairs(R, [u for u in range(600) if u not in (0, 255, 256, 599) and u % 3], mid)
    out.append(_case("B-big-at-0-255-256-last", R, 2 * mid, {"rows_largest_pair": 257, "n_big_pairs": 4, "n_units": 600}))
    for units in (1, 255, 256, 257):
        R = Rows()
        _small_pairs(R, range(units - 1), units)
        _big_pair(R, units - 1, units, 1, 256, "mixed")
        out.append(_case("B-%d-units" % units, R, 2 * units, {"n_units": units, "n_big_pairs": 1, "rows_largest_pair": 257}))
    for first_has in (False, True):       # a block of 256 read pairs without a single insert size next to one with 256
        R, mid = Rows(), 512
        lone, both = (np.arange(256, 512), np.arange(0, 256)) if first_has else (np.arange(0, 256), np.arange(256, 512))
        R.add(lone, 2, 1000, 0, 120)
        _small_pairs(R, both, mid)
        out.append(_case("B-block-without-inserts-%s" % ("second" if first_has else "first"), R, 2 * mid,
                         {"n_inserts": 256, "n_units": 512, "inserts_in_units_0_255": 256 if first_has else 0}, stages=1))
    # more big pairs than k_pair_big's grid of 2048 blocks
    mid = 2049

    def many_big_pairs():
        R = Rows()
        u = np.repeat(np.arange(mid), 128)
        k = np.tile(np.arange(128), mid)
        R.add(u, k % 65, 1000 + 7 * (k // 65) + u % 3, 0, 100 + 25 * (k % 5))
        u = np.repeat(np.arange(mid), 129)
        k = np.tile(np.arange(129), mid)
        R.add(u + mid, k % 65, 1203 + 7 * (k // 65), 1, 100 + 25 * ((k + u) % 5))
        return R
    out.append(_case("B-2049-big-pairs", many_big_pairs, 2 * mid, {"n_big_pairs": 2049, "rows_largest_pair": 257, "rows_smallest_pair": 257,
                                                      "n_rows": 2049 * 257}, thr=125))
    R = Rows()
    k = np.arange(300)
    R.add(4, k % 40, 1000 + k, k % 2, 100 + 25 * (k % 5))
    R.add([0, 9], 1, 500, 0, 150)
    out.append(_case("B-single-end-300-rows", R, 10, {"rows_largest_read": 300}, paired=False, thr=125, stages=2))
    return out


# ---- C: the insert-size statistics -----------------------------------------------------------------------------------------
def _insert_rows(values):
    """one read pair per value: its only alignment pair has this insert size (as int32; below zero: beyond 2^31 unsigned)"""
    v = np.asarray(values, dtype=np.int64)
    assert ((v < 0) | (v >= READ_LEN)).all()
    n = len(v)
    R = Rows()
    neg = v < 0
    rel1 = np.where(neg, -2 ** 31, 1000)
    R.pair(np.arange(n), n, np.arange(n) % 3, rel1, np.where(neg, v + 2 ** 32, v))
    return R


def _stat_case(name, values, extra=None):
    v = np.asarray(values, dtype=np.int64)
    claim = {"n_inserts": len(v), "max_insert_size": insert_limit_ref(v)}
    claim.update(extra or {})
    return _case("C-" + name, _insert_rows(v), 2 * len(v), claim, stages=1)


def limit_fixed_point():
    """insert sizes whose limit L is itself one of the values, next to an L + 1"""
    base = [200] * 100 + [400] * 100
    for L in range(500, 1200):
        if insert_limit_ref(base + [L, L + 1]) == L:
            return base + [L, L + 1], L
    raise AssertionError("no fixed point")


def cases_c():
    out = []
    for n in (1, 2, 3, 4, 99, 100, 101, 199, 200):
        out.append(_stat_case("n%d" % n, 300 + (np.arange(n) * 7) % 50))
    for pos in (0, 50, 98):
        for step in (LADDER_STEP, LADDER_STEP + 1):
            v = np.where(np.arange(100) <= pos, 300, 300 + step)
            out.append(_stat_case("ladder-step%d-at%d" % (step, pos), v, {"ladder_step": step, "ladder_position": pos}))
    out.append(_stat_case("all-negative", -5 - np.arange(40) * 1000, {"max_insert_size": 0xFFFFFFFF}))
    out.append(_stat_case("quartiles-minus3-minus2", [-3, -3, -3, -2, -2, -2, -2, 500], {"lower_quartile": -3, "upper_quartile": -2,
                                                                                      "max_insert_size": 500}))
    out.append(_stat_case("negative-at-ladder-break", [-5000] * 50 + [300] * 50, {"max_insert_size": 0xFFFFFFFF}))
    out.append(_stat_case("squares-wrap-ramp707", 100 + 707 * np.arange(100), {"inserts_above_46340": 34}))
    out.append(_stat_case("squares-wrap-ramp500", 100 + 500 * np.arange(200), {"inserts_above_46340": 107}))
    v, L = limit_fixed_point()
    out.append(_stat_case("at-limit-and-one-above", v, {"max_insert_size": L, "records_at_limit": 1, "records_at_limit_plus_1": 1}))
    return out


def stats_beyond_2p53():
    """4.4 M kept insert sizes just under 46 341: their squares add up to more than 2^53, the sums fall back to the sequential
    double accumulation (needs more than 2^53 / 46340^2 = 4 194 486 values)"""
    k = np.arange(4_400_000, dtype=np.int64)
    return (46001 + (k * 7919) % 340).astype(np.int32)


# ---- D: the screens --------------------------------------------------------------------------------------------------------
def _group(R, u, mid, K, n_far, s1=100, vary=True):
    """K alignment pairs for unit u, one per entry; the last n_far of them 5000 apart"""
    e = np.arange(K)
    R.pair(u, mid, e, 1000 + e % 5, np.where(e >= K - n_far, 5000 + e % 3, 300), s1, 60 + (e * 13) % 40 if vary else 90)


def _background(R, units, mid):
    units = np.asarray(list(units), dtype=np.int64)
    R.pair(units, mid, 2, 3000, 300, 100, 95)


def cases_d():
    out = []
    mid = 202
    for K in (SCREEN_BIG, SCREEN_BIG + 1):
        for far, tag in ((0, "none-beyond"), (K, "all-beyond"), (K // 2, "half-beyond")):
            for stages in ((1, 2, 3) if tag == "half-beyond" else (3,)):
                R = Rows()
                _group(R, 1, mid, K, far)
                _background(R, range(2, mid), mid)
                out.append(_case("D-%d-%s-stages%d" % (K, tag, stages), R, 2 * mid,
                                 {"pairs_largest_group": K, "cut_largest_group": K - far, "max_insert_size": 300}, stages=stages))
        R = Rows()
        _group(R, 1, mid, K, 0, vary=False)
        _background(R, range(2, mid), mid)
        out.append(_case("D-%d-all-scores-equal" % K, R, 2 * mid, {"pairs_largest_group": K, "distinct_scores_largest_group": 1,
                                                                    "pairs_out_largest_group": K}))
        # the bar: top 200, fraction 0.5: 100 stays, 99 goes
        R = Rows()
        e = np.arange(K)
        R.add(1, e, 1000, 0, np.where(e == 7, 200, np.where(e % 2 == 0, 100, 99)))
        _background(R, range(2, mid), mid)
        out.append(_case("D-%d-bar-equality" % K, R, 2 * mid, {"pairs_largest_group": K, "pairs_out_largest_group": int(((e % 2 == 0) | (e == 7)).sum())},
                         frac=0.5))
        R = Rows()
        R.add(1, e, 1000, 0, np.where(e % 10 == 3, 200, 199 - e % 4))
        _background(R, range(2, mid), mid)
        out.append(_case("D-%d-fraction-1" % K, R, 2 * mid, {"pairs_largest_group": K, "pairs_out_largest_group": int((e % 10 == 3).sum())},
                         frac=1.0))
    R = Rows()
    R.add(1, [0, 1, 2], 1000, 0, [100, 200, 99])
    _background(R, range(2, 20), 20)
    out.append(_case("D-3-bar-equality", R, 40, {"pairs_largest_group": 3, "pairs_out_largest_group": 2}, frac=0.5))
    R = Rows()
    _group(R, 0, 60, 4100, 2050)
    _background(R, range(1, 60), 60)
    out.append(_case("D-4100-pairs-half-beyond", R, 120, {"pairs_largest_group": 4100, "cut_largest_group": 2050}))
    # 97 would-be alignment pairs, every row under the threshold (scores 50 and 60 .. 99 against 100): the read pair has 194 rows,
    # so it is k_pair's thread that finds nothing to pair and the group reaches neither screen kernel (pairs_largest_group = 1 is a
    # background read pair's, whose mate 1 alone survives); the same through k_pair_big: B-257-rows-threshold-250
    R = Rows()
    _group(R, 1, mid, SCREEN_BIG + 1, 40, s1=50)
    _background(R, range(2, mid), mid)
    out.append(_case("D-97-nothing-survives-upstream", R, 2 * mid, {"rows_largest_pair": 194, "pairs_largest_group": 1,
                                                                     "n_groups_out": 200, "kept_rows": 200}, thr=100))
    # read pairs left without records first, last and between survivors (rows under the threshold, or none at all)
    R, mid = Rows(), 300
    alive = [u for u in range(2, 298) if u % 7 in (0, 1, 4)]
    _background(R, alive, mid)
    R.pair(np.array([0, 3, 5, 299]), mid, 1, 1000, 300, 20, 30)
    _group(R, 150, mid, SCREEN_BIG + 1, 30)
    out.append(_case("D-empty-first-last-between", R, 2 * mid, {"n_groups_out": len(alive) + 1, "first_group_out": 4, "last_group_out": 295,
                                                                 "n_units": 300}, thr=60))
    return out


# ---- E: pseudo-assembly ----------------------------------------------------------------------------------------------------
def _spans(R, entry, start, stop, score, first_read):
    """single end: one read per span, its only record is the span (ref_start / ref_end = the row's ref_begin / ref_end)"""
    start = np.asarray(start, dtype=np.int64)
    n = len(start)
    R.add(first_read + np.arange(n), entry, start, 0, score, start, stop)
    return first_read + n


def _dense_entry(n):
    """n spans: equal starts in twos, chains of ~50 spans broken by a jump, scores 120 .. 200"""
    k = np.arange(n)
    start = 7 * (k // 2) + 600 * (k // 50)
    return start, start + 60 + (k * 37) % 40, 120 + (k * 11) % 81


def _chain_probe(p, join, far):
    """p + 3 spans 1000 apart, 100 long (every one a chain of its own); the span at sorted index p starts exactly at
    reach - 20 (joins) or reach - 19 (starts a chain); far: the reach is the stop of span 2, not of the predecessor"""
    k = np.arange(p + 3)
    start, stop = 1000 * k, 1000 * k + 100
    reach = stop[p - 1]
    if far:
        stop[2] = reach = 1000 * p + 500
    start[p] = reach - (CHAIN_SLACK if join else CHAIN_SLACK - 1)
    stop[p] = start[p] + 100
    return start, stop, 150 + k % 30


def cases_e():
    out = []
    R = Rows()
    nxt = _spans(R, 3, *_dense_entry(PSEUDO_CAP), 0)
    nxt = _spans(R, 8, *_dense_entry(PSEUDO_CAP + 1), nxt)
    nxt = _spans(R, 5, *_dense_entry(10), nxt)
    out.append(_case("E-4000-and-4001-spans", R, nxt, {"spans_largest_entry": PSEUDO_CAP + 1, "spans_second_entry": PSEUDO_CAP},
                     paired=False, stages=7))
    R = Rows()                    # the longest entry exactly at the cap: LDS for 4000 spans, no second launch
    nxt = _spans(R, 3, *_dense_entry(PSEUDO_CAP), 0)
    nxt = _spans(R, 9, *_dense_entry(70), nxt)
    out.append(_case("E-4000-spans-longest", R, nxt, {"spans_largest_entry": PSEUDO_CAP, "spans_second_entry": 70}, paired=False, stages=7))
    for n, dev in ((300, True), (301, False)):
        R = Rows()
        nxt = _spans(R, 2, *_dense_entry(n), 0)
        nxt = _spans(R, 4, *_dense_entry(n - 1), nxt)
        out.append(_case("E-cap300-longest-%d" % n, R, nxt, {"spans_largest_entry": n}, paired=False, stages=7, pseudo_cap=300, on_device=dev))
    for far in (False, True):
        for p in ((255, 256, 257) if far else (5, 63, 64, 65)):
            for join in (True, False):
                R = Rows()
                start, stop, score = _chain_probe(p, join, far)
                nxt = _spans(R, 1, start, stop, score, 0)
                chains = (p + 3) - (p - 3 if far else 0) - int(join)
                out.append(_case("E-chain-%s-at%d-%s" % ("far" if far else "near", p, "joins" if join else "starts"), R, nxt,
                                 dict({"spans_largest_entry": p + 3, "chains_largest_entry": chains, "probe_index": p, "probe_joins": int(join)},
                                      **({"reach_setter_index": 2, "steps_between_setter_and_probe": p // 64} if far else
                                         {"reach_setter_index": p - 1})), paired=False, stages=7))
    R = Rows()
    nxt = _spans(R, 0, [100], [199], [150], 0)                                 # a chain of one: the score stays
    nxt = _spans(R, 1, [100, 150], [199, 249], [150, 170], nxt)                # a chain of two
    nxt = _spans(R, 2, [100, 150], [200, 150], [150, 170], nxt)                # a zero-length span: x / 0
    nxt = _spans(R, 3, [100, 150], [200, 120], [150, 170], nxt)                # a reversed one
    nxt = _spans(R, 4, [100, 100], [100, 100], [150, 170], nxt)                # two zero-length chains of one
    out.append(_case("E-chains-of-1-and-2-degenerate-spans", R, nxt, {"spans_largest_entry": 2, "zero_scores_out": 2}, paired=False, stages=7))
    R = Rows()
    k = np.arange(300)
    nxt = _spans(R, 6, np.full(300, 5000), 5050 + (k * 37) % 90, 120 + (k * 11) % 81, 0)
    nxt = _spans(R, 7, 5000 + k // 100, 5050 + (k * 41) % 90, 120 + (k * 7) % 81, nxt)
    out.append(_case("E-equal-starts", R, nxt, {"spans_largest_entry": 300, "distinct_starts_entry6": 1}, paired=False, stages=7))
    for top in (0, 255, 256, 65535, 65536):
        R = Rows()
        nxt = 0
        for e in sorted({0, top // 2, top}):
            nxt = _spans(R, e, [100, 150, 900], [199, 249, 999], [150, 170, 190], nxt)
        out.append(_case("E-largest-entry-%d" % top, R, nxt, {"largest_entry": top}, paired=False, stages=7))
    # the second screen.  Reads 0, 1: the same span 100 .. 200 on entry 2, a chain of two -> coverage 2 x average 2.0 per base x
    # length 100 = 400 (exact in double).  Read 0
    # also has rows on entries 1 (score 200 = 400 x 0.5: stays) and 3 (199: goes); read 2: two rows no chain touches
    R = Rows()
    R.add([0, 0, 0, 1, 2, 2], [1, 2, 3, 2, 5, 6], 100, 0, [200, 200, 199, 200, 200, 150], 100, 200)
    out.append(_case("E-second-screen-bar-equality", R, 3, {"pairs_before_second_screen": 6, "pairs_out": 5, "top_score_out": 400},
                     paired=False, frac=0.5, stages=7))
    R = Rows()
    R.add([0, 0, 1], [1, 2, 2], 100, 0, [200, 200, 100], 100, 200)      # the chain scores 2 x 1.5 x 100 = 300: 200 < 0.7 x 300 goes
    out.append(_case("E-second-screen-shrinks", R, 2, {"pairs_before_second_screen": 3, "pairs_out": 2, "top_score_out": 300},
                     paired=False, frac=0.7, stages=7))
    # paired: alignment pairs of three read pairs overlap along one entry
    R = Rows()
    R.pair(np.arange(3), 3, 4, 1000 + 40 * np.arange(3), 300, 100, 90)
    R.pair(np.arange(3), 3, 6, 9000 * (1 + np.arange(3)), 300, 100, 80)
    out.append(_case("E-paired-chain-of-three", R, 6, {"spans_largest_entry": 3, "pairs_out": 3}, stages=7))
    return out


def all_cases():
    return {"A": cases_a(), "B": cases_b(), "C": cases_c(), "D": cases_d(), "E": cases_e()}
