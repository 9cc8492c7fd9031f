"""The depth track of include/kslam_depth.h, restated in plain Python from the header's text: a difference array per entry with
one slot more than the entry has bases, its running sum, and runs cut at the entry's end.  The cases the host twin and the
device are held to are built with tests/variants_ref.py's Builder / random_case / concat.  Shares no code with host/depth.cpp.

table(case, min_depth) -> (rows as (entry, start, end, depth) tuples, stats dict)."""
import numpy as np

import variants_ref as V
from coverage_ref import NO_OVERLAP

STAT_NAMES = ("n_records", "n_skipped", "n_intervals", "n_keys", "n_rows", "covered_bases", "max_depth")
ROW_DT = np.dtype([("entry", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])


# ---------------------------------------------------------------- the definition

def _intervals(o, case, memo):
    """one overlap record -> None when it is skipped, else its closed M intervals [(begin, end)]"""
    key = (int(o["read"]), int(o["entry"]), int(o["ref_begin"]), int(o["query_begin"]), int(o["cigar_off"]), int(o["cigar_len"]))
    if key in memo:
        return memo[key]
    read, entry, ref_begin, query_begin, cigar_off, cigar_len = key
    goff, roff = case["goff"], case["roff"]
    out = None
    if entry < len(goff) - 1 and cigar_len > 0 and ref_begin >= 0:
        ref_len, read_len = int(goff[entry + 1]) - int(goff[entry]), int(roff[read + 1]) - int(roff[read])
        ops = [(int(c) >> 4, int(c) & 15) for c in case["pool"][cigar_off:cigar_off + cigar_len]]
        rp, qp, fits = ref_begin, max(query_begin, 0), True
        for n, op in ops:      # the whole CIGAR first
            if op == 0:
                rp, qp = rp + n, qp + n
            elif op == 1:
                qp += n
            elif op == 2:
                rp += n
            if rp > ref_len or qp > read_len:
                fits = False
                break
        if fits:
            out, rp = [], ref_begin
            for n, op in ops:
                if op == 0:
                    if n > 0:
                        out.append((rp, rp + n - 1))
                    rp += n
                elif op == 2:
                    rp += n
    memo[key] = out
    return out


def named(case):
    got = set()
    for g in case["rp"]:
        live = case["pr"][int(g["first"]):int(g["first"]) + int(g["count"])]   # the records behind first + count are dead
        for f in ("r1", "r2"):
            got.update(int(i) for i in live[f] if int(i) != NO_OVERLAP)
    return got


def profile(case):
    """-> (per entry: the depth at every base as an int64 array, stats with the first four counts filled)"""
    n_entries = len(case["goff"]) - 1
    diff = [np.zeros(int(case["goff"][e + 1]) - int(case["goff"][e]) + 1, dtype=np.int64) for e in range(n_entries)]
    stats = dict.fromkeys(STAT_NAMES, 0)
    memo = {}
    for i in sorted(named(case)):      # each contributes once, however many live pairs name it
        stats["n_records"] += 1
        o = case["ov"][i]
        got = _intervals(o, case, memo)
        if got is None:
            stats["n_skipped"] += 1
            continue
        for b, t in got:
            diff[int(o["entry"])][b] += 1
            diff[int(o["entry"])][t + 1] -= 1
        stats["n_intervals"] += len(got)
    stats["n_keys"] = int(sum(np.count_nonzero(d) for d in diff))   # the distinct boundaries whose begins and ends do not cancel
    return [np.cumsum(d)[:-1] for d in diff], stats


def table(case, min_depth=1):
    depth, stats = profile(case)
    floor = max(int(min_depth), 1)      # 0 is read as 1
    rows = []
    for e, d in enumerate(depth):
        if not len(d):
            continue
        cut = (np.nonzero(np.diff(d))[0] + 1).tolist()       # a run ends where the depth changes -- and at the entry's end
        for s, t in zip([0] + cut, cut + [len(d)]):
            v = int(d[s])
            if v > 0:
                stats["n_rows"] += 1
                stats["covered_bases"] += t - s
                stats["max_depth"] = max(stats["max_depth"], v)
                if v >= floor:
                    rows.append((e, s, t, v))
    return rows, stats


def fields(rows):
    return [(int(r["entry"]), int(r["start"]), int(r["end"]), int(r["depth"])) for r in rows]


def as_array(rows):
    return np.array(rows, dtype=ROW_DT) if len(rows) else np.zeros(0, dtype=ROW_DT)


def bedgraph_bytes(rows, loci):
    return b"".join(b"%s\t%d\t%d\t%d\n" % (loci[e], s, t, v) for e, s, t, v in rows)


# ---------------------------------------------------------------- the cases

def _entries(rng, lens):
    return [V.random_bases(rng, n) for n in lens]


def interval_case(name, lens, intervals, seed=1):
    """entries of these lengths, one record of one M run per (entry, begin, end) -- end inclusive"""
    b = V.Builder(name, _entries(np.random.default_rng(seed), lens))
    for e, s, t in intervals:
        b.single(b.aligned(e, s, [(t - s + 1, "M")], (s + t) & 1))
    return b.done()


def cigar_case(name, ref_begin, ops, length=60):
    b = V.Builder(name, _entries(np.random.default_rng(7), [length]))
    b.single(b.aligned(0, ref_begin, ops, 0))
    return b.done()


def boundaries(name, n):
    """exactly n distinct boundaries (n >= 2): one-base intervals three apart, and for an odd n [0, 0] under [0, 1] in front"""
    b = V.Builder(name, _entries(np.random.default_rng(n), [3 * (n // 2) + 8]))
    read, cig = b.read(b.entries[0][:1]), b.cigar([(1, "M")])
    at, left = 0, n
    if n & 1:
        b.single(b.rec(read, 0, 0, cig))
        b.single(b.rec(b.read(b.entries[0][:2]), 0, 0, b.cigar([(2, "M")])))
        at, left = 4, n - 3
    for k in range(left // 2):
        b.single(b.rec(read, 0, at + 3 * k, cig))
    return b.done()


# name -> (case, expected rows at min_depth 1, expected n_skipped): written by hand
def seam_cases():
    out = {}

    def add(case, rows, skipped=0):
        out[case["name"]] = (case, rows, skipped)

    # ---- the walk
    add(cigar_case("m-only", 5, [(40, "M")]), [(0, 5, 45, 1)])
    add(cigar_case("m-i-d-mix", 2, [(10, "M"), (2, "I"), (5, "M"), (3, "D"), (4, "M")]), [(0, 2, 17, 1), (0, 20, 24, 1)])
    add(cigar_case("m-of-one", 0, [(1, "M"), (1, "D"), (1, "M"), (1, "I"), (1, "M")]), [(0, 0, 1, 1), (0, 2, 4, 1)])
    add(cigar_case("zero-m", 10, [(5, "M"), (0, "M"), (2, "I"), (0, "M"), (5, "M"), (2, "D"), (0, "M"), (3, "M")]), [(0, 10, 20, 1), (0, 22, 25, 1)])
    add(cigar_case("leading-i", 7, [(3, "I"), (5, "M")]), [(0, 7, 12, 1)])
    add(cigar_case("d-after-first-m", 3, [(1, "M"), (2, "D"), (5, "M")]), [(0, 3, 4, 1), (0, 6, 11, 1)])
    b = V.Builder("every-skip-rule", _entries(np.random.default_rng(3), [100, 100]))
    b.single(b.aligned(0, 60, [(40, "M")], 0))                    # ends exactly at the entry's end: valid
    for r in V.invalid_kinds(b, 0):
        b.single(r)
    add(b.done(), [(0, 60, 100, 1)], 7)
    b = V.Builder("all-skipped", _entries(np.random.default_rng(4), [100]))
    for r in V.invalid_kinds(b, 0):
        b.single(r)
    add(b.done(), [], 7)
    # ---- entry seams
    add(interval_case("first-base", [10, 10], [(0, 0, 3)]), [(0, 0, 4, 1)])
    add(interval_case("last-base-of-all", [10, 10], [(1, 5, 9)]), [(1, 5, 10, 1)])
    add(interval_case("seam", [10, 10], [(0, 6, 9), (1, 0, 3)]), [(0, 6, 10, 1), (1, 0, 4, 1)])             # two rows, not (.., 6, 14, 1)
    add(interval_case("seam-over-one", [10, 1, 10], [(0, 6, 9), (2, 0, 3)]), [(0, 6, 10, 1), (2, 0, 4, 1)])
    add(interval_case("seam-one-covered", [10, 1, 10], [(0, 6, 9), (1, 0, 0), (2, 0, 3)]), [(0, 6, 10, 1), (1, 0, 1, 1), (2, 0, 4, 1)])
    add(interval_case("whole-entries", [4, 1, 5], [(0, 0, 3), (1, 0, 0), (1, 0, 0), (2, 0, 4)]), [(0, 0, 4, 1), (1, 0, 1, 2), (2, 0, 5, 1)])
    # ---- runs
    add(interval_case("abutting", [40], [(0, 10, 19), (0, 20, 29)]), [(0, 10, 30, 1)])
    add(interval_case("overlapping", [40], [(0, 0, 9), (0, 5, 14)]), [(0, 0, 5, 1), (0, 5, 10, 2), (0, 10, 15, 1)])
    add(interval_case("nested", [40], [(0, 0, 29), (0, 5, 24), (0, 10, 19)]),
        [(0, 0, 5, 1), (0, 5, 10, 2), (0, 10, 20, 3), (0, 20, 25, 2), (0, 25, 30, 1)])
    # the depth returns to 2 behind a stretch of 1 that neither 2 touches
    add(interval_case("returns", [40], [(0, 0, 30), (0, 2, 8), (0, 12, 18)]), [(0, 0, 2, 1), (0, 2, 9, 2), (0, 9, 12, 1), (0, 12, 19, 2), (0, 19, 31, 1)])
    add(V.repeated("identical-70001", 70001), [(0, 10, 30, 70001)])      # a 16-bit counter would wrap
    return out


TILES = (256, 1024, 4096)      # the walk's and the row pass's block, the 64-bit scan's tile, scan.hip's SCAN_TILE


def tile_cases():
    out = []
    for t in TILES:
        for n in (t - 1, t, t + 1):
            out.append(V.repeated("records-%d" % n, n))
            out.append(boundaries("boundaries-%d" % n, n))
    return out


def filter_case():
    """depths 1, 2, 3, 2, 1 side by side"""
    return interval_case("filter", [40], [(0, 0, 29), (0, 5, 24), (0, 10, 19)])


def random_cases():
    a = V.random_case("a", 71, 900, 7, 300)
    ents = [a["gbases"][int(a["goff"][e]):int(a["goff"][e + 1])].tobytes() for e in range(7)]
    b = V.random_case("b", 72, 3000, 7, entries=ents)
    return a, b, ents
