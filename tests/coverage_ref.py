"""The coverage table of include/kslam_coverage.h, restated in plain Python from the header's text (a numpy boolean array per
entry), and the builder of the cases the host twin and the device are held to.  Shares no code with host/coverage.cpp.

A case is a dict: name, lengths (of the entries), ov / rp / pr (the overlap records, read pairs and alignment-pair records as
structured arrays laid out like kslam_overlap, kslam_read_pair and kslam_paired_overlap)."""
import numpy as np

NO_OVERLAP = 0xFFFFFFFF
MARK_BLOCK = 256   # csrc/common.h: COV_MARK_BLOCK, the mark pass's workgroup
OVERLAP_DT = np.dtype([("read", "<u4"), ("entry", "<u4"), ("rel", "<i4"), ("revcomp", "u1"), ("pad", "u1"), ("score", "<u2"),
                       ("ref_begin", "<i4"), ("ref_end", "<i4"), ("query_begin", "<i4"), ("query_end", "<i4"),
                       ("cigar_len", "<u4"), ("pad2", "<u4"), ("cigar_off", "<u8")])
PAIRED_OVERLAP_DT = np.dtype([("combined_score", "<u4"), ("entry", "<u4"), ("ref_start", "<i4"), ("ref_end", "<i4"),
                              ("insert_size", "<u4"), ("r1", "<u4"), ("r2", "<u4"), ("pad", "<u4")])
READ_PAIR_DT = np.dtype([("r1_read", "<u4"), ("r2_read", "<u4"), ("first", "<u8"), ("count", "<u8")])
ROW_DT = np.dtype([("alignments", "<u8"), ("unique_read_pairs", "<u8"), ("aligned_bases", "<u8"), ("covered_bases", "<u8")])
HEADER = b"#entry\tlocus\ttaxid\tlength\talignments\tunique_read_pairs\taligned_bases\tcovered_bases\tbreadth\tmean_depth\n"


# ---------------------------------------------------------------- the definition

def table(lengths, ov, rp, pr):
    """-> (rows [ROW_DT, one per entry], n_skipped, covered [one boolean array per entry])"""
    n = len(lengths)
    rows = np.zeros(n, dtype=ROW_DT)
    covered = [np.zeros(int(l), dtype=bool) for l in lengths]
    skipped = 0
    for g in rp:
        live = pr[int(g["first"]):int(g["first"]) + int(g["count"])]   # the records behind first + count are dead
        entries = set()
        for p in live:
            entries.add(int(p["entry"]))
            if p["entry"] < n:
                rows[int(p["entry"])]["alignments"] += 1
            for idx in (int(p["r1"]), int(p["r2"])):
                if idx == NO_OVERLAP:
                    continue
                o = ov[idx]
                e, b, t = int(o["entry"]), int(o["ref_begin"]), int(o["ref_end"])
                if e >= n or b < 0 or t < b or t >= int(lengths[e]):
                    skipped += 1
                    continue
                rows[e]["aligned_bases"] += t - b + 1
                covered[e][b:t + 1] = True   # closed interval
        if len(live) and len(entries) == 1 and min(entries) < n:
            rows[min(entries)]["unique_read_pairs"] += 1
    for e in range(n):
        rows[e]["covered_bases"] = int(covered[e].sum())
    return rows, skipped, covered


def words(bits):
    """a boolean array -> its ceil(len / 64) 64-bit words, bit b of word w = position 64 w + b"""
    n_words = (len(bits) + 63) // 64
    padded = np.zeros(n_words * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded.reshape(n_words, 64), axis=1, bitorder="little").view("<u8").reshape(n_words) if n_words else np.zeros(0, dtype=np.uint64)


def report(rows, lengths, loci, taxids):
    """the report's bytes, formatted here"""
    out = [HEADER]
    for e, r in enumerate(rows):
        if int(r["alignments"]) == 0:
            continue
        length = int(lengths[e])
        breadth = int(r["covered_bases"]) / length if length else 0.0
        depth = int(r["aligned_bases"]) / length if length else 0.0
        out.append(b"%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (e, loci[e], int(taxids[e]), length, int(r["alignments"]), int(r["unique_read_pairs"]),
                                                              int(r["aligned_bases"]), int(r["covered_bases"]), b"%.6f" % breadth, b"%.4f" % depth))
    return b"".join(out)


# ---------------------------------------------------------------- the cases

def build(name, lengths, groups, single=False):
    """groups: a list of (live, dead) record lists; a record is (pair_entry, mate1, mate2), a mate (entry, ref_begin, ref_end) or
    None.  The dead records follow the live ones in the pairs array, as device pseudo-assembly leaves them."""
    ov, pr, rp = [], [], []
    n_groups = len(groups)
    for g, (live, dead) in enumerate(groups):
        rp.append((g, 0 if single else n_groups + g, len(pr), len(live)))
        for pe, m1, m2 in list(live) + list(dead):
            idx = []
            for m in (m1, m2):
                if m is None:
                    idx.append(NO_OVERLAP)
                else:
                    idx.append(len(ov))
                    ov.append((m[0], m[1], m[2]))
            pr.append((pe, idx[0], idx[1]))
    return arrays(name, lengths, ov, rp, pr)


def arrays(name, lengths, ov, rp, pr):
    a = np.zeros(len(ov), dtype=OVERLAP_DT)
    if len(ov):
        t = np.asarray(ov, dtype=np.int64).reshape(-1, 3)
        a["entry"], a["ref_begin"], a["ref_end"] = t[:, 0], t[:, 1], t[:, 2]
        a["read"] = np.arange(len(ov)) % 7
        a["score"] = 60
    p = np.zeros(len(pr), dtype=PAIRED_OVERLAP_DT)
    if len(pr):
        t = np.asarray(pr, dtype=np.int64).reshape(-1, 3)
        p["entry"], p["r1"], p["r2"] = t[:, 0], t[:, 1], t[:, 2]
        p["combined_score"] = 100
    r = np.zeros(len(rp), dtype=READ_PAIR_DT)
    if len(rp):
        t = np.asarray(rp, dtype=np.int64).reshape(-1, 4)
        r["r1_read"], r["r2_read"], r["first"], r["count"] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    return {"name": name, "lengths": np.asarray(lengths, dtype=np.uint64), "ov": a, "rp": r, "pr": p}


def _one(e, b, t):
    return (e, (e, b, t), None)


BIT_SEAMS = [(0, 0), (63, 63), (63, 64), (64, 64), (0, 63), (0, 64), (1, 62), (64, 127), (5, 199), (199, 199)]
ENTRY_SEAM_LENGTHS = [1, 63, 64, 65, 128, 129]


def random_case(name, seed, n_pairs, n_entries, max_len, invalid=True, max_group=6, lengths=None):
    """n_pairs alignment-pair records (live and dead) in groups of random size over entries of random lengths 1..max_len"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, max_len + 1, n_entries) if lengths is None else np.asarray(lengths)
    ov, pr, rp = [], [], []
    while len(pr) < n_pairs:
        size = int(min(rng.integers(1, max_group + 1), n_pairs - len(pr)))
        live = int(rng.integers(0, size + 1)) if rng.random() < 0.3 else size
        home = int(rng.integers(0, n_entries))
        rp.append((len(rp), len(rp) + 1000000, len(pr), live))
        for _ in range(size):
            pe = home if rng.random() < 0.85 else int(rng.integers(0, n_entries + (2 if invalid else 0)))
            idx = []
            for m in range(2):
                if rng.random() < 0.15 and (m == 0 or idx[0] != NO_OVERLAP):
                    idx.append(NO_OVERLAP)
                    continue
                e = pe if rng.random() < 0.9 and pe < n_entries else int(rng.integers(0, n_entries))
                length = int(lengths[e])
                b = int(rng.integers(0, length))
                t = min(length - 1, b + int(rng.integers(0, 300)))
                if invalid and rng.random() < 0.03:
                    kind = int(rng.integers(0, 4))
                    if kind == 0:
                        e = n_entries + int(rng.integers(0, 3))
                    elif kind == 1:
                        b = -1 - int(rng.integers(0, 5))
                    elif kind == 2:
                        b, t = t + 1, b
                    else:
                        t = length + int(rng.integers(0, 3))
                idx.append(len(ov))
                ov.append((e, b, t))
            pr.append((pe, idx[0], idx[1]))
    return arrays(name, lengths, ov, rp, pr)


def cases():
    out = []
    # ---- bit seams: an entry of length 200, each interval alone and all together
    for b, t in BIT_SEAMS:
        out.append(build("bits-%d-%d" % (b, t), [200], [([_one(0, b, t)], [])]))
    out.append(build("bits-all", [200], [([_one(0, b, t)], []) for b, t in BIT_SEAMS]))
    # ---- entry seams: entries side by side, every second one covered whole (the last entry of the index among them)
    for odd in (0, 1):
        live = [_one(e, 0, l - 1) for e, l in enumerate(ENTRY_SEAM_LENGTHS) if e % 2 == odd]
        out.append(build("entries-%s" % ("odd" if odd else "even"), ENTRY_SEAM_LENGTHS, [([r], []) for r in live]))
    # ---- contention: 20 000 alignment pairs, r1 always [10, 159], r2 inside word 1 at different offsets
    out.append(build("contention", [400], [([(0, (0, 10, 159), (0, 64 + k % 32, 96 + k % 31))], []) for k in range(20000)]))
    # ---- dead records: they point at entry 3, which nothing else touches
    dead = _one(3, 0, 49)
    out.append(build("dead", [100, 100, 100, 100], [
        ([_one(0, 0, 9)], [dead, dead]),                      # count smaller than the gap to the next first
        ([], [dead]),                                         # count == 0
        ([_one(1, 5, 20), _one(1, 30, 40)], []),
        ([_one(2, 1, 2)], [dead, dead, dead])]))              # the last group with a dead tail
    # ---- mates
    out.append(build("mates", [300, 300], [
        ([(0, (0, 10, 59), None)], []), ([(0, None, (0, 100, 149))], []), ([(0, (0, 160, 199), (0, 220, 259))], []),
        ([(1, (1, 10, 100), (1, 60, 150))], [])]))            # mates that overlap: the union in covered, both in aligned
    out.append(build("single-end", [300, 300], [([_one(0, 10, 59)], []), ([_one(1, 0, 299), _one(0, 50, 70)], [])], single=True))
    # ---- unique read pairs
    big = [_one(1, (7 * k) % 900, (7 * k) % 900 + 99) for k in range(5000)]
    out.append(build("unique", [1000, 1000, 1000], [
        ([_one(0, 0, 9), _one(0, 5, 14)], []),                # all on one entry
        ([_one(0, 20, 29), _one(2, 20, 29)], []),             # two entries: neither gets it
        ([_one(2, 40, 49), _one(2, 45, 60)], [_one(0, 0, 9)]),   # one entry once the dead record is ignored
        (big, []),                                            # 5 000 live records on one entry
        (big[:-1] + [_one(0, 100, 120)], [])]))               # the same with the last record elsewhere
    # ---- skipped mates, one of each kind among valid ones
    out.append(build("skipped", [100, 50], [
        ([_one(0, 0, 99)], []),                               # ends exactly at length - 1: valid
        ([(0, (0, 10, 100), (0, 10, 20))], []),               # ends at length: skipped, its mate is not
        ([(1, (2, 0, 5), (1, 0, 5))], []),                    # entry >= n_entries
        ([(1, (1, -1, 5), None)], []),                        # ref_begin < 0
        ([(1, (1, 30, 29), (1, 49, 49))], []),                # ref_end < ref_begin
        ([(5, (1, 10, 19), None)], [])]))                     # the pair's own entry outside: no row, the mate still counts
    # ---- long intervals: the wavefront's path
    longs = []
    for span in (600, 4000, 4033):
        for off in (0, 1, 63):
            longs.append(([_one(0, 128 + off, 128 + off + span - 1)], []))
    for k, g in enumerate(longs):
        out.append(build("long-%d" % k, [10000], [g]))
    out.append(build("long-all", [10000, 70], longs + [([_one(1, 3, 66)], [])]))
    # ---- grid seams
    out.append(random_case("grid-70001", 4242, 70001, 300, 5000))
    for n in (0, 1, MARK_BLOCK - 1, MARK_BLOCK + 1):
        out.append(random_case("grid-%d" % n, 100 + n, n, 5, 700, invalid=False))
    return out


def concat(a, b):
    """two cases over the same entries as one batch"""
    ov = np.concatenate([a["ov"], b["ov"]])
    pr2, rp2 = b["pr"].copy(), b["rp"].copy()
    for f in ("r1", "r2"):
        keep = pr2[f] != NO_OVERLAP
        pr2[f][keep] += len(a["ov"])
    rp2["first"] += len(a["pr"])
    return {"name": a["name"] + "+" + b["name"], "lengths": a["lengths"], "ov": ov, "rp": np.concatenate([a["rp"], rp2]),
            "pr": np.concatenate([a["pr"], pr2])}
