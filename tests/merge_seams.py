"""Cases and a plain reference for the seams of the shard merge, split and export (k-slam_amd/csrc/merge.hip, driven from
csrc/api_multi.hip, host/comm.cpp and dist.py).  Pure numpy: tests/test_merge_seams.py holds every case to the reference and
to kslam_amd.dist.reassemble on the CPU and shows that the case list can see each plausible kernel mistake;
tests/test_gpu_merge_seams.py runs the same cases through the device.

THE ORACLE IS CONSTRUCTION.  Every case starts from a batch-GLOBAL table -- what one context returns for the whole batch:
rows sorted by (read, entry, rel), read ids in block layout (R1 of pair p is p, R2 is n_pairs + p), the CIGAR pool in row
order, cigar_off the exclusive scan of cigar_len and 0 where cigar_len == 0.  split_batch cuts that table into per-shard
results in LOCAL terms (local read ids [R1 of its pairs | R2 of its pairs], its own pool in its own row order, local offsets).
Whatever a device path makes of the shards must be the table the case started from, byte for byte; no reference code sits
between the input and the expectation.  Every pass-through field carries a row-unique pattern, so a misplaced 16-byte piece
shows; the pads stay 0.

counts_ref, export_ref and merge_ref state the contract of the three entry points once more, slowly and obviously.

A case is a dict: name, n_pairs, bounds [(pair_lo, pair_hi) per shard], rows, pool (the global table), junk {shard: words
behind its pool that no row refers to}, and for the one-shard cases pool_bases (pool_base_r1, pool_base_r2 - n_cigar_r1):
what the export adds to the CIGAR offsets of its R1 / R2 rows, as if other shards' ops came first."""
import numpy as np

# copies of the sizes in csrc/merge.hip and csrc/common.h (test_merge_seams.py compares them with the source text)
WALK = 256            # k_shard_first_cigar: rows a step
MAX_SHARDS = 256      # MERGE_MAX_SHARDS
BLOCK = 256           # threads a block in k_export_rows / k_merge_rows
WAVE = 64
PIECES = 3            # 16-byte pieces a record
MAX_PAIRS = 1 << 31   # n_pairs, n_local_pairs stay below
JUNK_WORD = 0xDEADBEEF

OVERLAP_DT = np.dtype([("read", "<u4"), ("entry", "<u4"), ("rel", "<i4"), ("revcomp", "u1"), ("pad", "u1"), ("score", "<u2"),
                       ("ref_begin", "<i4"), ("ref_end", "<i4"), ("query_begin", "<i4"), ("query_end", "<i4"),
                       ("cigar_len", "<u4"), ("pad2", "<u4"), ("cigar_off", "<u8")])
PASS_THROUGH = ("entry", "rel", "revcomp", "score", "ref_begin", "ref_end", "query_begin", "query_end", "cigar_len")


def _scan(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, dtype=np.int64)


def row_ops(pool, off, lens):
    """the ops rows address, row after row"""
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, dtype=np.uint32)
    within = np.arange(total, dtype=np.int64) - np.repeat(_scan(lens), lens)
    return pool[np.repeat(off, lens) + within]


def make_table(reads, lens, seed):
    """the batch-global table for rows with these (sorted) read ids and CIGAR lengths"""
    reads, lens = np.asarray(reads, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(reads)
    assert len(lens) == n and (np.diff(reads) >= 0).all()
    i = np.arange(n, dtype=np.int64)
    first = np.ones(n, dtype=bool)
    first[1:] = reads[1:] != reads[:-1]
    rank = i - np.maximum.accumulate(np.where(first, i, 0))          # the row's place among the rows of its read
    h = (i * 2654435761 + seed * 40503 + 12345) & 0xFFFFFFFF
    rows = np.zeros(n, dtype=OVERLAP_DT)
    rows["read"] = reads
    rows["entry"] = rank * 4099 + (h >> 20) % 4099                     # grows with the rank: sorted by (read, entry, rel)
    rows["rel"] = seed * 7919 + i * 37 - 50000                         # row-unique: piece 0
    rows["revcomp"] = h & 1
    rows["score"] = (h >> 7) & 0xFFFF
    rows["ref_begin"] = seed + 1 + 3 * i                               # row-unique: piece 1
    rows["ref_end"] = rows["ref_begin"] + 100 + (h >> 3) % 50
    rows["query_begin"] = (h >> 11) % 40
    rows["query_end"] = 60 + (h >> 17) % 90
    rows["cigar_len"] = lens
    off = _scan(lens)
    rows["cigar_off"] = np.where(lens > 0, off, 0)
    total = int(lens.sum())
    within = np.arange(total, dtype=np.int64) - np.repeat(off, lens)
    pool = (((seed & 0x7F) << 24) | ((np.repeat(i, lens) + 1) << 12) | within).astype(np.uint32)   # word-unique
    return rows, pool


def split_batch(rows, pool, bounds, n_pairs):
    """the global table -> [(rows, pool) per shard] in the shard's local terms"""
    read = rows["read"].astype(np.int64)
    out = []
    for lo, hi in bounds:
        mine = rows[((read >= lo) & (read < hi)) | ((read >= n_pairs + lo) & (read < n_pairs + hi))].copy()
        r = mine["read"].astype(np.int64)
        mine["read"] = np.where(r < n_pairs, r - lo, r - n_pairs - lo + (hi - lo))
        lens = mine["cigar_len"].astype(np.int64)
        ops = row_ops(pool, mine["cigar_off"].astype(np.int64), lens)
        mine["cigar_off"] = np.where(lens > 0, _scan(lens), 0)
        out.append((mine, ops))
    return out


# ---- the contract, slowly ------------------------------------------------------------------------------------------------
def counts_ref(rows, n_local_pairs):
    """kslam_shard_counts_device -> (n_rows, n_rows_r1, n_cigar, n_cigar_r1)"""
    n_r1 = n_cigar = n_cigar_r1 = 0
    for read, ln in zip(rows["read"].tolist(), rows["cigar_len"].tolist()):
        n_cigar += ln
        if read < n_local_pairs:
            n_r1 += 1
            n_cigar_r1 += ln
    return len(rows), n_r1, n_cigar, n_cigar_r1


def export_ref(rows, pool, n_local_pairs, pair_lo, n_pairs_total, pool_base_r1, pool_base_r2):
    """kslam_export_shard_device -> (rows of R1, rows of R2, pool of R1, pool of R2), the rows in batch terms"""
    _, n_r1, _, c1 = counts_ref(rows, n_local_pairs)
    out = rows.copy()
    for k in range(len(rows)):
        read, off, ln = int(rows["read"][k]), int(rows["cigar_off"][k]), int(rows["cigar_len"][k])
        if read < n_local_pairs:
            out["read"][k] = pair_lo + read
            out["cigar_off"][k] = pool_base_r1 + off if ln else 0
        else:
            out["read"][k] = n_pairs_total + pair_lo + (read - n_local_pairs)
            out["cigar_off"][k] = pool_base_r2 + (off - c1) if ln else 0
    return out[:n_r1], out[n_r1:], pool[:c1].copy(), pool[c1:].copy()


def merge_ref(shards, bounds, n_pairs):
    """kslam_merge_shards_device: [(rows, pool) per shard, local terms] -> the batch-global (rows, pool)"""
    blocks = ([], [])                                    # (the row, its ops) of the R1 rows, of the R2 rows
    for (rows, pool), (lo, hi) in zip(shards, bounds):
        n_loc = hi - lo
        for k in range(len(rows)):
            row = rows[k:k + 1].copy()
            read, off, ln = int(row["read"][0]), int(row["cigar_off"][0]), int(row["cigar_len"][0])
            r2 = read >= n_loc
            row["read"] = n_pairs + lo + (read - n_loc) if r2 else lo + read
            blocks[r2].append((row, pool[off:off + ln] if ln else pool[:0]))
    out, ops = [], []
    at = 0
    for row, o in blocks[0] + blocks[1]:
        row["cigar_off"] = at if len(o) else 0
        at += len(o)
        out.append(row)
        ops.append(o)
    return (np.concatenate(out) if out else np.zeros(0, dtype=OVERLAP_DT),
            np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, dtype=np.uint32))


# ---- what a case says about itself -----------------------------------------------------------------------------------------
def shards_of(case):
    """[(rows, pool) per shard] in local terms, the junk words behind the pools that have some"""
    parts = split_batch(case["rows"], case["pool"], case["bounds"], case["n_pairs"])
    return [(r, np.concatenate([p, np.full(case["junk"].get(s, 0), JUNK_WORD, dtype=np.uint32)])) for s, (r, p) in enumerate(parts)]


def gathered(case):
    """what the collecting device holds: (rows back to back, pools back to back, [(pair_lo, pair_hi, n_rows, n_cigar)])"""
    parts = shards_of(case)
    rows = np.concatenate([r for r, _ in parts]) if parts else np.zeros(0, dtype=OVERLAP_DT)
    pool = np.concatenate([p for _, p in parts]) if parts else np.zeros(0, dtype=np.uint32)
    return rows, pool, [(lo, hi, len(r), len(p)) for (lo, hi), (r, p) in zip(case["bounds"], parts)]


def counts_of(case, s=0):
    """the 4-tuple of shard s by construction: its rows are the global rows in its two id ranges"""
    lo, hi = case["bounds"][s]
    read, lens = case["rows"]["read"].astype(np.int64), case["rows"]["cigar_len"].astype(np.int64)
    m1 = (read >= lo) & (read < hi)
    m2 = (read >= case["n_pairs"] + lo) & (read < case["n_pairs"] + hi)
    return int(m1.sum() + m2.sum()), int(m1.sum()), int(lens[m1].sum() + lens[m2].sum()) + case["junk"].get(s, 0), int(lens[m1].sum())


def exported(case):
    """what the export of a one-shard case must write: the global table cut at the split, the CIGAR offsets moved by the
    case's pool bases -> (rows of R1, rows of R2, pool of R1, pool of R2, pool_base_r1, pool_base_r2)"""
    assert len(case["bounds"]) == 1 and not case["junk"]
    _, n_r1, _, c1 = counts_of(case)
    add1, add2 = case["pool_bases"]
    rows = case["rows"].copy()
    has = rows["cigar_len"] > 0
    side = np.arange(len(rows)) < n_r1
    rows["cigar_off"] = np.where(has, rows["cigar_off"] + np.where(side, np.uint64(add1), np.uint64(add2)), np.uint64(0))
    return rows[:n_r1], rows[n_r1:], case["pool"][:c1], case["pool"][c1:], add1, add2 + c1


# ---- builders --------------------------------------------------------------------------------------------------------------
MIX = (2, 0, 1, 0, 0, 3)


def cyc(pattern, n, shift=0):
    """n CIGAR lengths, the pattern over and over"""
    return np.roll(np.resize(np.asarray(pattern, dtype=np.int64), max(n, 1)), -shift)[:n] if n else np.zeros(0, dtype=np.int64)


def shard(lo, hi, lens1, lens2, junk=0):
    """a shard of pairs [lo, hi) with len(lens1) R1 rows and len(lens2) R2 rows, spread over its pairs in order (several rows a
    read where there are more rows than pairs)"""
    lens1, lens2 = np.asarray(lens1, dtype=np.int64), np.asarray(lens2, dtype=np.int64)
    assert hi > lo or (len(lens1) == 0 and len(lens2) == 0)
    return {"lo": lo, "hi": hi, "lens1": lens1, "lens2": lens2, "junk": junk}


def build(name, n_pairs, shards, seed, pool_bases=(0, 0)):
    reads, lens = [], []
    for which, base in (("lens1", 0), ("lens2", n_pairs)):
        for sh in shards:
            k, n_loc = len(sh[which]), sh["hi"] - sh["lo"]
            reads.append(base + sh["lo"] + ((np.arange(k, dtype=np.int64) + 1) * n_loc - 1) // max(k, 1))   # the last row on the last pair
            lens.append(sh[which])
    rows, pool = make_table(np.concatenate(reads) if reads else [], np.concatenate(lens) if lens else [], seed)
    return {"name": name, "n_pairs": n_pairs, "bounds": [(sh["lo"], sh["hi"]) for sh in shards], "rows": rows, "pool": pool,
            "junk": {s: sh["junk"] for s, sh in enumerate(shards) if sh["junk"]}, "pool_bases": pool_bases}


def one(name, lens1, lens2, seed, n_loc=None, lo=5, behind=3, pool_bases=(7, 1000)):
    """one shard of a larger batch: pairs [lo, lo + n_loc) of lo + n_loc + behind"""
    if n_loc is None:
        n_loc = max(len(lens1), len(lens2), 1) // 2 + 2         # more rows than pairs: some reads have two rows
    return build(name, lo + n_loc + behind, [shard(lo, lo + n_loc, lens1, lens2)], seed, pool_bases)


WALK_DISTANCES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)


def cases_split():
    """S: k_shard_split's binary search at its ends, k_shard_first_cigar beyond its first step"""
    out, seed = [one("n0_pairs0", [], [], 1, n_loc=0)], 2
    for n in (0, 1, 2, 255, 256, 257):
        for n_r1 in sorted({0, 1, n - 1, n} & set(range(n + 1))):
            lens = cyc(MIX, n, seed)
            out.append(one("n%d_r1_%d" % (n, n_r1), lens[:n_r1], lens[n_r1:], seed))
            seed += 1
    for d in WALK_DISTANCES:
        for r1 in (0, 1):
            # d R2 rows without a CIGAR, then the first with one; four rows behind it, so that the last step of the walk ends
            # beyond the rows for every d but 251
            out.append(one("walk_d%d_r1cig%d" % (d, r1), cyc((2, 0, 1, 3, 0), 5) * r1, np.concatenate([np.zeros(d), [4, 0, 2, 1, 0]]), seed))
            seed += 1
    out.append(one("walk_none_r2_300", cyc(MIX, 10), np.zeros(300), seed))         # R2 rows, none with a CIGAR: ~0 -> n_cigar
    out.append(one("walk_none_r2_256", cyc(MIX, 10), np.zeros(256), seed + 1))
    out.append(one("walk_none_r2_1", cyc(MIX, 10), np.zeros(1), seed + 2))
    out.append(one("no_cigar_anywhere", np.zeros(100), np.zeros(200), seed + 3))
    out.append(one("walk_last_step_1_row", cyc(MIX, 3), np.concatenate([np.zeros(256), [5]]), seed + 4))
    return out


EXPORT_SPLITS = (0, 1, 21, 22, 85, 86, 171, 200)     # 3 * n_r1 = 0, 3, 63, 66, 255, 258, 513, 600


def cases_export():
    """X: everything in S, and a wave of k_export_rows that straddles the split; offsets that carry into the high word; read ids
    up to 2^32 - 3"""
    out, seed = cases_split(), 200
    for n_r1 in EXPORT_SPLITS:
        lens = cyc(MIX, 200, seed)
        out.append(one("x_r1_%d_of_200" % n_r1, lens[:n_r1], lens[n_r1:], seed))
        seed += 1
    lens = cyc((2, 0, 1, 0, 0, 3), 60)
    c1 = int(lens[:22].sum())
    hi_bases = ((1 << 32) - 3, (1 << 33) + (1 << 32) - 1 - c1)
    out.append(one("x_high_word_bases", lens[:22], lens[22:], seed, pool_bases=hi_bases))
    top = MAX_PAIRS - 1
    out.append(one("x_read_ids_to_2p32", lens[:22], lens[22:], seed + 1, n_loc=40, lo=top - 40, behind=0))
    out.append(one("x_high_word_bases_read_ids_to_2p32", lens[:22], lens[22:], seed + 2, n_loc=40, lo=top - 40, behind=0, pool_bases=hi_bases))
    out.append(one("x_r1_only_high_word", lens, [], seed + 3, pool_bases=hi_bases))
    out.append(one("x_r2_only_high_word", [], lens, seed + 4, pool_bases=hi_bases))
    return out


def _real(lo, n_loc, n1, n2, k, pattern=MIX, junk=0):
    return shard(lo, lo + n_loc, cyc(pattern, n1, k), cyc(pattern, n2, k + 1), junk)


def _with_empties(real, where, count, kinds):
    """`real` shards (pair ranges laid end to end from pair 0, 10 pairs apart) with `count` empty shards at the front, in the
    middle or at the end; kind "norows": a pair range without rows, "norange": an empty pair range"""
    seq = list(real)
    at = {"front": 0, "middle": len(real) // 2, "end": len(real)}[where]
    seq[at:at] = [kinds[k % len(kinds)] for k in range(count)]
    shards, lo = [], 0
    for k, s in enumerate(seq):
        if s == "norange":
            shards.append(shard(lo, lo, [], []))
        elif s == "norows":
            shards.append(shard(lo, lo + 2, [], []))
            lo += 2
        else:
            n_loc, n1, n2 = s
            shards.append(_real(lo, n_loc, n1, n2, k))
            lo += n_loc
    return shards, lo


def cases_merge():
    """M: the shard lookup of k_merge_rows with empty shards, at block edges and beyond 8 shards; k_merge_plan's search at its
    ends; k_merge_cigars with rows without a CIGAR between rows with one, a long CIGAR, words no row refers to"""
    out = []
    real = [(40, 70, 50), (30, 33, 61), (50, 90, 20)]
    out.append(build("m1", 150, [_real(0, 150, 140, 160, 0)], 301))
    out.append(build("m2", 100, [_real(0, 45, 70, 50, 0), _real(45, 55, 33, 61, 1)], 302))
    sh, n = _with_empties(real, "front", 0, ())
    out.append(build("m3", n, sh, 303))
    seed = 304
    for where in ("front", "middle", "end"):
        for kind in ("norows", "norange"):
            sh, n = _with_empties(real, where, 1, (kind,))
            out.append(build("m3_empty_%s_%s" % (where, kind), n, sh, seed))
            seed += 1
        sh, n = _with_empties(real, where, 100, ("norows", "norange", "norange"))
        out.append(build("m3_100_empty_%s" % where, n, sh, seed))
        seed += 1
    out.append(build("m3_gaps", 200, [_real(3, 37, 70, 50, 0), _real(50, 40, 33, 61, 1), _real(100, 60, 90, 20, 2)], seed))
    # shard boundaries at rows 255, 256, 257 and 512 of the gathered array
    out.append(build("m_rows_255_256_257_512", 400, [_real(0, 100, 200, 55, 0), _real(100, 1, 1, 0, 1), _real(101, 1, 0, 1, 2),
                                                      _real(102, 100, 100, 155, 3), _real(202, 100, 30, 30, 4)], seed + 1))
    out.append(build("m_r1_only_r2_only_single_rows", 300, [_real(0, 60, 50, 0, 0), _real(60, 60, 0, 50, 1), _real(120, 1, 1, 0, 2),
                                                             _real(121, 1, 0, 1, 3), _real(122, 100, 40, 45, 4), _real(222, 1, 1, 1, 5)], seed + 2))
    out.append(build("m_cigar_0_1_300", 90, [_real(0, 30, 20, 17, 0, (0, 1, 300, 0, 300, 1)), _real(30, 30, 19, 23, 1, (300, 0, 0, 1)),
                                              _real(60, 30, 21, 18, 2, (0, 1, 300, 0, 300, 1))], seed + 3))
    out.append(build("m_junk_5_words", 150, [_real(0, 40, 70, 50, 0, junk=5), _real(40, 30, 33, 61, 1), _real(70, 50, 90, 20, 2, junk=5),
                                              _real(120, 30, 10, 10, 3)], seed + 4))
    out.append(build("m_junk_on_rows_without_cigar", 60, [shard(0, 20, np.zeros(9), np.zeros(8), junk=5), _real(20, 20, 12, 13, 1),
                                                           shard(40, 60, np.zeros(4), [1, 0, 2])], seed + 5))
    for n_sh in (255, 256):
        # two pairs a shard; 0 .. 3 rows, R1 only / R2 only / both / none in turn
        shapes = ((1, 1), (0, 0), (2, 0), (0, 3), (1, 2), (0, 0), (0, 0), (3, 1))
        out.append(build("m%d" % n_sh, 2 * n_sh, [_real(2 * k, 2, shapes[k % 8][0], shapes[k % 8][1], k) for k in range(n_sh)], seed + n_sh))
    out.append(build("m_all_empty_3", 30, [shard(0, 10, [], []), shard(10, 10, [], []), shard(10, 30, [], [])], 1))
    out.append(build("m_all_empty_1", 30, [shard(0, 30, [], [])], 1))
    return out


# the M cases with three or more shards that have rows of both blocks, run through the export protocol as well
EQUIVALENCE = ("m3", "m3_gaps", "m3_empty_middle_norows", "m3_empty_front_norange", "m_r1_only_r2_only_single_rows", "m_cigar_0_1_300",
               "m_rows_255_256_257_512")


def refusals():
    """(name, shards [(pair_lo, pair_hi, n_rows, n_cigar)], n_pairs, which buffers are null, what the message says)"""
    ok = (0, 10, 4, 6)
    return [("no_shards", [], 100, (), "shards"),
            ("257_shards", [(k, k + 1, 0, 0) for k in range(MAX_SHARDS + 1)], 1000, (), "shards"),
            ("pair_hi_beyond_n_pairs", [ok, (10, 101, 2, 0)], 100, (), "pair range"),
            ("pair_hi_below_pair_lo", [ok, (20, 19, 2, 0)], 100, (), "pair range"),
            ("out_of_batch_order", [(10, 20, 2, 0), ok], 100, (), "order"),
            ("overlapping_ranges", [ok, (9, 20, 2, 0)], 100, (), "order"),
            ("null_rows_in", [ok], 100, ("rows_in",), "null"),
            ("null_rows_out", [ok], 100, ("rows_out",), "null"),
            ("null_pool_in", [ok], 100, ("pool_in",), "null"),
            ("null_pool_out", [ok], 100, ("pool_out",), "null")]


def all_cases():
    return {"S": cases_split(), "X": cases_export(), "M": cases_merge()}
