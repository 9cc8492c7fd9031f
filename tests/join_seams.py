"""Synthetic cases for the join hooks (kslam_debug_join / kslam_debug_overlap_unique), every seam of
k-slam_amd/csrc/join.hip placed on purpose, and the functions that say where a case's seams lie (numpy only).

tests/test_join_ref.py checks, without a GPU, that every named seam is present in its case -- so that a later change of
a constant cannot turn a seam test into a plain test unnoticed; tests/test_gpu_join_seams.py runs the cases.
Keys are synthetic, never DNA.  A case is a dict; the read records of a join case are ordered by their top
`sorted_top_bits` key bits (what the merge route needs; the probe does not care) and in no order below them.
"""
import numpy as np

import join_ref as R

# ---- the constants of k-slam_amd/csrc/join.hip this file places seams at ---------------------------------------------
JOIN_TILE = 1024        # common.h: constexpr int JOIN_TILE = 1024
JB = 256                # join.hip: constexpr int JB = 256                      threads per block
JI = JOIN_TILE // JB    # join.hip: constexpr int JI = JOIN_TILE / JB           records per thread
SMALL_BUCKET = 16       # join.hip, find_run: if (hi - lo <= 16u)               two batches of eight loads, else binary search
BIG = 48                # join.hip: constexpr uint32_t BIG = 48                 longer runs go through the block's queue
BIGQ = 64               # join.hip: constexpr int BIGQ = 64                     entries of that queue
FLAT_MAX = 4096         # join.hip: constexpr uint32_t FLAT_MAX = 4096          block totals up to this take the flat route
MP = 4096               # join.hip: constexpr uint32_t MP = 4096                keys per piece of the merge
RUN_STEPS = 4           # join.hip, k_join_merge: while (c < 4 && ...)          a run's end: 4 steps, then a second search
GROUP_CAP = 64          # join.hip: constexpr uint32_t GROUP_CAP = 64           keys of a (read, entry) group k_group_order takes
GROUP_BLOCK = 256       # join.hip, k_group_order: base = blockIdx.x * 256      keys whose groups a block owns
WAVE = 64

U64 = np.uint64
LAYOUT = (15, 10, 21, 512)          # the plain cases: reads < 2^15, entries < 2^10, genome offsets < 2^20, reads <= 512 bases


def bucket_base(b, bits):
    return U64(b) << U64(64 - bits)


def _meta(ids, rc, gb):
    return (np.asarray(ids, dtype=np.uint32) & np.uint32(R.ID_MASK)) | (np.asarray(rc, dtype=np.uint32) << np.uint32(30)) | \
        np.uint32(0x80000000 if gb else 0)


def genome_records(keys, rng, layout=LAYOUT):
    """sorted keys -> records with random entry ids, strands and offsets the layout holds"""
    keys = np.sort(np.asarray(keys, dtype=U64))
    n = len(keys)
    g = np.zeros(n, dtype=R.KMER_DT)
    g["kmer"] = keys
    g["meta"] = _meta(rng.integers(0, 1 << layout[1], n), rng.integers(0, 2, n), True)
    g["offset"] = rng.integers(0, (1 << layout[2]) - 2 * layout[3], n)
    return g


def read_records(keys, rng, sorted_top_bits, layout=LAYOUT, n_reads=777, keep_order=False):
    """read keys -> (records, read_len): random ids, strands, lengths of 32 .. rel_bias bases and offsets inside the read;
    ordered by the top sorted_top_bits key bits only (shuffled below them) unless keep_order"""
    keys = np.asarray(keys, dtype=U64)
    n = len(keys)
    if not keep_order and n:
        keys = keys[rng.permutation(n)]
        keys = keys[np.argsort(keys >> U64(64 - sorted_top_bits), kind="stable")]
    n_reads = min(n_reads, 1 << layout[0])
    read_len = rng.integers(R.K, layout[3] + 1, n_reads).astype(np.uint32)
    r = np.zeros(n, dtype=R.KMER_DT)
    r["kmer"] = keys
    ids = rng.integers(0, n_reads, n)
    r["meta"] = _meta(ids, rng.integers(0, 2, n), False)
    r["offset"] = (rng.random(n) * (read_len[ids] - R.K + 1)).astype(np.uint32)
    edge = rng.integers(0, 4, n)                       # a quarter each at the read's first and last k-mer
    r["offset"] = np.where(edge == 0, 0, np.where(edge == 1, read_len[ids] - R.K, r["offset"]))
    return r, read_len


def join_case(name, gkeys, rkeys, seed, bucket_bits=8, sorted_top_bits=None, layout=LAYOUT, keep_order=False, **extra):
    rng = np.random.default_rng(seed)
    stb = bucket_bits if sorted_top_bits is None else sorted_top_bits
    g = genome_records(gkeys, rng, layout)
    r, read_len = read_records(rkeys, rng, stb, layout, keep_order=keep_order)
    c = {"name": name, "genome": g, "reads": r, "read_len": read_len, "bucket_bits": bucket_bits, "sorted_top_bits": stb,
         "layout": layout}
    c.update(extra)
    return c


def _distinct(rng, n, lo=1, hi=1 << 64):
    """n distinct keys in [lo, hi), ascending"""
    out = np.unique(rng.integers(lo, hi, n + n // 8 + 8, dtype=U64))
    while len(out) < n:
        out = np.unique(np.concatenate([out, rng.integers(lo, hi, n, dtype=U64)]))
    return np.sort(out[rng.permutation(len(out))[:n]])


def _in_bucket(b, bits, size, fill=False):
    """`size` keys of bucket b: distinct with room between them, or (fill) one key `size` times"""
    base = bucket_base(b, bits) + U64(1000)
    if fill:
        return np.full(size, base + U64(4), dtype=U64)
    return base + U64(4) * np.arange(size, dtype=U64)


# ---- where a join case's seams lie --------------------------------------------------------------------------------
def bucket_sizes(c):
    return np.diff(R.bucket_table(c["genome"]["kmer"], c["bucket_bits"]).astype(np.int64))


def tile_totals(c):
    """overlaps per tile of JOIN_TILE consecutive read records"""
    cnt = R.run_counts(c["genome"], c["reads"])
    return [int(cnt[t:t + JOIN_TILE].sum()) for t in range(0, len(cnt), JOIN_TILE)]


def tile_long_runs(c):
    """read records per tile whose run is longer than BIG"""
    cnt = R.run_counts(c["genome"], c["reads"])
    return [int((cnt[t:t + JOIN_TILE] > BIG).sum()) for t in range(0, len(cnt), JOIN_TILE)]


def merge_ranges(c):
    """per tile: (start, end) of the key range k_join_merge streams, before it rounds the start down"""
    bits = c["bucket_bits"]
    gb = min(c["sorted_top_bits"], bits)
    table = R.bucket_table(c["genome"]["kmer"], bits).astype(np.int64)
    k = c["reads"]["kmer"]
    out = []
    for t in range(0, len(k), JOIN_TILE):
        a, z = int(k[t]) >> (64 - gb), int(k[min(t + JOIN_TILE, len(k)) - 1]) >> (64 - gb)
        out.append((int(table[a << (bits - gb)]), int(table[(z + 1) << (bits - gb)])))
    return out


def piece_index_of_runs(c):
    """for every read record with a hit: (index of its run's first key in the piece it starts in ... as the offset from
    the tile's rounded-down range start, run length)"""
    runs = R.genome_runs(c["genome"])
    rng_of = merge_ranges(c)
    out = set()
    for i, k in enumerate(c["reads"]["kmer"].tolist()):
        if k and k in runs:
            lo, cnt = runs[k]
            out.add((lo - (rng_of[i // JOIN_TILE][0] & ~1), cnt))
    return out


# ---- join cases ---------------------------------------------------------------------------------------------------
def _hits_and_misses(rng, gkeys, n_r, frac=0.6):
    n_hit = int(n_r * frac) if len(gkeys) else 0
    hits = np.asarray(gkeys, dtype=U64)[rng.integers(0, max(len(gkeys), 1), n_hit)] if n_hit else np.zeros(0, dtype=U64)
    return np.concatenate([hits, rng.integers(1, 1 << 64, n_r - n_hit, dtype=U64)])


def count_cases():
    out = []
    for n_r in (1, 255, 256, 257, 1023, 1024, 1025, 2049):
        rng = np.random.default_rng(100 + n_r)
        gk = np.repeat(_distinct(rng, 500), rng.integers(1, 4, 500))
        out.append(join_case("n_r=%d" % n_r, gk, _hits_and_misses(rng, gk, n_r), n_r))
    for n_g in (0, 1, 2):
        rng = np.random.default_rng(200 + n_g)
        gk = _distinct(rng, n_g)
        rk = np.concatenate([np.repeat(gk, 5), rng.integers(1, 1 << 64, 300, dtype=U64)])
        out.append(join_case("n_g=%d" % n_g, gk, rk, 210 + n_g))
    rng = np.random.default_rng(220)
    gk = _distinct(rng, 3000)
    out.append(join_case("no_hit", gk, gk[rng.integers(0, 3000, 1500)] + U64(1), 221, no_hit=True))
    return out


BUCKET_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 40, 3000]


def bucket_cases():
    """every bucket size, in the first bucket, the last bucket and between long stretches of empty buckets; read keys below,
    above, between, on the first and on the last key of each bucket; `fill`: every bucket one run of equal keys"""
    out = []
    for bits in (8, 12):
        nb = 1 << bits
        for rot in (0, 6, 7):          # first / last bucket of 0 / 3000, 16 / 15 and 17 / 16 keys
            for fill in (False, True):
                sizes = BUCKET_SIZES[rot:] + BUCKET_SIZES[:rot]
                where = [0] + [nb // 3 + 2 * j for j in range(len(sizes) - 2)] + [nb - 1]     # first, a cluster, last
                gk, rk = [], []
                for b, s in zip(where, sizes):
                    ks = _in_bucket(b, bits, s, fill)
                    gk.append(ks)
                    base = bucket_base(b, bits)
                    if s == 0:
                        rk += [base + U64(1000), base + U64(1), base + U64(77)]
                        continue
                    rk += [ks[0] - U64(1), ks[-1] + U64(1), ks[0], ks[-1], ks[s // 2], ks[0], ks[-1]]
                    if not fill and s > 1:
                        rk += [ks[0] + U64(2), ks[-2] + U64(1), ks[s // 2] + U64(3)]
                rk += [bucket_base(5, bits) + U64(9), bucket_base(nb - 2, bits) + U64(9)]     # in the empty stretches
                name = "buckets/bits%d/rot%d/%s" % (bits, rot, "fill" if fill else "distinct")
                out.append(join_case(name, np.concatenate(gk), np.array(rk, dtype=U64), 300 + bits + rot, bucket_bits=bits,
                                     want_sizes=sorted(set(BUCKET_SIZES)), first_last=(sizes[0], sizes[-1])))
    return out


ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)


def edge_key_cases():
    out = []
    rng = np.random.default_rng(400)
    gk = np.concatenate([np.zeros(3, dtype=U64), _distinct(rng, 200)])
    rk = np.concatenate([np.zeros(5, dtype=U64), gk[3:40], gk[3:10]])
    out.append(join_case("key_zero", gk, rk, 401, zero=True))
    for ones in (1, 2, 5):
        for n_g in (ones, 10, 11, 4097, 4098):
            if n_g < ones:
                continue
            rng = np.random.default_rng(410 + ones + n_g)
            gk = np.concatenate([_distinct(rng, n_g - ones, hi=(1 << 64) - 1), np.full(ones, ALL_ONES)])
            rk = np.concatenate([np.full(3, ALL_ONES), gk[:20], [ALL_ONES - U64(1)]])
            out.append(join_case("all_ones/x%d/n_g=%d" % (ones, n_g), gk, rk, 420 + n_g, ones=ones))
    return out


RUN_LENGTHS = [1, 4, 5, 6, 48, 49, 5000]


def run_length_case():
    rng = np.random.default_rng(500)
    heads = _distinct(rng, len(RUN_LENGTHS))
    gk = np.concatenate([np.repeat(heads, RUN_LENGTHS), _distinct(rng, 700)])
    rk = np.concatenate([np.repeat(heads, 3), rng.integers(1, 1 << 64, 900, dtype=U64), heads + U64(1)])
    return join_case("run_lengths", gk, rk, 501, run_lengths=RUN_LENGTHS)


def block_total_cases():
    """tile 0 built for its block total; tile 1 a plain tile behind it (higher keys)"""
    out = []
    b = 40
    k4, k5, k49, k5000 = (bucket_base(b, 8) + U64(x) for x in (100, 200, 300, 400))
    base_g = np.concatenate([np.full(4, k4), np.full(5, k5), np.full(49, k49), np.full(5000, k5000)])
    rng = np.random.default_rng(600)
    tail_g = _distinct(rng, 400, lo=int(bucket_base(b + 1, 8)))
    tail_r = np.sort(np.concatenate([tail_g[:200], tail_g[:100] + U64(1)]))
    miss = bucket_base(b, 8) + U64(7)
    tiles = {"flat_4096": (np.full(JOIN_TILE, k4), FLAT_MAX, 0),
             "per_thread_4097": (np.concatenate([np.full(JOIN_TILE - 1, k4), [k5]]), FLAT_MAX + 1, 0),
             "queue_overflow": (np.concatenate([np.full(70, k49), np.full(JOIN_TILE - 70, k4)]), 70 * 49 + 954 * 4, 70),
             "one_run_of_5000": (np.concatenate([[k5000], np.full(JOIN_TILE - 1, miss)]), 5000, 1)}
    for i, (name, (tile, total, long_runs)) in enumerate(tiles.items()):
        rng = np.random.default_rng(610 + i)
        rk = np.concatenate([tile[rng.permutation(JOIN_TILE)], tail_r])
        out.append(join_case("block_total/" + name, np.concatenate([base_g, tail_g]), rk, 620 + i, keep_order=True,
                             tile0_total=total, tile0_long_runs=long_runs))
    return out


def strand_offset_case():
    """all four strand combinations, the first and the last k-mer of reads of different lengths, rel + rel_bias at 0 and at
    2^bits_rel - 1, entry and read ids at the top of their fields"""
    bits_read, bits_entry, bits_rel = 12, 30, 15
    n_reads = 1 << bits_read
    read_len = (32 + (np.arange(n_reads) * 7) % 200).astype(np.uint32)
    read_len[n_reads - 1] = 231                                        # the longest: rel_bias = its last offset
    read_len[0] = 32
    bias = int(read_len.max()) - R.K
    layout = (bits_read, bits_entry, bits_rel, bias)
    top_e, top_off = (1 << bits_entry) - 1, (1 << bits_rel) - 1 - bias
    keys = [U64(0x1111 << 48), U64(0x2222 << 48), U64(0x3333 << 48), U64(0x4444 << 48)]
    g = np.zeros(8, dtype=R.KMER_DT)
    # per key: a forward and a reverse genome record; offsets 0 and the largest the rel field takes
    g["kmer"] = np.repeat(keys, 2)
    g["meta"] = _meta([top_e, 0, 5, top_e, top_e, 1, 7, top_e], [0, 1, 0, 1, 0, 1, 0, 1], True)
    g["offset"] = [0, 0, top_off, top_off, 0, top_off, top_off, 0]
    recs = []
    for k in keys:
        for rid in (0, 1, 77, n_reads - 1):
            L = int(read_len[rid])
            for rrc in (0, 1):
                for roff in sorted({0, L - R.K, (L - R.K) // 2}):
                    recs.append((k, rid | (rrc << 30), roff))
    r = np.array(recs, dtype=R.KMER_DT)
    return {"name": "strand_offset", "genome": g, "reads": r, "read_len": read_len, "bucket_bits": 8, "sorted_top_bits": 8,
            "layout": layout, "rel_extremes": (0, (1 << bits_rel) - 1), "top_ids": (n_reads - 1, top_e)}


def join_cases():
    return count_cases() + bucket_cases() + edge_key_cases() + [run_length_case()] + block_total_cases() + [strand_offset_case()]


# ---- merge only -------------------------------------------------------------------------------------------------------
def sorted_bits_cases():
    """keys that share their top sorted_top_bits bits three hundred ways, so that the shuffle below those bits shows"""
    out = []
    for stb, bits in ((8, 8), (8, 12), (16, 12), (16, 16), (24, 8), (24, 16)):
        rng = np.random.default_rng(700 + stb + bits)
        tops = _distinct(rng, min(300, 1 << (stb - 1)), lo=0, hi=1 << stb) << U64(64 - stb)
        low = lambda n: rng.integers(1, 1 << (64 - stb), n, dtype=U64)
        gk = np.repeat(tops[rng.integers(0, len(tops), 4000)] | low(4000), rng.integers(1, 4, 4000))
        rk = np.concatenate([gk[rng.integers(0, len(gk), 1800)], tops[rng.integers(0, len(tops), 1200)] | low(1200)])
        out.append(join_case("sorted_top_bits=%d/bits%d" % (stb, bits), gk, rk, 710 + stb + bits, bucket_bits=bits, sorted_top_bits=stb))
    return out


RANGE_LENGTHS = [0, 1, MP - 1, MP, MP + 1, 2 * MP + 1]


def range_cases():
    """one tile whose reads all lie in bucket 41, of `length` keys; the bucket before it holds 7 or 8 keys, so the tile's
    key range starts at an odd or an even index"""
    out = []
    for length in RANGE_LENGTHS:
        for before in (7, 8):
            rng = np.random.default_rng(800 + length + before)
            b = 41
            ks = bucket_base(b, 8) + U64(1000) + U64(4) * np.arange(length, dtype=U64)
            gk = np.concatenate([_in_bucket(b - 1, 8, before), ks, _in_bucket(b + 3, 8, 5)])
            rk = [bucket_base(b, 8) + U64(5), bucket_base(b, 8) + U64(999)]
            if length:
                at = [0, length - 1, length // 2] + [x for x in (MP - 2, MP - 1, MP, MP + 1, 2 * MP - 1, 2 * MP) if x < length]
                rk += [ks[x] for x in at] + [ks[x] + U64(1) for x in at] + list(ks[rng.integers(0, length, 200)])
            out.append(join_case("range/len%d/start_%s" % (length, "odd" if before & 1 else "even"), gk, np.array(rk, dtype=U64),
                                 810 + length + before, range_len=length, range_start=before))
    return out


PIECE_STARTS = [MP - 2, MP - 1, MP]
PIECE_RUNS = [1, 2, 3, 4, 5, 6, MP + 4]


def piece_cases():
    """a run of equal keys that starts at a chosen index of the first piece (the tile's range starts at the even index 8)"""
    out = []
    for start in PIECE_STARTS:
        for run in PIECE_RUNS:
            rng = np.random.default_rng(900 + start + run)
            b = 41
            before = bucket_base(b, 8) + U64(1000) + U64(4) * np.arange(start, dtype=U64)
            key = before[-1] + U64(4)
            after = key + U64(4) * np.arange(1, 40, dtype=U64)
            gk = np.concatenate([_in_bucket(b - 1, 8, 8), before, np.full(run, key), after])
            rk = np.concatenate([[key] * 3, [key - U64(4), key - U64(1), key + U64(1), key + U64(4)], before[rng.integers(0, start, 100)], after[:5]])
            out.append(join_case("piece/start%d/run%d" % (start, run), gk, rk, 910 + start + run, piece_run=(start, run)))
    return out


def column_end_cases():
    """a run that is exactly the last keys of the column"""
    out = []
    for run in (1, 3, 5, MP + 4):
        for n_g in (run + 100, run + 101, run + 2 * MP, run + 2 * MP + 1):
            rng = np.random.default_rng(1000 + run + n_g)
            key = bucket_base(255, 8) + U64(12345)
            gk = np.concatenate([_distinct(rng, n_g - run, lo=int(bucket_base(250, 8)), hi=int(key)), np.full(run, key)])
            rk = np.concatenate([[key] * 3, [key - U64(1), key + U64(1)], gk[rng.integers(0, n_g, 150)]])
            out.append(join_case("column_end/run%d/n_g=%d" % (run, n_g), gk, rk, 1010 + run + n_g, end_run=run))
    return out


def wide_tile_case():
    rng = np.random.default_rng(1100)
    gk = np.concatenate([[U64(5)], _distinct(rng, 9000), [ALL_ONES - U64(3)]])
    rk = np.concatenate([[U64(5), ALL_ONES - U64(3)], _hits_and_misses(rng, gk, JOIN_TILE - 2)])
    return join_case("wide_tile", gk, rk, 1101, wide=True)


def merge_cases():
    return sorted_bits_cases() + range_cases() + piece_cases() + column_end_cases() + [wide_tile_case()]


# ---- unique cases -----------------------------------------------------------------------------------------------------
UNIQUE_LAYOUTS = [(10, 8, 15, 300), (20, 22, 20, 0), (5, 30, 27, (1 << 27) - 1)]         # 34, 63 and 63 bits wide


def _pack_all(read, entry, relb, rc, layout):
    _br, be, bl, _bias = layout
    return (np.asarray(read, dtype=U64) << U64(be + bl + 1)) | (np.asarray(entry, dtype=U64) << U64(bl + 1)) | \
        (np.asarray(relb, dtype=U64) << U64(1)) | np.asarray(rc, dtype=U64)


def _chain(steps, start=0):
    return start + np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)


def unique_sorted_cases():
    """(name, layout, fully sorted keys) for route 0; rel values below are BIASED (the field's content)"""
    out = []
    for li, lay in enumerate(UNIQUE_LAYOUTS):
        br, be, bl, _bias = lay
        top_r, top_e, top_rel = (1 << br) - 1, (1 << be) - 1, (1 << bl) - 1
        tag = "rel%d/" % bl

        def add(name, read, entry, relb, rc=None, seed=0):
            rng = np.random.default_rng(seed + li)
            relb = np.asarray(relb, dtype=np.int64)
            assert relb.min() >= 0 and relb.max() <= top_rel, name
            rc = rng.integers(0, 2, len(relb)) if rc is None else rc
            out.append((tag + name, lay, np.sort(_pack_all(np.broadcast_to(read, relb.shape), np.broadcast_to(entry, relb.shape), relb, rc, lay))))

        for n in (1, 255, 256, 257):
            rng = np.random.default_rng(1200 + n)
            add("n=%d" % n, top_r, 3, _chain(rng.integers(0, 5, n - 1), 7), seed=n)
        for step in (0, 1, 2, 3, 4):
            add("step%d" % step, 1, top_e, _chain(np.full(299, step), 11), seed=step)
        add("chain_by_2", 2, 2, _chain(np.full(999, 2)), rc=np.zeros(1000, dtype=np.int64))
        add("chain_by_1", 2, 2, _chain(np.full(999, 1)), rc=np.zeros(1000, dtype=np.int64))
        add("step2_then_gap3", 0, 0, _chain(np.tile([2, 3], 300)))
        add("two_2s_then_gap3", 0, 0, _chain(np.tile([2, 2, 3], 200)))
        # equal rel across a change of entry and across a change of read: both kept
        add("equal_rel_across_groups", np.repeat([4, 4, 5, 5], 3), np.repeat([1, 2, 2, 3], 3), np.tile([50, 51, 52], 4))
        add("identical_200", 3, 3, np.full(200, 99), rc=np.zeros(200, dtype=np.int64))
        # 255 equal keys (one survivor in lane 0, then waves without any) and a new key in lane 63 of the fourth wave
        add("survivor_in_lane_63", np.concatenate([np.full(255, 3), np.full(70, 4)]), 3, np.full(325, 99), rc=np.zeros(325, dtype=np.int64))
        add("rel_field_edges", 1, 1, np.concatenate([[0, 0, 1, 2, 3, 4], top_rel - np.array([7, 4, 3, 2, 1, 0, 0])]))
        rng = np.random.default_rng(1300 + li)
        n = 3000
        add("random", rng.integers(0, min(top_r, 40) + 1, n), rng.integers(0, min(top_e, 3) + 1, n), rng.integers(0, min(top_rel, 60) + 1, n), seed=77)
    return out


def keep_flags_by_wave(keys, layout):
    f = R.unique_flags(keys, layout)
    pad = (-len(f)) % WAVE
    return np.concatenate([f, np.zeros(pad, dtype=bool)]).reshape(-1, WAVE)


def shuffle_low(keys, layout, rng):
    """the keys ordered by the bits above rel and revComp only: every (read, entry) group shuffled"""
    keys = np.sort(np.asarray(keys, dtype=U64))
    hi = keys >> U64(layout[2] + 1)
    edges = np.flatnonzero(np.concatenate([[True], hi[1:] != hi[:-1], [True]]))
    out = keys.copy()
    for a, z in zip(edges[:-1], edges[1:]):
        out[a:z] = keys[a:z][rng.permutation(z - a)]
    return out


def group_sizes(keys, layout):
    """(start, size) of every (read, entry) group of keys ordered by their high bits"""
    hi = np.asarray(keys, dtype=U64) >> U64(layout[2] + 1)
    edges = np.flatnonzero(np.concatenate([[True], hi[1:] != hi[:-1], [True]]))
    return [(int(a), int(z - a)) for a, z in zip(edges[:-1], edges[1:])]


GROUPED = {  # name -> the sizes of the groups, in order
    "sizes_1_2_3_63_64": [1, 2, 3, 63, 64, 1, 64, 63, 3, 2, 1],
    "size_65": [1, 2, 65, 3],
    "g64_lane0": [64, 1, 1],
    "g64_lane0_block1": [1] * 256 + [64, 2],
    "g64_lane255": [1] * 255 + [64, 2],
    "g64_lane255_is_the_end": [1] * 255 + [64],
    "g65_lane255": [1] * 255 + [65, 2],
    "g64_straddles": [1] * 230 + [64, 3],
    "n_mod_256=0": [3] * 169 + [5],
    "n_mod_256=1": [3] * 169 + [6],
    "n_mod_256=255": [3] * 169 + [4],
    "many_64s": [64] * 9,
}


def unique_grouped_cases():
    """(name, layout, keys ordered by their high bits only) for route 1"""
    out = []
    for li, lay in enumerate(UNIQUE_LAYOUTS):
        br, be, bl, _bias = lay
        top_rel = (1 << bl) - 1
        for name, sizes in GROUPED.items():
            rng = np.random.default_rng(1400 + li + len(sizes))
            keys = []
            for gi, s in enumerate(sizes):
                start = int(rng.integers(0, top_rel - 5 * s))
                if gi % 7 == 3:
                    start = top_rel - 4 * (s - 1)                                  # may reach the field's end
                relb = _chain(rng.integers(0, 5, s - 1), start)
                g_id = gi + 1                                                      # (read, entry) ascending, never 0 / 0
                keys.append(_pack_all(np.full(s, g_id >> be if be < 20 else 0), np.full(s, g_id & ((1 << be) - 1) if be < 20 else g_id),
                                      relb, rng.integers(0, 2, s), lay))
            out.append(("rel%d/%s" % (bl, name), lay, shuffle_low(np.concatenate(keys), lay, rng)))
        for s in (3, 64):      # ONE group of read 0 / entry 0: the tile's zero padding looks like more of it
            rng = np.random.default_rng(1500 + li + s)
            relb = _chain(rng.integers(0, 4, s - 1), 0)
            out.append(("rel%d/zero_group_of_%d" % (bl, s), lay, shuffle_low(_pack_all(np.zeros(s), np.zeros(s), relb, rng.integers(0, 2, s), lay), lay, rng)))
    return out
