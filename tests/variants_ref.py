"""The SNV table of include/kslam_variants.h, restated in plain Python from the header's text (a dictionary of sites and a
difference array of depth per entry), the builder of the cases the host twin and the device are held to, a writer of the VCF
bytes and a strict reader of them.  Shares no code with host/variants.cpp.

A case is a dict: name, gbases / goff (the entries' bases and n + 1 offsets), rbases / roff (the reads'), pool (the CIGAR pool,
len << 4 | op), ov / rp / pr (the overlap records, read pairs and alignment-pair records laid out as in tests/coverage_ref.py)."""
import numpy as np

from coverage_ref import NO_OVERLAP, OVERLAP_DT, PAIRED_OVERLAP_DT, READ_PAIR_DT

ROW_DT = np.dtype([("entry", "<u4"), ("pos", "<u4"), ("ref", "u1"), ("alt", "u1"), ("pad", "u1", (2,)), ("alt_fwd", "<u4"), ("alt_rev", "<u4"),
                   ("depth", "<u4")])
STAT_NAMES = ("n_records", "n_skipped", "n_intervals", "n_events", "n_sites")
ACGT = b"ACGT"
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")   # upper case only; every other byte stays
OPS = {"M": 0, "I": 1, "D": 2}
INFO_LINES = [
    b'##INFO=<ID=DP,Number=1,Type=Integer,Description="Aligned reads with a match or mismatch column at the site">\n',
    b'##INFO=<ID=AO,Number=A,Type=Integer,Description="Alternate allele observations">\n',
    b'##INFO=<ID=SAF,Number=A,Type=Integer,Description="Alternate allele observations on the forward strand">\n',
    b'##INFO=<ID=SAR,Number=A,Type=Integer,Description="Alternate allele observations on the reverse strand">\n',
    b'##INFO=<ID=AF,Number=A,Type=Float,Description="Alternate allele observations over depth">\n']
COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def reverse_complement(b):
    return bytes(b)[::-1].translate(_COMPLEMENT)


# ---------------------------------------------------------------- the definition

def _walk(o, case, memo):
    """one overlap record -> None when it is skipped, else (events [(pos, alt, strand)], intervals [(begin, end)])"""
    key = (int(o["read"]), int(o["entry"]), int(o["ref_begin"]), int(o["query_begin"]), int(o["revcomp"]) != 0, int(o["cigar_off"]), int(o["cigar_len"]))
    if key in memo:
        return memo[key]
    read, entry, ref_begin, query_begin, strand, cigar_off, cigar_len = key
    goff, roff = case["goff"], case["roff"]
    out = None
    if entry < len(goff) - 1 and cigar_len > 0 and ref_begin >= 0:
        ref = case["gbases"][int(goff[entry]):int(goff[entry + 1])]
        query = case["rbases"][int(roff[read]):int(roff[read + 1])]
        if strand:
            query = np.frombuffer(reverse_complement(query.tobytes()), dtype=np.uint8)
        ops = [(int(c) >> 4, int(c) & 15) for c in case["pool"][cigar_off:cigar_off + cigar_len]]
        rp, qp, fits = ref_begin, max(query_begin, 0), True
        for n, op in ops:      # the whole CIGAR first: nothing of a record that runs past its read or its entry is emitted
            if op == 0:
                rp, qp = rp + n, qp + n
            elif op == 1:
                qp += n
            elif op == 2:
                rp += n
            if rp > len(ref) or qp > len(query):
                fits = False
                break
        if fits:
            events, intervals = [], []
            rp, qp = ref_begin, max(query_begin, 0)
            for n, op in ops:
                if op == 0:
                    if n > 0:
                        intervals.append((rp, rp + n - 1))
                        r, q = ref[rp:rp + n], query[qp:qp + n]
                        for j in np.nonzero(r != q)[0]:
                            if int(r[j]) in ACGT and int(q[j]) in ACGT:     # upper case only, on both sides
                                events.append((rp + int(j), int(q[j]), strand))
                    rp, qp = rp + n, qp + n
                elif op == 1:
                    qp += n
                elif op == 2:
                    rp += n
            out = (events, intervals)
    memo[key] = out
    return out


def table(case, min_alt=1, min_depth=0):
    """-> (rows [ROW_DT], stats dict)"""
    ov, rp, pr = case["ov"], case["rp"], case["pr"]
    n_entries = len(case["goff"]) - 1
    named = set()
    for g in rp:
        live = pr[int(g["first"]):int(g["first"]) + int(g["count"])]   # the records behind first + count are dead
        for f in ("r1", "r2"):
            named.update(int(i) for i in live[f] if int(i) != NO_OVERLAP)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["n_records"] = len(named)
    sites = {}
    begins = [[] for _ in range(n_entries)]
    ends = [[] for _ in range(n_entries)]
    memo = {}
    for i in sorted(named):      # each contributes once, however many live pairs name it
        o = ov[i]
        got = _walk(o, case, memo)
        if got is None:
            stats["n_skipped"] += 1
            continue
        events, intervals = got
        e = int(o["entry"])
        for b, t in intervals:
            begins[e].append(b)
            ends[e].append(t)
        stats["n_intervals"] += len(intervals)
        stats["n_events"] += len(events)
        for pos, alt, strand in events:
            s = sites.setdefault((e, pos, alt), [0, 0])
            s[1 if strand else 0] += 1
    stats["n_sites"] = len(sites)
    depth = []
    for e in range(n_entries):
        d = np.zeros(int(case["goff"][e + 1] - case["goff"][e]) + 1, dtype=np.int64)
        if begins[e]:
            np.add.at(d, np.asarray(begins[e], dtype=np.int64), 1)
            np.add.at(d, np.asarray(ends[e], dtype=np.int64) + 1, -1)
        depth.append(np.cumsum(d))
    out = []
    for (e, pos, alt) in sorted(sites):     # the bytes A < C < G < T sort as the alts do
        fwd, rev = sites[(e, pos, alt)]
        d = int(depth[e][pos])
        if fwd + rev >= min_alt and d >= min_depth:
            out.append((e, pos, int(case["gbases"][int(case["goff"][e]) + pos]), alt, (0, 0), fwd, rev, d))
    return np.array(out, dtype=ROW_DT) if out else np.zeros(0, dtype=ROW_DT), stats


def fields(rows):
    """the rows as tuples without the padding (what two tables are compared by)"""
    return [(int(r["entry"]), int(r["pos"]), int(r["ref"]), int(r["alt"]), int(r["alt_fwd"]), int(r["alt_rev"]), int(r["depth"])) for r in rows]


# ---------------------------------------------------------------- the file

def vcf_bytes(rows, loci, lengths, source):
    out = [b"##fileformat=VCFv4.2\n", b"##source=" + source + b"\n"]
    for e in sorted({int(r["entry"]) for r in rows}):
        out.append(b"##contig=<ID=%s,length=%d>\n" % (loci[e], int(lengths[e])))
    out += INFO_LINES + [COLUMNS]
    for r in rows:
        ao, dp = int(r["alt_fwd"]) + int(r["alt_rev"]), int(r["depth"])
        out.append(b"%s\t%d\t.\t%c\t%c\t.\t.\tDP=%d;AO=%d;SAF=%d;SAR=%d;AF=%s\n" % (loci[int(r["entry"])], int(r["pos"]) + 1, int(r["ref"]), int(r["alt"]), dp,
                                                                                   ao, int(r["alt_fwd"]), int(r["alt_rev"]), b"%.6f" % (ao / dp if dp else 0.0)))
    return b"".join(out)


def read_vcf(text, loci, lengths):
    """strict: every line is what kslam_variants_write may write and nothing else.  loci / lengths: of the index, in entry order.
    -> rows as (entry, pos0, ref, alt, alt_fwd, alt_rev, depth) tuples"""
    assert text.endswith(b"\n")
    lines = text[:-1].split(b"\n")
    assert lines[0] == b"##fileformat=VCFv4.2"
    assert lines[1].startswith(b"##source=") and len(lines[1]) > 9 and b" " not in lines[1]
    at = 2
    contigs = []
    while lines[at].startswith(b"##contig="):
        body = lines[at][len(b"##contig=<ID="):-1]
        assert lines[at].startswith(b"##contig=<ID=") and lines[at].endswith(b">")
        name, length = body.rsplit(b",length=", 1)
        e = loci.index(name)
        assert int(length) == int(lengths[e]) and (not contigs or contigs[-1] < e)
        contigs.append(e)
        at += 1
    assert [l + b"\n" for l in lines[at:at + 5]] == INFO_LINES
    assert lines[at + 5] + b"\n" == COLUMNS
    rows = []
    for line in lines[at + 6:]:
        f = line.split(b"\t")
        assert len(f) == 8 and f[2] == b"." and f[5] == b"." and f[6] == b"."
        e = loci.index(f[0])
        pos = int(f[1]) - 1
        assert 0 <= pos < int(lengths[e]) and f[1] == b"%d" % (pos + 1)
        assert len(f[3]) == 1 and f[3] in ACGT and len(f[4]) == 1 and f[4] in ACGT and f[3] != f[4]
        info = [kv.split(b"=") for kv in f[7].split(b";")]
        assert [k for k, _ in info] == [b"DP", b"AO", b"SAF", b"SAR", b"AF"]
        dp, ao, saf, sar = (int(v) for _, v in info[:4])
        assert saf + sar == ao and 1 <= ao <= dp and info[4][1] == b"%.6f" % (ao / dp)
        rows.append((e, pos, f[3][0], f[4][0], saf, sar, dp))
    assert sorted({r[0] for r in rows}) == contigs
    assert rows == sorted(rows) and len({r[:4] for r in rows}) == len(rows)   # (entry, pos, then alt; ref is a function of the two)
    return rows


# ---------------------------------------------------------------- the cases

def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(ACGT, dtype=np.uint8), int(n)).tobytes())


def other_base(b, step=1):
    """another of ACGT than the byte b (any byte that is not ACGT gives 'A')"""
    i = ACGT.find(bytes([b]))
    return ACGT[(i + step) % 4] if i >= 0 else ACGT[0]


class Builder:
    def __init__(self, name, entries):
        self.name, self.entries = name, [bytes(e) for e in entries]
        self.reads, self.pool, self.ov, self.groups = [], [], [], []

    def read(self, bases):
        self.reads.append(bytes(bases))
        return len(self.reads) - 1

    def cigar(self, ops):
        off = len(self.pool)
        self.pool += [(n << 4) | (OPS[op] if isinstance(op, str) else op) for n, op in ops]
        return off, len(ops)

    def rec(self, read, entry, ref_begin, cigar, revcomp=0, query_begin=0):
        """an overlap record over a read and a CIGAR slice (off, len) added before; -> its index"""
        self.ov.append((read, entry, ref_begin, revcomp, query_begin, cigar[0], cigar[1]))
        return len(self.ov) - 1

    def query(self, entry, ref_begin, ops, subs=None, fill=b"A"):
        """the query an alignment of these ops at ref_begin reads: the entry's bases on M, `fill`'s on I; subs: {query position: byte}"""
        ref, q, rp = self.entries[entry], bytearray(), ref_begin
        for n, op in ops:
            if op == "M":
                q += ref[rp:rp + n]
                rp += n
            elif op == "I":
                q += (fill * n)[:n]
            else:
                rp += n
        for at, b in (subs or {}).items():
            q[at] = b
        return bytes(q)

    def aligned(self, entry, ref_begin, ops, revcomp=0, subs=None, mismatch_at=()):
        """read + CIGAR + record of an alignment; mismatch_at: query positions that get another base than the entry has there"""
        q = bytearray(self.query(entry, ref_begin, ops, subs))
        for at in mismatch_at:
            q[at] = other_base(q[at])
        read = self.read(reverse_complement(q) if revcomp else bytes(q))
        return self.rec(read, entry, ref_begin, self.cigar(ops), revcomp)

    def group(self, live, dead=()):
        """live / dead: alignment-pair records (pair_entry, r1, r2) with r1 / r2 an overlap record's index or None"""
        self.groups.append((list(live), list(dead)))

    def single(self, r):
        self.group([(self.ov[r][1], r, None)])

    def done(self, single_end=False):
        goff = np.concatenate([[0], np.cumsum([len(e) for e in self.entries])]).astype(np.uint64)
        roff = np.concatenate([[0], np.cumsum([len(r) for r in self.reads])]).astype(np.uint64)
        ov = np.zeros(len(self.ov), dtype=OVERLAP_DT)
        for i, (read, entry, ref_begin, revcomp, query_begin, off, n) in enumerate(self.ov):
            ov[i]["read"], ov[i]["entry"], ov[i]["ref_begin"], ov[i]["revcomp"], ov[i]["query_begin"] = read, entry, ref_begin, revcomp, query_begin
            ov[i]["cigar_off"], ov[i]["cigar_len"], ov[i]["score"] = off, n, 60
        rp, pr = [], []
        for g, (live, dead) in enumerate(self.groups):
            rp.append((g, 0 if single_end else len(self.groups) + g, len(pr), len(live)))
            for pe, r1, r2 in live + dead:
                pr.append((pe, NO_OVERLAP if r1 is None else r1, NO_OVERLAP if r2 is None else r2))
        return arrays(self.name, b"".join(self.entries), goff, b"".join(self.reads), roff, self.pool, ov, rp, pr)


def arrays(name, gbases, goff, rbases, roff, pool, ov, rp, pr):
    p = np.zeros(len(pr), dtype=PAIRED_OVERLAP_DT)
    if len(pr):
        t = np.asarray(pr, dtype=np.int64).reshape(-1, 3)
        p["entry"], p["r1"], p["r2"] = t[:, 0], t[:, 1], t[:, 2]
        p["combined_score"] = 100
    r = np.zeros(len(rp), dtype=READ_PAIR_DT)
    if len(rp):
        t = np.asarray(rp, dtype=np.int64).reshape(-1, 4)
        r["r1_read"], r["r2_read"], r["first"], r["count"] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    return {"name": name, "gbases": np.frombuffer(bytes(gbases), dtype=np.uint8), "goff": np.asarray(goff, dtype=np.uint64),
            "rbases": np.frombuffer(bytes(rbases), dtype=np.uint8), "roff": np.asarray(roff, dtype=np.uint64),
            "pool": np.asarray(pool, dtype=np.uint32), "ov": ov, "rp": r, "pr": p}


def concat(a, b):
    """two cases over the same entries as one batch"""
    assert a["gbases"].tobytes() == b["gbases"].tobytes()
    ov2, pr2, rp2 = b["ov"].copy(), b["pr"].copy(), b["rp"].copy()
    ov2["read"] += len(a["roff"]) - 1
    ov2["cigar_off"] += len(a["pool"])
    for f in ("r1", "r2"):
        keep = pr2[f] != NO_OVERLAP
        pr2[f][keep] += len(a["ov"])
    rp2["first"] += len(a["pr"])
    roff = np.concatenate([a["roff"], b["roff"][1:] + a["roff"][-1]])
    return {"name": a["name"] + "+" + b["name"], "gbases": a["gbases"], "goff": a["goff"], "rbases": np.concatenate([a["rbases"], b["rbases"]]),
            "roff": roff, "pool": np.concatenate([a["pool"], b["pool"]]), "ov": np.concatenate([a["ov"], ov2]),
            "rp": np.concatenate([a["rp"], rp2]), "pr": np.concatenate([a["pr"], pr2])}


WALK_COLUMNS = (0, 15, 16, 17, 31, 39)   # of a 40-base read: both sides of the 16-byte chunks, the first and the last column
CIGAR_SHAPES = {
    "ins-del": [(1, "M"), (2, "I"), (30, "M"), (2, "D"), (1, "M")],       # I directly after the first M, D directly before the last
    "del-ins": [(1, "M"), (2, "D"), (30, "M"), (2, "I"), (1, "M")],
    "split": [(20, "M"), (5, "D"), (20, "M")],                             # two intervals: the deleted positions have one less depth
    "m-i-m": [(10, "M"), (3, "I"), (10, "M")],                             # adjacent intervals, no gap in depth
    "zero-m": [(0, "M"), (10, "M"), (0, "M"), (2, "I"), (0, "M"), (17, "M"), (0, "M")],
}


def repeated(name, n_records, entry_len=60):
    """n_records records over one read with one mismatch: ONE key n_records times"""
    rng = np.random.default_rng(n_records)
    b = Builder(name, [random_bases(rng, entry_len)])
    fwd = b.aligned(0, 10, [(20, "M")], 0, mismatch_at=(7,))
    read, cig = b.ov[fwd][0], (b.ov[fwd][5], b.ov[fwd][6])
    b.single(fwd)
    for k in range(1, n_records):
        b.single(b.rec(read, 0, 10, cig))
    return b.done()


def distinct(name, n_keys):
    """n_keys distinct (pos, alt): one-base reads A, C, G, T against every position of one entry"""
    rng = np.random.default_rng(n_keys)
    b = Builder(name, [random_bases(rng, (n_keys + 2) // 3)])
    reads = [b.read(bytes([c])) for c in ACGT]
    cig = b.cigar([(1, "M")])
    made = 0
    for pos, ref in enumerate(b.entries[0]):
        for k, c in enumerate(ACGT):
            if c != ref and made < n_keys:
                b.single(b.rec(reads[k], 0, pos, cig, revcomp=0))
                made += 1
    return b.done()


def invalid_kinds(b, entry, rng=None):
    """one skipped record of each kind on `entry` (at least 60 long) of builder b -> their indices"""
    n = len(b.entries[entry])
    read = b.read(b.entries[entry][5:45])
    full = b.cigar([(40, "M")])
    out = [b.rec(read, entry, 5, (0, 0)),                              # cigar_len == 0
           b.rec(read, len(b.entries) + 1, 5, full),                   # entry >= n_entries
           b.rec(read, entry, -1, full),                               # ref_begin < 0
           b.rec(read, entry, n - 39, full),                           # M past the entry (by one)
           b.rec(read, entry, 5, b.cigar([(41, "M")])),                # M past the read
           b.rec(read, entry, 5, b.cigar([(30, "M"), (11, "I")])),     # I past the read
           b.rec(read, entry, n - 40, b.cigar([(39, "M"), (2, "D"), (1, "M")]))]   # D past the entry
    return out


def random_case(name, seed, n_pairs, n_entries, max_len=400, n_alignments=None, invalid=True, entries=None):
    """n_pairs alignment-pair records (live and dead) in groups of random size over a pool of random alignments"""
    rng = np.random.default_rng(seed)
    if entries is None:
        entries = [random_bases(rng, rng.integers(1, max_len + 1)) for _ in range(n_entries)]
    b = Builder(name, entries)
    n_alignments = n_alignments if n_alignments is not None else max(1, n_pairs // 3)
    for _ in range(n_alignments):
        e = int(rng.integers(0, len(entries)))
        n = len(entries[e])
        span = int(min(n, rng.integers(1, 121)))
        begin = int(rng.integers(0, n - span + 1))
        ops, left = [], span
        while left:      # M runs with an I or a D between them, inside the span
            m = int(min(left, rng.integers(1, 60)))
            ops.append((m, "M"))
            left -= m
            if left > 2 and rng.random() < 0.4:
                if rng.random() < 0.5:
                    ops.append((int(rng.integers(1, 4)), "I"))
                else:
                    d = int(rng.integers(1, 3))
                    ops.append((d, "D"))
                    left -= d
        if ops[-1][1] != "M":
            ops.pop()
        q_len = sum(n_ for n_, op in ops if op != "D")
        miss = [int(x) for x in np.nonzero(rng.random(q_len) < 0.06)[0]]
        subs = {int(x): b"Nacgtn"[int(rng.integers(0, 6))] for x in np.nonzero(rng.random(q_len) < 0.01)[0]}
        b.aligned(e, begin, ops, int(rng.random() < 0.5), subs=subs, mismatch_at=[m for m in miss if m not in subs])
    if invalid:
        long_entries = [e for e in range(len(entries)) if len(entries[e]) >= 60]
        for e in long_entries[:3]:
            invalid_kinds(b, e)
    n_ov = len(b.ov)
    made = 0
    while made < n_pairs:
        size = int(min(rng.integers(1, 7), n_pairs - made))
        live = int(rng.integers(0, size + 1)) if rng.random() < 0.3 else size
        recs = []
        for _ in range(size):
            r1 = int(rng.integers(0, n_ov)) if rng.random() < 0.85 else None
            r2 = int(rng.integers(0, n_ov)) if (rng.random() < 0.85 or r1 is None) else None
            recs.append((b.ov[r1 if r1 is not None else r2][1], r1, r2))
        b.group(recs[:live], recs[live:])
        made += size
    return b.done()


def cases():
    rng = np.random.default_rng(20260)
    out = []
    base = random_bases(rng, 200)
    # ---- walk seams: one read of 40 bases with one mismatch, per column and strand; the reverse read is read 0 of its batch
    for col in WALK_COLUMNS:
        for rc in (0, 1):
            b = Builder("walk-col%d-%s" % (col, "rev" if rc else "fwd"), [base])
            b.single(b.aligned(0, 50, [(40, "M")], rc, mismatch_at=(col,)))
            out.append(b.done())
    for rc in (0, 1):
        b = Builder("walk-all-%s" % ("rev" if rc else "fwd"), [base])
        b.single(b.aligned(0, 50, [(40, "M")], rc, mismatch_at=WALK_COLUMNS))
        b.single(b.aligned(0, 0, [(40, "M")], rc, mismatch_at=WALK_COLUMNS))       # from the entry's first base
        b.single(b.aligned(0, 160, [(40, "M")], rc, mismatch_at=WALK_COLUMNS))     # to its last
        b.single(b.aligned(0, 50, [(40, "M")], 1 - rc, mismatch_at=(0, 16, 39)))   # the other strand on the same sites
        out.append(b.done())
    for shape, ops in CIGAR_SHAPES.items():
        q_len = sum(n for n, op in ops if op != "D")
        for rc in (0, 1):
            b = Builder("cigar-%s-%s" % (shape, "rev" if rc else "fwd"), [base])
            b.single(b.aligned(0, 30, ops, rc, mismatch_at=sorted({0, 1, 9, 10, 12, 19, 20, 22, q_len - 2, q_len - 1})))
            b.single(b.aligned(0, 20, [(70, "M")], 1 - rc, mismatch_at=range(5, 70, 3)))   # a plain read over all of it: depth on both sides
            out.append(b.done())
    # ---- alphabet: N and lower case in the read, in the entry and in both at one column: no event, but depth
    e = bytearray(random_bases(rng, 100))
    e[10:14] = b"NaNg"
    e[20], e[21] = ord("A"), ord("C")
    for rc in (0, 1):
        b = Builder("alphabet-%s" % ("rev" if rc else "fwd"), [bytes(e)])
        q = bytearray(b.query(0, 5, [(60, "M")]))
        q[5:9] = b"CCNg"              # over N a N g: upper against N, upper against lower, N against N, the same lower case
        q[15], q[16] = ord("n"), ord("a")   # lower case and n in the read against A and C
        q[30] = other_base(q[30])    # and one true event
        read = b.read(reverse_complement(q) if rc else bytes(q))
        b.single(b.rec(read, 0, 5, b.cigar([(60, "M")]), rc))
        b.single(b.aligned(0, 0, [(70, "M")], 1 - rc, mismatch_at=(20, 21, 35, 12)))   # true events on the columns above: depth 2 there
        out.append(b.done())
    # ---- entry seams: entries of length 1, 63, 64, 65 side by side, covered whole and at their ends
    lens = [1, 63, 64, 65]
    entries = [random_bases(rng, n) for n in lens]
    for rc in (0, 1):
        b = Builder("entries-%s" % ("rev" if rc else "fwd"), entries)
        for e_, n in enumerate(lens):
            b.single(b.aligned(e_, 0, [(n, "M")], rc, mismatch_at=sorted({0, n - 1})))
        b.single(b.aligned(1, 40, [(23, "M")], rc, mismatch_at=(22,)))      # ends at len - 1 of entry 1 ...
        b.single(b.aligned(2, 0, [(20, "M")], 1 - rc, mismatch_at=(0,)))    # ... next to one that starts at 0 of entry 2
        b.single(b.aligned(3, 45, [(20, "M")], rc, mismatch_at=(19,)))      # the last base of the index
        out.append(b.done())
    # ---- depth seams around a site p
    p = 100
    b = Builder("depth", [random_bases(rng, 300)])
    b.single(b.aligned(0, 90, [(40, "M")], 0, mismatch_at=(10,)))
    for begin, n in ((p, 1), (p + 1, 30), (p - 30, 30), (0, p + 1), (p, 300 - p)):
        b.single(b.aligned(0, begin, [(n, "M")], begin & 1))
    out.append(b.done())
    out.append(repeated("depth-20000", 20000))
    # ---- run seams
    for n in (255, 256, 257, 70001):
        out.append(repeated("run-%d" % n, n))
    out.append(distinct("distinct-70001", 70001))
    b = Builder("alts", [random_bases(rng, 80)])
    for step in (1, 2, 3):         # three alts at one site on both strands, and events that differ only in the strand
        for rc in (0, 1, 1):
            q = bytearray(b.query(0, 10, [(30, "M")]))
            q[12] = other_base(q[12], step)
            b.single(b.rec(b.read(reverse_complement(q) if rc else bytes(q)), 0, 10, b.cigar([(30, "M")]), rc))
    out.append(b.done())
    # ---- contributing set
    ents = [random_bases(rng, 100) for _ in range(4)]
    b = Builder("contributing", ents)
    dead = b.aligned(3, 0, [(50, "M")], 0, mismatch_at=(3, 4))          # entry 3: only dead records point at it
    a0 = b.aligned(0, 0, [(10, "M")], 0, mismatch_at=(2,))
    b.group([(0, a0, None)], [(3, dead, None), (3, None, dead)])        # count smaller than the gap to the next first
    b.group([], [(3, dead, dead)])                                      # count == 0
    thrice = b.aligned(1, 5, [(30, "M")], 1, mismatch_at=(0, 29))
    mate = b.aligned(1, 20, [(30, "M")], 0, mismatch_at=(14,))         # over thrice's last column: depth 2 there
    b.group([(1, thrice, None), (1, None, thrice), (1, thrice, mate)])  # named by three live pairs: once
    b.group([(2, b.aligned(2, 1, [(8, "M")], 0, mismatch_at=(7,)), None)], [(3, dead, None)] * 3)   # r2 == KSLAM_NO_OVERLAP, a dead tail at the end
    out.append(b.done())
    b = Builder("single-end", ents)
    b.single(b.aligned(0, 10, [(50, "M")], 0, mismatch_at=(0, 49)))
    b.group([(1, b.aligned(1, 0, [(100, "M")], 1, mismatch_at=(0, 50, 99)), None), (0, b.aligned(0, 50, [(20, "M")], 1, mismatch_at=(5,)), None)])
    out.append(b.done(single_end=True))
    # ---- skipped: one of each kind among valid ones
    b = Builder("skipped", ents)
    b.single(b.aligned(0, 60, [(40, "M")], 0, mismatch_at=(39,)))      # ends exactly at the entry's end: valid
    for r in invalid_kinds(b, 0):
        b.single(r)
    b.single(b.aligned(0, 0, [(30, "M"), (10, "I")], 0, mismatch_at=(1,)))   # I up to the read's end: valid
    b.single(b.aligned(0, 58, [(40, "M"), (2, "D")], 0, mismatch_at=(1,)))   # D up to the entry's end: valid
    out.append(b.done())
    # ---- grid seams
    for n in (0, 1, 255, 257):
        out.append(random_case("grid-%d" % n, 100 + n, n, 5, invalid=False))
    out.append(random_case("grid-70001", 4242, 70001, 300))
    return out


def filter_case():
    """a site with exactly 2 events and depth 5, next to one with 1 event and one with 3"""
    rng = np.random.default_rng(77)
    b = Builder("filters", [random_bases(rng, 120)])
    for k in range(5):
        b.single(b.aligned(0, 10 + k, [(60, "M")], k & 1, mismatch_at=[at for at, n in ((30 - k, 2), (35 - k, 1), (40 - k, 3)) if k < n]))
    return b.done()


def planted(seed=2026, length=20000, n_sites=100, read_len=100, fold=15):
    """an entry of random bases, a copy with n_sites substitutions at least 200 apart, and error-free reads of the copy on both
    strands -> (entry, sites {pos: planted base}, reads [(bases as sequenced, position, revcomp)])"""
    rng = np.random.default_rng(seed)
    entry = random_bases(rng, length)
    copy = bytearray(entry)
    sites = {}
    first = (length - 200 * (n_sites - 1)) // 2      # a read length from both ends: full coverage on every site
    for k in range(n_sites):
        pos = first + 200 * k
        sites[pos] = other_base(entry[pos], 1 + int(rng.integers(0, 3)))
        copy[pos] = sites[pos]
    reads = []
    for _ in range(fold * length // read_len):
        at = int(rng.integers(0, length - read_len + 1))
        rc = int(rng.random() < 0.5)
        q = bytes(copy[at:at + read_len])
        reads.append((reverse_complement(q) if rc else q, at, rc))
    return entry, sites, reads


def planted_case(entry, reads, extra_entries=()):
    b = Builder("planted", [entry] + list(extra_entries))
    cig = b.cigar([(len(reads[0][0]), "M")])
    for bases, at, rc in reads:
        b.single(b.rec(b.read(bases), 0, at, cig, rc))       # its true alignment: one full-length M at its true position
    return b.done()
