"""Case builders for the seams of the per-row walk (k-slam_amd/csrc/details.hip) and of the device SAM text and per-read
lines (k-slam_amd/csrc/samtext.hip): overlap rows and their CIGAR pool written by hand, so that a match run is exactly 999 /
1000 columns, an MD text exactly 48 / 49 bytes, a mismatch sits in column 15 / 16 of a chunk, a row's log-probability just
above / below the mapping-quality plan's bar of -300, a POS has 9 / 10 digits, a batch 255 / 256 / 257 rows or read pairs.
Pure numpy: tests/test_details_seams.py proves every claim with tests/rowdetails_ref.py and holds the host tail to the oracle's
restatement on the same rows; tests/test_gpu_details_seams.py runs the same cases through the device.

A case is a dict: name, entries, reads ([R1 block | R2 block] when paired), quals, ids, ov (OVERLAP_DT, sorted by read, entry,
rel as the aligner emits them), pool (the CIGAR pool), claim {measure: exact value}, the parameters (paired, num_alignments,
sam_xa, report_cigar, score_threshold; stages and score_fraction of the pairing: the score screen with a fraction of 0, which
removes nothing, unless the case says otherwise), the annotations (locus, tax_ids, genes, taxdb) and
  oracle   False where the reference has no answer (a quality byte outside '!' .. '~' in an aligned column indexes past its
           tables): the two host paths are still compared with each other
  refusal  the message every path must refuse the batch with (None: the text is compared)."""
import numpy as np

from tail_seams import OVERLAP_DT

# copies of the constants in csrc/details.hip, csrc/samtext.hip, host/tail.cpp and csrc/gnu_sort.h (test_details_seams.py
# compares them with the source text)
MD_SLOT = 48          # an MD text of up to 48 bytes waits in the row's slot, a longer one is walked again into the pool
CHUNK = 16            # columns per unaligned 16-byte load
MD_SMALL = 1000       # MdOut::num: below this, the three-digit path
Q_CLAMP = 100         # phred+33 values 0 .. 99 are in the tables
LOGP_BAR = -300.0     # a lone reported row at or below this has its 10^logp evaluated
BLOCK = 256           # threads per block, every kernel of both files
INSERTION_SORT = 16   # gnu_sort.h: ranges up to 16 records are insertion-sorted
Q93 = 126             # '~': phred 93, the highest printable quality

_COMP = bytes.maketrans(b"ACGT", b"TGCA")       # upper case only, as reverseComplement
_OTHER = bytes.maketrans(b"ACGT", b"CGTA")      # a base that differs
OPS = {"M": 0, "I": 1, "D": 2}

SPECIAL = b"ACGTacgtNnUuRYKMSWBDHVrykm-.*ACGTNACGTnacgtuACGT" * 8          # entry 1: every kind of character a column can hold


def genome(seed, n):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


ENTRIES = [genome(1, 9500), SPECIAL, genome(2, 700)]
DEFAULT_TAXDB = [(1, 1, b"root", b"no rank"), (2, 1, b"Bacteria", b"superkingdom")]


def taxdb_text(recs):
    return b"".join(b"%d\n%d\n%s\n%s\n" % r for r in recs)


def parse_cigar(text):
    """"10M2I10M" -> [(10, "M"), (2, "I"), (10, "M")]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), ch))
            n = ""
    return out


class Batch:
    """reads and rows, one at a time; case() sorts the rows as the aligner would and lays the reads out"""

    def __init__(self, entries=None):
        self.entries = list(ENTRIES if entries is None else entries)
        self.reads, self.quals, self.rows, self.pool = [], [], [], []

    def read(self, bases, qual=None):
        self.reads.append(bytes(bases))
        self.quals.append(bytes(qual) if qual is not None else b"I" * len(bases))
        return len(self.reads) - 1

    def row(self, read, entry, ref_begin, ref_end, rc=0, score=100, rel=None, query_begin=0, query_end=None, cigar=None):
        off = len(self.pool)
        if cigar:
            self.pool += [(n << 4) | OPS[op] for n, op in cigar]
        if query_end is None:
            query_end = len(self.reads[read]) - 1
        self.rows.append((read, entry, ref_begin - query_begin if rel is None else rel, int(bool(rc)), score, ref_begin, ref_end,
                          query_begin, query_end, len(cigar) if cigar else 0, off if cigar else 0))
        return len(self.rows) - 1

    def walk(self, cigar, entry=0, ref_begin=0, rc=False, miss=(), sub=None, clip=(0, 0), qual=None, score=None, cut=0, fill=73, ghost_insert=False):
        """a new read that aligns to entries[entry] at ref_begin with exactly this CIGAR.  miss: M columns (counted over all
        the M operations) whose read base differs; sub: {M column: byte} put into the read there; clip: soft-clipped bases in
        front and behind; qual: {position in the query, clips included: quality byte}; cut: bases taken off the end of the
        read after the row is made (the CIGAR then runs past it); ghost_insert: inserted bases are not in the read at all; a
        window past the end of the entry reads as 'A'"""
        cigar = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
        ref = self.entries[entry]
        q, rp, col = bytearray(b"T" * clip[0]), ref_begin, 0
        sub = sub or {}
        for n, op in cigar:
            if op == "M":
                for i in range(n):
                    r = ref[rp + i:rp + i + 1] or b"A"
                    if col in sub:
                        r = bytes([sub[col]])
                    elif col in miss:
                        r = r.translate(_OTHER) if r in (b"A", b"C", b"G", b"T") else b"A"
                    q += r
                    col += 1
                rp += n
            elif op == "I":
                if not ghost_insert:
                    q += (b"GATTACA" * (n // 7 + 1))[:n]
            else:
                rp += n
        aligned = len(q) - clip[0]
        q += b"G" * clip[1]
        ql = bytearray([fill]) * len(q)
        for at, b in (qual or {}).items():
            ql[at] = b
        if cut:
            q, ql = q[:-cut], ql[:-cut]
        q, ql = bytes(q), bytes(ql)
        r = self.read(q.translate(_COMP)[::-1] if rc else q, ql[::-1] if rc else ql)
        if score is None:
            score = 100 if len(self.rows) % 2 == 0 else 50
        return self.row(r, entry, ref_begin, rp - 1, rc, score, query_begin=clip[0], query_end=clip[0] + aligned - 1, cigar=cigar)

    def plain(self, entry=0, ref_begin=0, rc=False, score=None, length=30):
        """a new read with a row that has no CIGAR (it is not walked)"""
        r = self.read(b"ACGT" * (length // 4) + b"A" * (length % 4))
        if score is None:
            score = 100 if len(self.rows) % 2 == 0 else 50
        return self.row(r, entry, ref_begin, ref_begin + length - 1, rc, score)


def make_case(name, batch, claim, paired=True, num_alignments=10, sam_xa=False, report_cigar=True, score_threshold=0, ids=None,
              locus=None, tax_ids=None, genes=None, taxdb=None, oracle=True, refusal=None, keep_order=False, family=None, stages=2,
              score_fraction=0.0):
    reads, quals = list(batch.reads), list(batch.quals)
    if paired and len(reads) % 2:
        reads.append(b"ACGTACGTACGTACGTACGTACGTACGTAC")
        quals.append(b"I" * 30)
    n = len(reads)
    ov = np.zeros(len(batch.rows), dtype=OVERLAP_DT)
    fields = ("read", "entry", "rel", "revcomp", "score", "ref_begin", "ref_end", "query_begin", "query_end", "cigar_len", "cigar_off")
    for k, f in enumerate(fields):
        col = np.array([r[k] for r in batch.rows], dtype=np.int64)
        if len(col):
            assert col.min() >= np.iinfo(OVERLAP_DT[f]).min and col.max() <= np.iinfo(OVERLAP_DT[f]).max, (name, f)
        ov[f] = col
    if len(ov):           # every row names a read, an entry and a slice of the pool that exist
        assert ov["read"].max() < n and ov["entry"].max() < len(batch.entries), name
        assert (ov["cigar_off"] + ov["cigar_len"]).max() <= len(batch.pool), name
    order = np.lexsort((ov["rel"], ov["entry"], ov["read"]))
    if keep_order:        # the case speaks of row numbers: the rows must be in the aligner's order as they were added
        assert (order == np.arange(len(ov))).all(), name
    ov = ov[order]
    mid = n // 2 if paired else n
    if ids is None:
        ids = [b"r%d" % (i % mid) for i in range(n)]
    ne = len(batch.entries)
    return dict(name=name, family=family or name[0], entries=batch.entries, reads=reads, quals=quals, ids=list(ids), ov=ov,
                pool=np.array(batch.pool, dtype=np.uint32), claim=claim, paired=paired, num_alignments=num_alignments, sam_xa=sam_xa,
                report_cigar=report_cigar, score_threshold=score_threshold,
                locus=locus or [b"NC_%06d.%d" % (e, e % 3 + 1) for e in range(ne)],
                tax_ids=list(tax_ids) if tax_ids is not None else [1000 + e for e in range(ne)], genes=genes,
                taxdb=taxdb_text(taxdb if taxdb is not None else DEFAULT_TAXDB + [(1000 + e, 2, b"strain %d" % e, b"strain") for e in range(ne)]),
                oracle=oracle, refusal=refusal, stages=stages, score_fraction=score_fraction)


# ---- W: the walk -----------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 48)


def _w_runs():
    """one M run of each length on both strands: no mismatch, one in column 0 / 15 / 16 / the last, a whole chunk of them,
    and two runs with mismatches in the last column of the first and the first column of the second"""
    B, at, md = Batch(), 100, {}
    for rc in (False, True):
        for n in RUN_LENGTHS:
            sets = [set(), {0}, {n - 1}] + [{c} for c in (15, 16) if c < n]
            sets += [set(range(c, min(c + CHUNK, n))) for c in range(0, n, CHUNK)]
            for miss in sets:
                B.walk("%dM" % n, 0, at, rc, miss)
                at += 53
            for sep in ("1I", "1D", "2I3D"):
                B.walk("%dM%s%dM" % (n, sep, n), 0, at, rc, {n - 1, n})
                at += 53
    # what the reference's merge must give, worked by hand for a few of them
    e = ENTRIES[0]
    md["first_row"] = b"1"
    md["second_row"] = e[100 + 53:100 + 54]
    return make_case("W-runs-of-1-to-48-columns", B, {"rows": len(B.rows), "md_of_row_0": md["first_row"], "md_of_row_1": md["second_row"]},
                     keep_order=True)


def _w_indels():
    B, at = Batch(), 40
    e = ENTRIES[0]
    want = {}

    def add(key, cigar, miss=(), clip=(0, 0), md=None):
        nonlocal at
        for rc in (False, True):
            i = B.walk(cigar, 0, at, rc, miss, clip=clip)
            if md is not None:
                want["md_of_row_%d" % i] = md(at)
            at += 61
    add("merge", "10M2I10M", md=lambda a: b"20")
    add("merge3", "5M1I5M1I5M0M7M", md=lambda a: b"22")
    add("d-mismatch", "10M2D10M", {10}, md=lambda a: b"10^" + e[a + 10:a + 12] + b"0" + e[a + 12:a + 13] + b"9")
    add("d-match-mismatch", "10M2D10M", {11}, md=lambda a: b"10^" + e[a + 10:a + 12] + b"1" + e[a + 13:a + 14] + b"8")
    add("d-i-mismatch", "10M2D1I10M", {10}, md=lambda a: b"10^" + e[a + 10:a + 12] + b"0" + e[a + 12:a + 13] + b"9")
    add("d-d", "10M1D2D10M", md=lambda a: b"10^" + e[a + 10:a + 11] + b"^" + e[a + 11:a + 13] + b"10")
    add("d-d-mismatch", "10M1D2D10M", {10}, md=lambda a: b"10^" + e[a + 10:a + 11] + b"^" + e[a + 11:a + 13] + b"0" + e[a + 13:a + 14] + b"9")
    add("d-first", "2D20M", md=lambda a: b"^" + e[a:a + 2] + b"20")
    add("d-first-mismatch", "2D20M", {0}, md=lambda a: b"^" + e[a:a + 2] + b"0" + e[a + 2:a + 3] + b"19")
    add("d-last", "20M2D", md=lambda a: b"20^" + e[a + 20:a + 22])
    add("i-first", "2I20M", {0}, md=lambda a: e[a:a + 1] + b"19")
    add("i-last", "20M2I", {19}, md=lambda a: b"19" + e[a + 19:a + 20])
    add("zero-m", "10M0M10M", {9, 10}, md=lambda a: b"9" + e[a + 9:a + 11] + b"9")
    add("zero-m-first", "0M20M", md=lambda a: b"20")
    add("zero-m-last", "20M0M", {19})
    add("d-zero-m-mismatch", "10M2D0M10M", {10}, md=lambda a: b"10^" + e[a + 10:a + 12] + b"0" + e[a + 12:a + 13] + b"9")
    add("only-i", "7I", md=lambda a: b"")
    add("clip-front", "20M", {3}, clip=(5, 0))
    add("clip-back", "20M", {3}, clip=(0, 7))
    add("clip-both", "17M1I17M", {16, 17}, clip=(3, 4))
    add("clip-16", "33M", {32}, clip=(16, 16))
    return make_case("W-indels-clips-and-zero-length-runs", B, dict(want, rows=len(B.rows)), keep_order=True)


LONG_RUNS = (999, 1000, 1001, 8999)


def _w_long():
    """match runs of 999 / 1000 / 1001 / 8999 columns from reads of 1001 / 1001 / 1001 / 9000 bases"""
    B = Batch()
    e = ENTRIES[0]
    B.walk("999M", 0, 7, False, clip=(0, 2))
    B.walk("1001M", 0, 11, True, {1000})
    B.walk("1001M", 0, 13, False)
    B.walk("9000M", 0, 17, True, {8999})
    return make_case("W-match-runs-of-999-1000-1001-8999", B,
                     {"md_of_row_0": b"999", "md_of_row_1": b"1000" + e[1011:1012], "md_of_row_2": b"1001", "md_of_row_3": b"8999" + e[9016:9017],
                      "read_lengths": [1001, 1001, 1001, 9000]}, keep_order=True)


def md_walk_of_length(n):
    """(CIGAR, mismatching columns) of a row whose MD text is exactly n bytes: k times "1X", then the last run's digits"""
    if n % 2:
        k, t = (n - 1) // 2, 1
    else:
        k, t = (n - 2) // 2, 10
    return "%dM" % (2 * k + t), set(range(1, 2 * k, 2))


MD_LENGTHS = (47, 48, 49, 50, 200)


def _w_md_lengths():
    B, at = Batch(), 300
    claim = {}
    for rc in (False, True):
        for n in MD_LENGTHS:
            cigar, miss = md_walk_of_length(n)
            claim["md_len_of_row_%d" % B.walk(cigar, 0, at, rc, miss)] = n
            at += 211
    return make_case("W-md-of-47-48-49-50-200-bytes", B, claim, keep_order=True)


def _w_md_placement():
    """300 rows; the ones at thread 0, 255 and 256 of the launch have MD texts of 49 / 200 / 49 bytes, a few others 48"""
    B, claim = Batch(), {"rows": 300}
    for i in range(300):
        rc = i % 3 == 1
        if i in (0, 255, 256, 299):
            n = 200 if i == 255 else 49
            cigar, miss = md_walk_of_length(n)
            B.walk(cigar, 0, 20 + 29 * i, rc, miss)
            claim["md_len_of_row_%d" % i] = n
        elif i in (1, 254, 257):
            cigar, miss = md_walk_of_length(48)
            B.walk(cigar, 0, 20 + 29 * i, rc, miss)
            claim["md_len_of_row_%d" % i] = 48
        else:
            B.walk("20M", 0, 20 + 29 * i, rc, {i % 20})
    claim["rows_beyond_the_slot"] = 4
    return make_case("W-long-md-at-thread-0-255-256", B, claim, keep_order=True)


def _w_first_read_reverse():
    """read 0 of the batch on the reverse strand: the last chunk's 16-byte load would start 1 .. 15 bytes before the array"""
    out = []
    for r in range(1, 16):
        n = r if r % 2 else CHUNK + r
        B = Batch()
        B.walk("%dM" % n, 0, 500 + r, True, {0, n - 1} if r % 3 else set())
        B.walk("20M", 0, 900, False, {4})
        out.append(make_case("W-first-read-reverse-%d-bytes-before-the-array" % (CHUNK - r), B,
                             {"bytes_before_array": CHUNK - r, "run": n}, keep_order=True))
    return out


def _w_ends():
    B = Batch()
    last = len(ENTRIES) - 1
    n_last = len(ENTRIES[last])
    for rc in (False, True):
        B.walk("40M", 0, 0, rc, {0, 39})                                   # starts at ref_begin 0
        B.walk("40M", last, n_last - 40, rc, {0, 39})                      # ends on the last base of the last entry
        B.walk("10M3D", last, n_last - 13, rc, {9})                       # ... with a deletion
        B.walk("33M", 0, len(ENTRIES[0]) - 33, rc, {32})                   # ... of the first entry
    B.walk("17M", 1, 3, True)
    B.walk("47M", last, 100, False, {46})                                  # the last read, forward, to its last base
    assert len(B.reads) % 2 == 0
    return make_case("W-rows-at-the-ends-of-the-arrays", B, {"last_row_ends_the_last_read": 1, "rows_ending_the_last_entry": 4,
                                                            "rows_at_ref_begin_0": 2}, keep_order=True)


def _w_alphabet():
    """lower case, N, U, IUPAC codes and '-' in entry and read columns, both strands: columns compare raw bytes and only
    upper-case ACGT complement"""
    B = Batch()
    pal = b"acgtNnUuRY-ACGT.*"
    for rc in (False, True):
        for at in (0, 7, 48):
            B.walk("40M", 1, at, rc)                                                       # the read repeats the entry: all match
            B.walk("40M", 1, at, rc, sub={c: pal[(c + at) % len(pal)] for c in range(0, 40, 3)})
            B.walk("19M2D19M", 1, at, rc, sub={c: pal[(2 * c + at) % len(pal)] for c in range(0, 38, 2)})
        B.walk("30M", 0, 200, rc, sub={c: pal[c % len(pal)] for c in range(0, 30, 2)})      # an ACGT entry, special read
    return make_case("W-lower-case-N-U-IUPAC-and-dash", B, {"md_of_row_0": b"40", "nm_of_row_0": 0}, keep_order=True)


QUAL_BYTES = (32, 33, 132, 133)


def _w_quality(aligned, which=QUAL_BYTES, oracle=True):
    """quality bytes 32 / 33 / 132 / 133 (phred -1, 0, 99, 100) in an aligned column (32 and 133 set flag 1), or in a
    clipped / inserted base (no flag).  In an aligned column the reference answers for byte 33 alone: it indexes its tables
    with a signed char minus 33, so 32 and every byte from 128 on (132 is -124 there) read outside them"""
    B, claim, at = Batch(), {}, 60
    for rc in (False, True):
        for b in which:
            if aligned:
                for pos, miss in ((0, ()), (16, {16}), (24, ())):
                    i = B.walk("12M1I12M", 0, at, rc, miss, qual={pos: b}, clip=(0, 3))
                    claim["flags_of_row_%d" % i] = int(b in (32, 133))
                    at += 37
            else:
                for pos in (0, 14, 27):             # a clipped base in front, the inserted base, a clipped base behind
                    i = B.walk("12M1I12M", 0, at, rc, {5}, qual={pos: b}, clip=(2, 3))
                    claim["flags_of_row_%d" % i] = 0
                    at += 37
    name = "W-quality-%s-in-%s" % ("-".join(str(b) for b in which), "an-aligned-column" if aligned else "a-clipped-or-inserted-base")
    return make_case(name, B, claim, oracle=oracle, keep_order=True)


def _w_n_rows(n):
    """n rows, every seventh without a CIGAR"""
    B = Batch()
    for i in range(n):
        if i % 7 == 3:
            B.plain(0, 10 + 31 * i, i % 2 == 1)
        else:
            B.walk("%dM" % (20 + i % 5), 0, 10 + 31 * i, i % 2 == 1, {i % 20})
    return make_case("W-%d-rows" % n, B, {"rows": n, "rows_without_cigar": len(range(3, n, 7))}, keep_order=True)


def cases_w():
    out = [_w_runs(), _w_indels(), _w_long(), _w_md_lengths(), _w_md_placement()] + _w_first_read_reverse()
    out += [_w_ends(), _w_alphabet(), _w_quality(True, (33,)), _w_quality(True, (32, 132, 133), oracle=False), _w_quality(False)]
    out += [_w_n_rows(n) for n in (1, BLOCK - 1, BLOCK, BLOCK + 1)]
    return out


# ---- F: CIGARs that run past the read or the entry (flags & 2) -------------------------------------------------------------
def cases_f():
    out = []
    last = len(ENTRIES) - 1
    n_last = len(ENTRIES[last])
    for what in ("M-past-read", "M-past-read-reverse", "M-past-entry", "D-past-entry", "M-past-read-after-I"):
        B = Batch()
        for i in range(3):
            B.walk("25M", 0, 100 + 40 * i, i % 2 == 1, {i})
        if what == "M-past-read":
            bad = B.walk("30M", 0, 400, False, {3}, cut=1)
        elif what == "M-past-read-reverse":
            bad = B.walk("30M", 0, 400, True, {3}, cut=1)
        elif what == "M-past-entry":
            bad = B.walk("30M", last, n_last - 29, False)
        elif what == "D-past-entry":
            bad = B.walk("20M3D", last, n_last - 22, True)
        else:
            bad = B.walk("10M5I16M", 0, 400, False, cut=1)
        for i in range(3):
            B.walk("25M", 0, 600 + 40 * i, i % 2 == 0, {i + 5})
        out.append(make_case("F-" + what, B, {"bad_rows": [bad], "one_column_past": 1}, keep_order=True,
                             refusal="cigar runs past the end of the read or the entry", family="F"))
    return out


# ---- L: the row list -------------------------------------------------------------------------------------------------------
def cases_l():
    """the W rows whose scores alternate 100 / 50, under a threshold of 75 (about half of the rows are in no alignment pair),
    200 (none is: the list is empty) and 0 (every row is)"""
    out = []
    for build in (_w_runs, _w_indels, _w_md_placement, lambda: _w_n_rows(BLOCK + 1)):
        for thr, tag in ((75, "half"), (200, "none"), (0, "all")):
            c = build()
            c.update(name="L-%s-of-%s" % (tag, c["name"]), score_threshold=thr, family="L", claim={"listed": tag})
            out.append(c)
    return out


# ---- T: the text -----------------------------------------------------------------------------------------------------------
class Pairs(Batch):
    """rows without CIGAR for n read pairs (reads u and u + n) over short entries; coordinates are free"""

    def __init__(self, n_pairs, n_entries=4, paired=True, id_len=None):
        Batch.__init__(self, [genome(100 + e, 60) for e in range(n_entries)])
        self.n, self.paired = n_pairs, paired
        for i in range(2 * n_pairs if paired else n_pairs):
            self.read(b"ACGTTGCAAC" * 3)
        self.ids = []
        for i in range(len(self.reads)):
            u = i % n_pairs
            name = b"q%d" % u
            if id_len:
                name = (name + b"x" * id_len(u))[:id_len(u)]
            self.ids.append(name)

    def single(self, u, entry, pos, mate=1, rc=0, score=100, span=30):
        self.row(u + (self.n if mate == 2 else 0), entry, pos - 1, pos - 2 + span, rc, score)

    def both(self, u, entry, pos1, pos2, s1=100, s2=90, span=1, forward_first=True):
        self.row(u, entry, pos1 - 1, pos1 - 2 + span, 0 if forward_first else 1, s1)
        self.row(u + self.n, entry, pos2 - 1, pos2 - 2 + span, 1 if forward_first else 0, s2)


WIDE = (9, 10, 99_999_999, 100_000_000, 999_999_999, 1_000_000_000, 2 ** 31 - 1)


def _t_numbers():
    """POS / PNEXT / TLEN of 1 .. 10 digits with the 9 -> 10 digit steps, TLEN of both signs; AS / XS 0, 9, 10, 65535; XT 1 and
    2^32 - 1"""
    B = Pairs(4 * len(WIDE) + 10, 7)
    u = 0
    for v in WIDE:
        B.both(u, 0, 1, v)                       # TLEN +v: mate 1 at POS 1, mate 2 at POS v
        B.both(u + 1, 1, v, 1)                   # TLEN -v
        B.both(u + 2, 2, v, v)                   # both mates at v: TLEN -1
        B.single(u + 3, 1, v, mate=2, rc=1, span=1)
        u += 4
    for k, (s1, s2) in enumerate(((0, 0), (9, 0), (5, 5), (65535, 0), (0, 65535), (10, 65525), (65535, 1), (99, 1), (255, 0), (255, 1))):
        B.both(u + k, k % 7, 100, 300, s1, s2)   # (65535 + 1 wraps XS to 0; 255 / 256: where a BAM tag widens)
    return make_case("T-pos-tlen-of-1-to-10-digits-as-xs-xt-at-their-widths", B,
                     {"pos_digits": [1, 2, 3, 8, 9, 10], "tlen_digits": [1, 2, 3, 8, 9, 10], "tlen_signs": [-1, 1], "as_digits": [1, 2, 3, 5],
                      "xs_digits": [1, 2, 3, 5], "xt_values": [1, 255, 256, 65535, 65536, 2 ** 32 - 1]}, ids=B.ids,
                     tax_ids=[1, 2 ** 32 - 1, 0, 255, 256, 65535, 65536])


def _t_cigar_numbers():
    """operation lengths and clip lengths of 1 .. 9 digits: a long insertion as the last operation is not checked against the
    read by any implementation, and the clip behind comes from query_end (which may lie far before the read's start); NM takes the
    same widths"""
    B = Batch()
    for d in range(1, 10):
        n = 10 ** (d - 1)
        i = B.walk([(12, "M"), (n, "I")], 0, 50 * d, d % 2 == 0, {3}, ghost_insert=True)
        B.rows[i] = B.rows[i][:8] + (11 - 10 ** d + 10 ** (d - 1),) + B.rows[i][9:]     # the clip behind: 12 - query_end - 1 = 10^d - 10^(d-1)
    for k, n in enumerate((254, 255, 65534, 65535)):               # NM 255 / 256 / 65535 / 65536: where a BAM tag widens
        B.walk([(12, "M"), (n, "I")], 0, 1000 + 50 * k, k % 2 == 1, {3}, ghost_insert=True)
    B.walk("30M", 0, 700, False, {1}, clip=(9, 0))
    B.walk("30M", 0, 760, True, {1}, clip=(10, 0))
    B.walk("30M", 0, 820, False, {1}, clip=(99, 100))
    return make_case("T-operation-and-clip-lengths-of-1-to-9-digits", B, {"widest_operation_digits": 9, "widest_clip_digits": 9, "widest_nm_digits": 9},
                     keep_order=True)


def _t_ids():
    """ids of 1 .. 17 and 300 bytes: lines start at every phase of the 8-byte sink"""
    lens = list(range(1, 18)) + [300]
    B = Pairs(len(lens), 2, id_len=lambda u: lens[u])
    for u in range(len(lens)):
        B.both(u, u % 2, 10 + u, 200 + 3 * u, span=30)
    return make_case("T-ids-of-1-to-17-and-300-bytes", B, {"id_lengths": lens}, ids=B.ids)


def _t_empty(where):
    """read pairs that end without a record (their rows are under the threshold): first, last, between others, a block of 256,
    all of them.  The device's groups are dense, as the host's: a read pair without records has no group"""
    n = 600
    B = Pairs(n, 2)
    dead = {"first": {0}, "last": {n - 1}, "between": set(range(1, n - 1, 2)), "block-of-256": set(range(256, 512)),
            "first-block-of-256": set(range(0, 256)), "all": set(range(n))}[where]
    for u in range(n):
        s = 20 if u in dead else 100
        if u % 5 == 4 and u not in dead:
            continue                                        # no rows at all
        B.both(u, u % 2, 10 + u, 300 + u, s, s, span=30)
    alive = len([u for u in range(n) if u not in dead and u % 5 != 4])
    return make_case("T-read-pairs-without-records-%s" % where, B, {"read_pairs_out": alive, "text_is_empty": int(alive == 0)}, ids=B.ids,
                     score_threshold=60)


def _t_zero_count(where):
    """groups whose count is 0, first, last, between others, as a block of 256 and all of them.  The one public way to them:
    the pseudo-assembly stage alone (every record a chain of one: its score stays) and its score screen with a fraction of
    1.5, which leaves nothing of a group whose best score is above 0 and everything of a group whose scores are all 0"""
    n = 600
    B = Pairs(n, 2)
    dead = {"first": {0}, "last": {n - 1}, "between": set(range(1, n - 1, 2)), "block-of-256": set(range(256, 512)),
            "first-block-of-256": set(range(0, 256)), "all": set(range(n))}[where]
    groups = 0
    for u in range(n):
        if u % 5 == 4 and u not in dead:
            continue                                        # no rows at all: no group
        s = 50 if u in dead else 0
        B.both(u, u % 2, 1000 * u + 10, 1000 * u + 300, s, s, span=30)
        groups += 1
    return make_case("T-groups-with-count-0-%s" % where, B, {"groups": groups, "groups_with_count_0": len(dead),
                                                             "text_is_empty": int(len(dead) == n)}, ids=B.ids, stages=4, score_fraction=1.5)


def _t_n_pairs(n):
    B = Pairs(n, 3)
    for u in range(n):
        if u % 3 == 0:
            B.both(u, u % 3, 10 + u, 250 + u, 100 + u % 7, 90, span=30)
        elif u % 3 == 1:
            B.single(u, 1, 40 + u, mate=1, rc=u % 2, score=80 + u % 9)
        else:
            B.single(u, 2, 40 + u, mate=2, rc=u % 2, score=80 + u % 9)
    return make_case("T-%d-read-pairs" % n, B, {"read_pairs_out": n}, ids=B.ids)


GROUP_SIZES = (1, 16, 17, 33, 200)


def _t_groups(num_alignments, sam_xa=False, paired=True):
    """read pairs of 1 / 16 / 17 / 33 / 200 alignment pairs with many tied combined scores (the per-pair std::sort permutes
    from 17 on), rows with mate 1 only, mate 2 only and both mixed inside one group"""
    B = Pairs(len(GROUP_SIZES) + 1, max(GROUP_SIZES), paired=paired)
    for u, k in enumerate(GROUP_SIZES):
        for e in range(k):
            kind = (e + u) % 4 if paired else 1
            s = 100 + (e * 7) % 3                      # three distinct scores: ties everywhere
            if kind in (0, 3):
                B.both(u, e, 5 + e, 40 + e, s, s - 10, span=20, forward_first=kind == 0)
            elif kind == 1:
                B.single(u, e, 5 + e, mate=1, rc=e % 2, score=2 * s - 10, span=20)
            else:
                B.single(u, e, 5 + e, mate=2, rc=e % 2, score=2 * s - 10, span=20)
    name = "T-groups-of-1-16-17-33-200-%s-num-alignments-%d%s" % ("paired" if paired else "single-end", num_alignments, "-xa" if sam_xa else "")
    return make_case(name, B, {"group_sizes": list(GROUP_SIZES), "distinct_scores_largest_group": 3}, ids=B.ids, num_alignments=num_alignments,
                     sam_xa=sam_xa, paired=paired)


def _t_x0():
    """255 / 256 / 257 reported rows of one mate: X0 at the widths of a BAM tag"""
    B = Pairs(3, 257)
    for u, k in enumerate((255, 256, 257)):
        for e in range(k):
            B.single(u, e, 5 + e % 9, mate=1 + u % 2, rc=e % 2, score=100 + (e * 5) % 4, span=20)
    return make_case("T-x0-of-255-256-257", B, {"x0_values": [255, 256, 257]}, ids=B.ids, num_alignments=500)


def _t_report_cigar_off():
    c = _w_indels()
    c.update(name="T-report-cigar-off", report_cigar=False, family="T", claim={"cigar_columns": [b"*"]})
    return c


def _mismatch_row(B, k, at, rc=False, qual=None, entry=0, n=100):
    """a row of n columns whose first k mismatch, phred 93 throughout"""
    return B.walk("%dM" % n, entry, at, rc, set(range(k)), fill=Q93, qual=qual, score=100)


def _t_mapq():
    """the mapping-quality plan: a mate with one reported row of 32 / 33 / 34 / 35 phred-93 mismatches (log-probability above
    the bar, below it, 10^logp denormal, 10^logp zero), and a mate with two reported rows that both underflow (their sum is 0)"""
    g = genome(7, 2000)
    B, claim = Batch([g, g]), {}                                       # two equal entries: one read aligns to both
    for k in (32, 33, 34, 35):
        i = _mismatch_row(B, k, 100 + 10 * k, rc=k % 2 == 1)
        claim["logp_of_row_%d" % i] = {32: "above_bar", 33: "normal", 34: "denormal", 35: "zero"}[k]
    B.read(b"ACGT" * 10)                                               # read 4: no rows
    i = _mismatch_row(B, 35, 700)                                      # read 5: two rows of 35 mismatches
    j = B.row(B.rows[i][0], 1, 700, 799, 0, 100, cigar=[(100, "M")])
    claim["logp_of_row_%d" % i] = claim["logp_of_row_%d" % j] = "zero"
    claim["reported_rows_of_read_5"] = 2
    for _ in range(6):                                                 # the mates 2: no rows
        B.read(b"ACGT" * 10)
    return make_case("T-mapping-quality-at-the-bar-of-minus-300", B, claim, keep_order=True)


def _t_bad_quality(needed):
    """a quality byte outside phred+33 0 .. 99 in an aligned column of a row whose probability is needed (the read has two
    reported rows: refused with the host's message) or not (one row: the text is written)"""
    B = Batch([genome(7, 2000), genome(7, 2000)])            # two equal entries: one read aligns to both
    B.walk("40M", 0, 50, False, {7}, score=100)
    i = B.walk("40M", 0, 200, False, {3}, qual={11: 133}, score=100)
    if needed:
        B.row(B.rows[i][0], 1, 200, 239, 0, 100, cigar=[(40, "M")])
    B.walk("40M", 0, 400, True, {9}, score=100)
    B.read(b"ACGT" * 10)
    if len(B.reads) % 2:
        B.read(b"ACGT" * 10)
    return make_case("T-quality-133-on-a-row-whose-probability-is-%s" % ("needed" if needed else "not-needed"), B,
                     {"flagged_rows": 2 if needed else 1, "rows_of_the_flagged_read": 2 if needed else 1}, oracle=False,
                     refusal="quality character outside phred+33 0..99" if needed else None, keep_order=True)


def _t_bad_quality_below_the_bar():
    """one reported row of 33 phred-93 mismatches (log-probability between -310 and -300: below the bar, 10^logp is evaluated)
    with a quality byte outside the tables in an aligned column: refused, although the mate has no second row"""
    g = genome(7, 2000)
    B = Batch([g, g])
    B.walk("40M", 0, 50, False, {7}, score=100)
    i = _mismatch_row(B, 33, 300, qual={70: 133})
    B.walk("40M", 0, 600, True, {9}, score=100)
    B.read(b"ACGT" * 10)
    return make_case("T-quality-133-on-a-lone-row-below-the-bar", B, {"flagged_rows": 1, "rows_of_the_flagged_read": 1,
                                                                     "logp_of_row_%d" % i: "normal"}, oracle=False,
                     refusal="quality character outside phred+33 0..99", keep_order=True)


def _t_genes(with_genes=True):
    """best_gene: two genes sharing the same width with the span (the first wins), a gene touching but not overlapping, each of
    name / protein / product empty, an entry without genes, an index without any gene"""
    B = Pairs(8, 5)
    for u in range(8):
        B.single(u, u % 5, 101, mate=1 + u % 2, rc=u % 2, span=100)      # span 100 .. 199 (0-based, ref_end inclusive)
    genes = [[(50, 150, b"first", b"P1", b"wins the tie"), (149, 300, b"second", b"P2", b"loses")],
             [(199, 300, b"touches", b"P3", b"shares nothing")],
             [(0, 120, b"", b"P4", b"no name"), (300, 400, b"far", b"", b"")],
             [],
             [(150, 400, b"name", b"", b""), (0, 110, b"short", b"P6", b"ten bases")]] if with_genes else None
    claim = {"xg_values": [b"first", b"name"], "mapped_lines_without_gene_tags": 3} if with_genes else {"xg_values": [], "mapped_lines_without_gene_tags": 8}
    return make_case("T-genes-tie-touching-empty-columns" if with_genes else "T-index-without-any-gene", B, claim, ids=B.ids, genes=genes)


def cases_t():
    out = [_t_numbers(), _t_cigar_numbers(), _t_ids()]
    out += [_t_zero_count(w) for w in ("first", "last", "between", "block-of-256", "first-block-of-256", "all")]
    out += [_t_empty(w) for w in ("between", "all")]
    out += [_t_n_pairs(n) for n in (1, BLOCK - 1, BLOCK, BLOCK + 1)]
    out += [_t_groups(na) for na in (0, 1, 17, 200, 500)]
    out += [_t_x0(), _t_groups(10, sam_xa=True), _t_groups(1, sam_xa=True), _t_groups(33, paired=False), _t_report_cigar_off()]
    out += [_t_mapq(), _t_bad_quality(True), _t_bad_quality(False), _t_bad_quality_below_the_bar(), _t_genes(True), _t_genes(False)]
    return out


# ---- X: the lowest common ancestor -----------------------------------------------------------------------------------------
X_TAXDB = [(1, 1, b"root", b"no rank"), (2, 1, b"Bacteria", b"superkingdom"), (20, 2, b"Genus", b"genus"), (200, 20, b"Species a", b"species"),
           (201, 20, b"Species b", b"species"), (2000, 200, b"Strain", b"strain"), (3, 1, b"Viruses", b"superkingdom"), (30, 3, b"Virus", b"species"),
           (5000, 0, b"another root", b"no rank"), (5001, 5000, b"Other", b"superkingdom"), (5002, 5001, b"Other species", b"species")]
X_ENTRY_TAX = [200, 200, 2000, 201, 30, 1, 0, 777777, 777777, 888888, 5002, 20, 2, 5000]
X_SETS = [("single-entry", [0]), ("same-node-twice", [0, 1]), ("parent-and-child", [0, 2]), ("child-and-parent", [2, 0]), ("siblings", [0, 3]),
          ("different-depths", [2, 3]), ("different-depths-reversed", [3, 2]), ("strain-and-superkingdom", [2, 12]), ("across-superkingdoms", [0, 4]),
          ("the-root", [5]), ("the-root-and-a-species", [5, 0]), ("id-0-first", [6, 0]), ("id-0-later", [0, 3, 6]), ("id-0-alone", [6]),
          ("unknown-alone", [7]), ("unknown-twice-the-same", [7, 8]), ("unknown-twice-different", [7, 9]), ("unknown-then-known", [7, 0]),
          ("known-then-unknown", [0, 7]), ("known-unknown-known", [0, 7, 3]), ("two-roots", [0, 10]), ("the-other-tree", [10]),
          ("the-other-root-and-its-leaf", [13, 10]), ("three-way", [0, 3, 2]), ("genus-and-species", [11, 3])]
X_SETS.insert(9, ("no-rows", []))


def cases_x():
    """one read pair per entry set; the records' scores fall along the set, so after writeSAMOutputPairs' sort they stand in
    the order the set is written in"""
    B = Pairs(len(X_SETS), len(X_ENTRY_TAX))
    for u, (_, es) in enumerate(X_SETS):
        for k, e in enumerate(es):
            B.single(u, e, 3 + u, mate=1 + (u + k) % 2, rc=k % 2, score=200 - 10 * k, span=20)
    return [make_case("X-every-branch-of-the-lca", B, {"sets": len(X_SETS), "lines": len(X_SETS) - 1}, ids=B.ids, tax_ids=X_ENTRY_TAX, taxdb=X_TAXDB)]


def all_cases():
    return {"W": cases_w(), "F": cases_f(), "L": cases_l(), "T": cases_t(), "X": cases_x()}
