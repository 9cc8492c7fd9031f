"""The consensus caller of include/kslam_consensus.h, restated in plain Python from the header's text by another method than the
library's: dense per-position counters for every entry and a dictionary of insertion strings per anchor -- no keys, no sorting, no
searches.  Also the writer of the FASTA bytes, and the builders of the cases the host twin and the device are held to (on
tests/variants_ref.py's Builder).  Shares no code with host/consensus.cpp.

A case is variants_ref's dict: name, gbases / goff, rbases / roff, pool, ov / rp / pr."""
import numpy as np

from variants_ref import ACGT, NO_OVERLAP, OVERLAP_DT, PAIRED_OVERLAP_DT, READ_PAIR_DT, Builder, arrays, concat, other_base, random_bases, random_case, reverse_complement  # noqa: F401

STAT_NAMES = ("n_records", "n_skipped", "n_intervals", "n_del_intervals", "n_events", "n_insertions", "n_ins_unanchored",
              "n_ins_unrepresentable", "n_entries_touched", "n_entries_reported")
ROW_NAMES = ("entry", "seq_off", "seq_len", "entry_len", "covered", "substitutions", "deleted", "insertions", "inserted_bases", "ambiguous")
FILL_N, FILL_REF = 0, 1
MAX_INS = 32
DEFAULTS = (1, 500, FILL_N, 1)
# the parameter sets every case is called with: the defaults, a depth floor, a stricter call with REF fill, a coverage floor
PARAMS = (DEFAULTS, (2, 500, FILL_N, 1), (1, 750, FILL_REF, 1), (1, 500, FILL_REF, 30), (3, 999, FILL_N, 0))


# ---------------------------------------------------------------- the definition

def consensus(case, min_depth=1, call_permille=500, fill=FILL_N, min_covered=1):
    """-> (rows: list of dicts by ROW_NAMES, seqs: list of bytes, stats: dict)"""
    assert min_depth >= 1 and 500 <= call_permille <= 999 and fill in (FILL_N, FILL_REF)
    ov, rp, pr, goff, roff = case["ov"], case["rp"], case["pr"], case["goff"], case["roff"]
    n_entries = len(goff) - 1
    named = set()
    for g in rp:
        live = pr[int(g["first"]):int(g["first"]) + int(g["count"])]
        for f in ("r1", "r2"):
            named.update(int(i) for i in live[f] if int(i) != NO_OVERLAP)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["n_records"] = len(named)
    lens = [int(goff[e + 1] - goff[e]) for e in range(n_entries)]
    m = [np.zeros(n, dtype=np.int64) for n in lens]
    dl = [np.zeros(n, dtype=np.int64) for n in lens]
    votes = [np.zeros((n, 5), dtype=np.int64) for n in lens]       # the query bytes that DIFFER from the entry's, by code
    touched = [False] * n_entries
    inserted = {}                                                   # (entry, anchor) -> {string: count}
    for i in sorted(named):
        o = ov[i]
        entry, read, ref_begin, cigar_len = int(o["entry"]), int(o["read"]), int(o["ref_begin"]), int(o["cigar_len"])
        if entry >= n_entries or cigar_len == 0 or ref_begin < 0:
            stats["n_skipped"] += 1
            continue
        ref = case["gbases"][int(goff[entry]):int(goff[entry + 1])].tobytes()
        query = case["rbases"][int(roff[read]):int(roff[read + 1])].tobytes()
        if int(o["revcomp"]) != 0:
            query = reverse_complement(query)
        ops = [(int(c) >> 4, int(c) & 15) for c in case["pool"][int(o["cigar_off"]):int(o["cigar_off"]) + cigar_len]]
        r, q = ref_begin, max(int(o["query_begin"]), 0)
        for n, op in ops:      # the whole CIGAR first
            r, q = r + (n if op in (0, 2) else 0), q + (n if op in (0, 1) else 0)
            if r > len(ref) or q > len(query):
                break
        else:
            r, q = ref_begin, max(int(o["query_begin"]), 0)
            for n, op in ops:
                if op == 0:
                    if n:
                        stats["n_intervals"] += 1
                        touched[entry] = True
                    for j in range(n):
                        m[entry][r + j] += 1
                        if query[q + j] != ref[r + j]:
                            code = ACGT.find(bytes([query[q + j]]))
                            votes[entry][r + j][code if code >= 0 else 4] += 1
                            stats["n_events"] += 1
                    r, q = r + n, q + n
                elif op == 1:
                    if n:
                        run = query[q:q + n]
                        if r == ref_begin:
                            stats["n_ins_unanchored"] += 1
                        elif n > MAX_INS or any(b not in ACGT for b in run):
                            stats["n_ins_unrepresentable"] += 1
                        else:
                            at = inserted.setdefault((entry, r - 1), {})
                            at[run] = at.get(run, 0) + 1
                            stats["n_insertions"] += 1
                    q += n
                elif op == 2:
                    if n:
                        stats["n_del_intervals"] += 1
                        touched[entry] = True
                    dl[entry][r:r + n] += 1
                    r += n
            continue
        stats["n_skipped"] += 1
    rows, seqs, off = [], [], 0
    for e in range(n_entries):
        if not touched[e]:
            continue
        stats["n_entries_touched"] += 1
        ref = case["gbases"][int(goff[e]):int(goff[e + 1])].tobytes()
        row = dict.fromkeys(ROW_NAMES, 0)
        row["entry"], row["entry_len"] = e, lens[e]
        out = bytearray()
        for pos in range(lens[e]):
            d = int(m[e][pos] + dl[e][pos])
            if d < min_depth:
                out.append(ref[pos] if fill == FILL_REF else ord("N"))
                continue
            row["covered"] += 1
            refc = int(m[e][pos] - votes[e][pos].sum())
            won = [b for k, b in enumerate(ACGT) if (int(votes[e][pos][k]) + (refc if ref[pos] == b else 0)) * 1000 > d * call_permille]
            gone = int(dl[e][pos]) * 1000 > d * call_permille
            assert len(won) + gone <= 1
            if won:
                out.append(won[0])
                row["substitutions"] += won[0] != ref[pos]
            elif gone:
                row["deleted"] += 1
            else:
                out.append(ord("N"))
                row["ambiguous"] += 1
            passing = [(len(s), s) for s, c in inserted.get((e, pos), {}).items() if c * 1000 > d * call_permille]
            if passing:
                n, s = min(passing)
                out += s
                row["insertions"] += 1
                row["inserted_bases"] += n
        if row["covered"] < max(min_covered, 1):
            continue
        row["seq_off"], row["seq_len"] = off, len(out)
        off += len(out)
        rows.append(row)
        seqs.append(bytes(out))
    stats["n_entries_reported"] = len(rows)
    return rows, seqs, stats


def fields(rows):
    """library rows (a structured array) or restated rows (dicts) as tuples without the padding"""
    return [tuple(int(r[n]) for n in ROW_NAMES) for r in rows]


def split(rows, seq):
    """the library's one byte array as a list of sequences"""
    return [bytes(seq[int(r["seq_off"]):int(r["seq_off"]) + int(r["seq_len"])]) for r in rows]


# ---------------------------------------------------------------- the file

def fasta_bytes(rows, seqs, loci):
    out = []
    for r, s in zip(rows, seqs):
        out.append(b">%s kslam_consensus entry_length=%d covered=%d substitutions=%d deletions=%d insertions=%d ambiguous=%d\n" % (
            loci[int(r["entry"])], int(r["entry_len"]), int(r["covered"]), int(r["substitutions"]), int(r["deleted"]), int(r["insertions"]),
            int(r["ambiguous"])))
        out += [s[at:at + 60] + b"\n" for at in range(0, len(s), 60)]
    return b"".join(out)


# ---------------------------------------------------------------- the cases

class CB(Builder):
    def gapped(self, entry, ref_begin, ops, revcomp=0, ins=(), mismatch_at=(), subs=None):
        """as aligned(), with the bases of the I runs given: ins[k] are the bytes of the k-th I run"""
        q, at, k, put = 0, dict(subs or {}), 0, list(ins)
        for n, op in ops:
            if op == "I":
                for j in range(n):
                    at[q + j] = put[k][j]
                k += 1
            if op != "D":
                q += n
        query = bytearray(self.query(entry, ref_begin, ops))
        for x in mismatch_at:
            query[x] = other_base(query[x])
        for x, b in at.items():
            query[x] = b
        read = self.read(reverse_complement(query) if revcomp else bytes(query))
        return self.rec(read, entry, ref_begin, self.cigar(ops), revcomp)

    def times(self, n, *a, **kw):
        for _ in range(n):
            self.single(self.gapped(*a, **kw))


def listed(name, n, skip_at=None):
    """n listed records, one per group; record skip_at runs past its entry"""
    rng = np.random.default_rng(n)
    b = CB(name, [random_bases(rng, 90), random_bases(rng, 70)])
    for k in range(n):
        e = k & 1
        if k == skip_at:
            b.single(b.rec(b.read(b.entries[e][:40]), e, len(b.entries[e]) - 39, b.cigar([(40, "M")])))
        elif k % 5 == 0:
            b.single(b.gapped(e, k % 20, [(12, "M"), (2, "I"), (10, "M"), (1, "D"), (9, "M")], k % 3 == 0, ins=[b"GT"], mismatch_at=(k % 12,)))
        else:
            b.single(b.gapped(e, k % 30, [(33, "M")], k % 3 == 0, mismatch_at=(k % 33,)))
    return b.done()


def cases():
    rng = np.random.default_rng(20261)
    out = []
    base = random_bases(rng, 300)
    # ---- walk
    for rc in (0, 1):
        s = "rev" if rc else "fwd"
        b = CB("walk-m-runs-" + s, [base])
        for n in (15, 16, 17, 31, 32, 33):      # both sides of the 16-column chunks
            b.single(b.gapped(0, 40 + n, [(n, "M")], rc, mismatch_at=sorted({0, n - 1, n // 2})))
            b.single(b.gapped(0, 5, [(n, "M"), (2, "D"), (n, "M")], rc, mismatch_at=(n - 1, n, 2 * n - 1)))
        out.append(b.done())
    b = CB("walk-rev-first-read", [base])            # the batch's first read, 10 bases, reverse strand: the chunk's load would
    b.single(b.gapped(0, 100, [(10, "M")], 1, mismatch_at=(0, 9)))   # begin before the array
    b.single(b.gapped(0, 95, [(3, "M"), (1, "I"), (6, "M")], 1, ins=[b"C"]))
    out.append(b.done())
    for n, ins in ((1, b"G"), (32, random_bases(rng, 32)), (33, random_bases(rng, 33))):
        for rc in (0, 1):
            b = CB("walk-ins-%d-%s" % (n, "rev" if rc else "fwd"), [base])
            b.times(3, 0, 50, [(20, "M"), (n, "I"), (20, "M")], rc, ins=[ins])
            b.times(1, 0, 40, [(60, "M")], 1 - rc)
            out.append(b.done())
    for tag, ins in (("N", b"ANG"), ("lower", b"AcG")):
        b = CB("walk-ins-" + tag, [base])
        b.times(2, 0, 50, [(20, "M"), (3, "I"), (20, "M")], 0, ins=[ins])
        b.times(2, 0, 50, [(20, "M"), (3, "I"), (20, "M")], 1, ins=[ins])
        b.times(1, 0, 50, [(20, "M"), (3, "I"), (20, "M")], 1, ins=[b"ATG"])
        out.append(b.done())
    b = CB("walk-ins-first", [base])                 # unanchored: also behind zero-length M and D runs, which consume nothing
    b.times(2, 0, 50, [(2, "I"), (30, "M")], 0, ins=[b"GG"])
    b.times(2, 0, 50, [(0, "M"), (0, "D"), (2, "I"), (30, "M")], 1, ins=[b"GG"])
    out.append(b.done())
    b = CB("walk-ins-after-del", [base])
    b.times(3, 0, 50, [(10, "M"), (2, "D"), (3, "I"), (10, "M")], 0, ins=[b"TGA"])
    b.times(1, 0, 45, [(30, "M")], 1)
    out.append(b.done())
    b = CB("walk-two-ins", [base])                   # two I runs in a row: two insertions at one anchor
    b.times(3, 0, 50, [(10, "M"), (2, "I"), (3, "I"), (10, "M")], 0, ins=[b"CA", b"TTT"])
    b.times(3, 0, 120, [(10, "M"), (2, "I"), (2, "I"), (10, "M")], 1, ins=[b"GA", b"CT"])   # both pass: the string that sorts first
    b.times(3, 0, 160, [(10, "M"), (2, "I"), (2, "I"), (10, "M")], 0, ins=[b"GA", b"GA"])   # the same pair twice per read
    out.append(b.done())
    b = CB("walk-del-to-end", [base])
    b.times(2, 0, 285, [(10, "M"), (5, "D")], 0)
    b.times(1, 0, 280, [(20, "M")], 1)
    out.append(b.done())
    b = CB("walk-zero-ops", [base])
    ops = [(0, "M"), (10, "M"), (0, "I"), (0, "D"), (5, "M"), (0, "D"), (2, "I"), (0, "I"), (8, "M"), (0, "M")]
    b.times(2, 0, 30, ops, 0, ins=[b"", b"AC", b""], mismatch_at=(0, 14, 24))
    b.times(1, 0, 30, ops, 1, ins=[b"", b"AC", b""])
    out.append(b.done())
    # ---- alphabet
    e = bytearray(random_bases(rng, 120))
    e[10:16] = b"NNaNgt"
    b = CB("alphabet", [bytes(e)])
    b.times(3, 0, 0, [(60, "M")], 0, subs={10: ord("C"), 12: ord("A"), 14: ord("g"), 15: ord("T"), 30: ord("N"), 31: ord("n")})   # N filled in by
    b.times(1, 0, 0, [(60, "M")], 1, subs={10: ord("C"), 11: ord("N"), 12: ord("a"), 30: ord("N")})   # the reads; N over N; lower case
    b.times(2, 0, 40, [(60, "M")], 1, subs={5: ord("N"), 6: ord("N")})
    out.append(b.done())
    # ---- entries
    ents = [b"", random_bases(rng, 1), random_bases(rng, 50), b"", random_bases(rng, 40), random_bases(rng, 64), b"", random_bases(rng, 33)]
    b = CB("entries", ents)
    b.times(2, 1, 0, [(1, "M")], 0, mismatch_at=(0,))                    # an entry of one base
    b.times(2, 2, 40, [(10, "M"), (2, "I")], 0, ins=[b"GC"])             # an insertion anchored at the last base of entry 2 ...
    b.times(2, 4, 0, [(20, "M")], 1, mismatch_at=(0,))                   # ... and reads from base 0 of the next entry with bases
    b.times(1, 5, 10, [(30, "M")], 0)                                    # touched, depth 1: not reported under min_depth = 2
    b.times(2, 7, 13, [(20, "M")], 1, mismatch_at=(19,))                 # the last base of the last entry
    b.times(2, 7, 30, [(1, "M"), (2, "D")], 0)                           # ... deleted by as many
    out.append(b.done())
    # ---- the call
    b = CB("call", [base])
    for k in range(4):       # at 60: 2 of 4; at 70: 3 of 4; at 80: 4 of 4
        b.times(1, 0, 50, [(50, "M")], k & 1, mismatch_at=[x for x, n in ((10, 2), (20, 3), (30, 4)) if k < n])
    for k in range(4):       # at 150 .. 152: deletion by 3 of 4; at 170: by 2 of 4
        ops = [(10, "M"), (3, "D"), (17, "M"), (1, "D"), (19, "M")] if k < 2 else [(10, "M"), (3, "D"), (37, "M")] if k < 3 else [(50, "M")]
        b.times(1, 0, 140, ops, k & 1)
    for k in range(4):       # at 209: a deletion and an insertion by 3 of 4; at 230: two insertions, two reads each
        ops = [(8, "M"), (2, "D"), (2, "I"), (20, "M"), (2, "I"), (20, "M")]
        if k < 3:
            b.times(1, 0, 200, ops, k & 1, ins=[b"AG", b"AA" if k < 2 else b"CC"])
        else:
            b.times(1, 0, 200, [(30, "M"), (2, "I"), (20, "M")], k & 1, ins=[b"CC"])
    out.append(b.done())
    b = CB("call-5000", [base])          # one site under 5 000 records: 2 600 with a substitution and an insertion, 2 400 plain
    first = b.gapped(0, 100, [(20, "M"), (4, "I"), (20, "M")], 0, ins=[b"ACGT"], mismatch_at=(7,))
    plain = b.gapped(0, 100, [(40, "M")], 1)
    for k in range(5000):
        src = b.ov[first if k < 2600 else plain]
        b.single(b.rec(src[0], 0, 100, (src[5], src[6]), src[3]))
    out.append(b.done())
    # ---- the grid
    for n in (63, 64, 65, 255, 256, 257):
        out.append(listed("grid-%d" % n, n))
    out.append(listed("grid-skip-in-wave", 128, skip_at=30))
    # ---- everything at once
    out.append(random_case("random-900", 501, 900, 9, 300))
    out.append(random_case("random-0", 502, 0, 3, invalid=False))
    return out


# ---------------------------------------------------------------- planted truth

def planted(seed=2027, length=6000, read_len=100, fold=30):
    """an entry of random bases and a copy with substitutions every 200 bases, one 3-base deletion and one 2-base insertion, each
    placed where no other placement of the gap gives the same two sequences (the bases around it differ), and error-free reads of
    the copy on both strands -> (entry, copy, substitutions, reads)"""
    rng = np.random.default_rng(seed)
    entry = bytearray(random_bases(rng, length))
    d, a = 2100, 3900
    # the deletion of entry[d .. d + 3) cannot slide: the base before differs from its last base, the base behind from its first
    entry[d - 1], entry[d], entry[d + 1], entry[d + 2], entry[d + 3] = b"ACGTG"
    # the insertion "GT" behind entry[a] cannot slide either: entry[a] is not T, entry[a + 1] is not G
    entry[a], entry[a + 1] = b"AC"
    entry = bytes(entry)
    copy, n_subs = bytearray(entry), 0
    for pos in range(500, length - 400, 200):
        if abs(pos - d) > 50 and abs(pos - a) > 50:
            copy[pos] = other_base(entry[pos], 1 + int(rng.integers(0, 3)))
            n_subs += 1
    copy = bytes(copy[:d]) + bytes(copy[d + 3:a + 1]) + b"GT" + bytes(copy[a + 1:])
    reads = []
    for _ in range(fold * length // read_len):
        at = int(rng.integers(0, len(copy) - read_len + 1))
        q = copy[at:at + read_len]
        reads.append(reverse_complement(q) if rng.random() < 0.5 else q)
    return entry, copy, n_subs, reads
