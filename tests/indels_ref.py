"""The indel table of include/kslam_indels.h, restated in plain Python from the header's text (byte strings, a dictionary of
keys and a difference array of depth per entry), the builder of the cases the host twin and the device are held to, and a writer
of the VCF bytes.  Shares no code with host/indels.cpp; the builder of batches is tests/variants_ref.py's.

A row is a tuple (entry, pos, kind, len, bases, alt_fwd, alt_rev, depth); bases is the inserted text (b"" for a deletion) here
and a packed number in the library's rows (fields() turns those into these)."""
import numpy as np

import variants_ref as V
from variants_ref import Builder, random_bases, reverse_complement  # noqa: F401

STAT_NAMES = ("n_records", "n_skipped", "n_intervals", "n_deletions", "n_insertions", "n_unanchored", "n_long_del", "n_unrepresentable", "n_sites")
ACGT = b"ACGT"
MAX_DEL, MAX_INS, DEL, INS = 65536, 32, 0, 1
INFO_LINES = [
    b'##INFO=<ID=DP,Number=1,Type=Integer,Description="Aligned reads with a match or mismatch column at the anchor">\n',
    b'##INFO=<ID=AO,Number=A,Type=Integer,Description="Alternate allele observations">\n',
    b'##INFO=<ID=SAF,Number=A,Type=Integer,Description="Alternate allele observations on the forward strand">\n',
    b'##INFO=<ID=SAR,Number=A,Type=Integer,Description="Alternate allele observations on the reverse strand">\n',
    b'##INFO=<ID=AF,Number=A,Type=Float,Description="Alternate allele observations over depth (not clamped)">\n',
    b'##INFO=<ID=TYPE,Number=A,Type=String,Description="del or ins">\n',
    b'##INFO=<ID=LEN,Number=A,Type=Integer,Description="Deleted or inserted bases">\n']
COLUMNS = V.COLUMNS
concat_cases = V.concat      # two cases over the same entries as one batch


# ---------------------------------------------------------------- the definition

def normalise_deletion(ref, p, n):
    """the leftmost equivalent position of the deletion of ref[p:p + n]"""
    while p >= 2 and ref[p - 1] == ref[p + n - 1] and ref[p - 1] in ACGT:
        p -= 1
    return p


def normalise_insertion(ref, p, s):
    """... of the insertion of s (upper-case ACGT alone) in front of ref[p] -> (p, s rotated)"""
    while p >= 2 and ref[p - 1] == s[-1]:
        s = s[-1:] + s[:-1]
        p -= 1
    return p, s


def raw_events(case, o):
    """one overlap record -> None when it is skipped, else (intervals [(begin, end)], events [(kind, p, len, bases)] as the walk
    meets them, tallies {name: n})"""
    read, entry, ref_begin, query_begin = int(o["read"]), int(o["entry"]), int(o["ref_begin"]), int(o["query_begin"])
    cigar_off, cigar_len = int(o["cigar_off"]), int(o["cigar_len"])
    goff, roff = case["goff"], case["roff"]
    if entry >= len(goff) - 1 or cigar_len == 0 or ref_begin < 0:
        return None
    ref_len = int(goff[entry + 1]) - int(goff[entry])
    query = case["rbases"][int(roff[read]):int(roff[read + 1])].tobytes()
    if int(o["revcomp"]):
        query = reverse_complement(query)
    ops = [(int(c) >> 4, int(c) & 15) for c in case["pool"][cigar_off:cigar_off + cigar_len]]
    rp, qp = ref_begin, max(query_begin, 0)
    for n, op in ops:      # the whole CIGAR first
        if op == 0:
            rp, qp = rp + n, qp + n
        elif op == 1:
            qp += n
        elif op == 2:
            rp += n
        if rp > ref_len or qp > len(query):
            return None
    intervals, events, tallies = [], [], dict.fromkeys(("n_unanchored", "n_long_del", "n_unrepresentable"), 0)
    rp, qp = ref_begin, max(query_begin, 0)
    for n, op in ops:
        if op == 0:
            if n > 0:
                intervals.append((rp, rp + n - 1))
            rp, qp = rp + n, qp + n
        elif op == 1:
            s = query[qp:qp + n]
            if n > 0:
                if rp <= ref_begin:
                    tallies["n_unanchored"] += 1
                elif n > MAX_INS or any(b not in ACGT for b in s):
                    tallies["n_unrepresentable"] += 1
                else:
                    events.append((INS, rp, n, s))
            qp += n
        elif op == 2:
            if n > 0:
                if rp <= ref_begin:
                    tallies["n_unanchored"] += 1
                elif n > MAX_DEL:
                    tallies["n_long_del"] += 1
                else:
                    events.append((DEL, rp, n, b""))
            rp += n
    return intervals, events, tallies


def entry_bytes(case, e):
    return case["gbases"][int(case["goff"][e]):int(case["goff"][e + 1])].tobytes()


def normalised(ref, kind, p, n, s):
    """-> the key's (anchor, kind, len, bases)"""
    if kind == DEL:
        return (normalise_deletion(ref, p, n) - 1, DEL, n, b"")
    p, s = normalise_insertion(ref, p, s)
    return (p - 1, INS, n, s)


def table(case, min_alt=1, min_depth=0):
    """-> (rows [tuples], stats dict)"""
    ov, rp, pr = case["ov"], case["rp"], case["pr"]
    n_entries = len(case["goff"]) - 1
    named = set()
    for g in rp:
        live = pr[int(g["first"]):int(g["first"]) + int(g["count"])]
        for f in ("r1", "r2"):
            named.update(int(i) for i in live[f] if int(i) != V.NO_OVERLAP)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["n_records"] = len(named)
    keys = {}
    begins = [[] for _ in range(n_entries)]
    ends = [[] for _ in range(n_entries)]
    refs = {}
    for i in sorted(named):
        o = ov[i]
        got = raw_events(case, o)
        if got is None:
            stats["n_skipped"] += 1
            continue
        intervals, events, tallies = got
        e = int(o["entry"])
        ref = refs.setdefault(e, entry_bytes(case, e))
        for b, t in intervals:
            begins[e].append(b)
            ends[e].append(t)
        stats["n_intervals"] += len(intervals)
        for k, n in tallies.items():
            stats[k] += n
        for kind, p, n, s in events:
            stats["n_deletions" if kind == DEL else "n_insertions"] += 1
            k = keys.setdefault((e,) + normalised(ref, kind, p, n, s), [0, 0])
            k[1 if int(o["revcomp"]) else 0] += 1
    stats["n_sites"] = len(keys)
    depth = {}
    out = []
    for key in sorted(keys):     # bytes of ACGT sort as the packed numbers of equal length do
        e, pos = key[0], key[1]
        if e not in depth:
            d = np.zeros(int(case["goff"][e + 1] - case["goff"][e]) + 1, dtype=np.int64)
            if begins[e]:
                np.add.at(d, np.asarray(begins[e], dtype=np.int64), 1)
                np.add.at(d, np.asarray(ends[e], dtype=np.int64) + 1, -1)
            depth[e] = np.cumsum(d)
        fwd, rev = keys[key]
        dp = int(depth[e][pos])
        if fwd + rev >= min_alt and dp >= min_depth:
            out.append(key + (fwd, rev, dp))
    return out, stats


def fields(rows):
    """the library's rows (kslam_amd.indels.ROW_DT) as this module's tuples"""
    out = []
    for r in rows:
        n = int(r["len"])
        s = bytes(ACGT[(int(r["bases"]) >> (2 * (n - 1 - j))) & 3] for j in range(n)) if int(r["kind"]) == INS else b""
        assert int(r["kind"]) == INS or int(r["bases"]) == 0
        out.append((int(r["entry"]), int(r["pos"]), int(r["kind"]), n, s, int(r["alt_fwd"]), int(r["alt_rev"]), int(r["depth"])))
    return out


def packed(rows, dtype):
    """this module's tuples as the library's rows"""
    out = np.zeros(len(rows), dtype=dtype)
    for i, (e, pos, kind, n, s, fwd, rev, dp) in enumerate(rows):
        w = 0
        for b in s:
            w = (w << 2) | ACGT.index(bytes([b]))
        out[i] = (e, pos, kind, (0, 0, 0), n, w, fwd, rev, dp, 0)
    return out


def apply_allele(ref, anchor, kind, n, s):
    """the haplotype a row's allele gives: the entry with the n bases behind the anchor deleted / s inserted behind the anchor"""
    return ref[:anchor + 1] + ref[anchor + 1 + n:] if kind == DEL else ref[:anchor + 1] + s + ref[anchor + 1:]


# ---------------------------------------------------------------- the file

def vcf_bytes(rows, case_or_entries, loci, source):
    entries = case_or_entries if isinstance(case_or_entries, list) else [entry_bytes(case_or_entries, e) for e in range(len(case_or_entries["goff"]) - 1)]
    out = [b"##fileformat=VCFv4.2\n", b"##source=" + source + b"\n"]
    for e in sorted({r[0] for r in rows}):
        out.append(b"##contig=<ID=%s,length=%d>\n" % (loci[e], len(entries[e])))
    out += INFO_LINES + [COLUMNS]
    for e, pos, kind, n, s, fwd, rev, dp in rows:
        ref = entries[e]
        a = ref[pos:pos + 1]
        r, alt = (ref[pos:pos + 1 + n], a) if kind == DEL else (a, a + s)
        out.append(b"%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AO=%d;SAF=%d;SAR=%d;AF=%s;TYPE=%s;LEN=%d\n" % (
            loci[e], pos + 1, r, alt, dp, fwd + rev, fwd, rev, b"%.6f" % ((fwd + rev) / dp if dp else 0.0), b"del" if kind == DEL else b"ins", n))
    return b"".join(out)


# ---------------------------------------------------------------- the cases

LEFT, RIGHT = b"GTCAGTCTGACTGCATGCTC", b"GTCGATCGTAGCTAGCTTGCAGT"   # flanks that end / begin with no base of the repeats below


def al(b, entry, begin, ops, rc=0, fill=b"A", single=True):
    """an alignment whose I runs read `fill`, as a record in a group of its own; -> the record's index"""
    q = b.query(entry, begin, ops, fill=fill)
    r = b.rec(b.read(reverse_complement(q) if rc else q), entry, begin, b.cigar(ops), rc)
    if single:
        b.single(r)
    return r


def split_at(total, at, op, n):
    """M up to `at` bases into the alignment, the run, M up to `total` reference bases"""
    return [(at, "M"), (n, op), (total - at - (n if op == "D" else 0), "M")]


def grid(n_records):
    """n_records listed records with one event each: one read, one CIGAR"""
    rng = np.random.default_rng(n_records)
    b = Builder("grid-%d" % n_records, [random_bases(rng, 120)])
    first = al(b, 0, 10, [(20, "M"), (1, "D"), (20, "M")])
    for _ in range(1, n_records):
        b.single(b.rec(b.ov[first][0], 0, 10, (b.ov[first][5], b.ov[first][6])))
    return b.done()


def repeat_case(name, unit, copies, del_lens=(), ins_lens=(), left=LEFT, right=RIGHT, before=(), rc_every=3):
    """one entry left + unit * copies + right (behind the entries `before`); every deletion of n bases inside the repeat and every
    insertion of n bases that continues it, at every phase"""
    ref = left + unit * copies + right
    b = Builder(name, list(before) + [ref])
    e, start, span = len(before), len(left), len(unit) * copies
    k = 0
    for n in del_lens:
        for j in range(span - n + 1):
            if start + j >= 1:
                al(b, e, 0, split_at(len(ref), start + j, "D", n), rc=int(k % rc_every == 1))
                k += 1
    for n in ins_lens:
        for j in range(span + 1):
            if start + j >= 1:
                s = ((unit * (copies + n))[j % len(unit):])[:n]     # the repeat's own text from phase j on
                al(b, e, 0, split_at(len(ref), start + j, "I", n), rc=int(k % rc_every == 1), fill=s)
                k += 1
    return b.done()


def alphabet_case():
    ref = LEFT + b"AAAANAAAA" + b"C" + b"TTTTtTTTT" + b"G" + b"CNNG" + RIGHT
    b = Builder("alphabet", [ref])
    n_at, t_at, nn_at = len(LEFT) + 4, len(LEFT) + 10 + 4, len(LEFT) + 20 + 1
    for p in (n_at + 1, n_at + 4, n_at - 1, n_at):           # right of the N (stops at it), left of it, the N itself
        al(b, 0, 0, split_at(len(ref), p, "D", 1))
        al(b, 0, 0, split_at(len(ref), p, "I", 1), fill=b"A")
    for p in (t_at + 1, t_at + 3, t_at):                     # lower case inside a run of T
        al(b, 0, 0, split_at(len(ref), p, "D", 1), rc=1)
        al(b, 0, 0, split_at(len(ref), p, "I", 1), fill=b"T")
    al(b, 0, 0, split_at(len(ref), nn_at + 1, "D", 1))       # the second of two N: equal bytes, no step
    al(b, 0, 0, split_at(len(ref), 30, "I", 1), fill=b"N")   # an inserted N, a lower-case base, one among good ones
    al(b, 0, 0, split_at(len(ref), 30, "I", 1), fill=b"a")
    al(b, 0, 0, split_at(len(ref), 30, "I", 3), fill=b"ANA")
    al(b, 0, 0, split_at(len(ref), 30, "I", 3), fill=b"ANA", rc=1)
    return b.done()


def limits_case():
    rng = np.random.default_rng(5)
    big = random_bases(rng, 70000)
    small = bytearray(random_bases(rng, 200))
    small[50:60] = b"ACGTACCGTA"                             # around position 55 nothing below can be shifted
    b = Builder("limits", [bytes(small), big])
    for n in (1, 32, 33):
        al(b, 0, 20, split_at(60, 30, "I", n), fill=random_bases(rng, n))
        al(b, 0, 20, split_at(60, 30, "I", n), fill=random_bases(rng, n), rc=1)
    for n in (65536, 65537):
        al(b, 1, 100, [(100, "M"), (n, "D"), (100, "M")])
    al(b, 0, 5, [(3, "I"), (40, "M")])                       # starts with I, with D: unanchored
    al(b, 0, 5, [(3, "D"), (40, "M")])
    al(b, 0, 5, [(0, "M"), (2, "D"), (0, "M"), (2, "I"), (40, "M")])   # a D in front (unanchored) and an I behind it (anchored: the D consumed reference)
    al(b, 0, 50, [(5, "M"), (2, "I"), (3, "D"), (5, "M")], fill=b"GT")   # I directly followed by D: one anchor
    al(b, 0, 50, [(5, "M"), (3, "D"), (2, "I"), (5, "M")], fill=b"GT", rc=1)
    return b.done()


def long_shift_case():
    """a deletion and an insertion at the right end of a homopolymer of 5 000, from records that begin shortly before it -- 4 999
    steps, far past the records' own first base -- next to 70 records without a shift in the same wave"""
    ref = LEFT + b"A" * 5000 + RIGHT
    b = Builder("long-shift", [ref])
    end = len(LEFT) + 5000
    for k in range(35):
        al(b, 0, 2, split_at(30, 10 + k % 5, "D", 1))
    al(b, 0, end - 12, [(11, "M"), (1, "D"), (15, "M")])
    al(b, 0, end - 12, [(12, "M"), (1, "I"), (15, "M")], fill=b"A", rc=1)
    for k in range(35):
        al(b, 0, 2, split_at(30, 10 + k % 5, "I", 1), fill=b"G")
    al(b, 0, 0, [(len(ref), "M")])                            # one read over all of it: depth 1 at the far anchor
    return b.done()


def strands_case():
    """the batch's first read is reverse-complemented; one deletion and one insertion from both strands"""
    rng = np.random.default_rng(11)
    ref = random_bases(rng, 40) + b"CACACA" + random_bases(rng, 40)
    b = Builder("strands", [ref])
    for rc in (1, 0, 1, 1, 0):
        al(b, 0, 10, split_at(70, 33 + rc, "D", 2), rc=rc)
        al(b, 0, 12, split_at(60, 30 + 2 * rc, "I", 4), rc=rc, fill=b"CACA")
    return b.done()


def depth_case():
    """around anchor 49: a deletion and an insertion at one anchor, two insertions of equal length and different bases, a shorter and
    a longer one; a row whose AO exceeds its DP (its reads begin behind the anchor normalisation gives it)"""
    rng = np.random.default_rng(13)
    ref = random_bases(rng, 49) + b"G" + b"CT" + random_bases(rng, 48) + b"G" + b"T" * 20 + b"C" + random_bases(rng, 30)
    b = Builder("depth", [ref])
    for k in range(3):
        al(b, 0, 40 + k, split_at(40, 10 - k, "D", 2), rc=k & 1)
    for k, s in enumerate((b"TA", b"AT", b"AT", b"A", b"ATA", b"AT")):
        al(b, 0, 30 + k, split_at(40, 20 - k, "I", len(s)), fill=s, rc=k & 1)
    for begin, n in ((49, 1), (50, 30), (20, 29), (0, 50), (49, 60)):      # depth seams at the anchor
        al(b, 0, begin, [(n, "M")], rc=begin & 1)
    t_end = 100 + 1 + 20
    for k in range(3):                                                       # begin inside the run of T: no M column at anchor 100
        al(b, 0, t_end - 8 - k, split_at(20, 6 + k, "D", 1))
    al(b, 0, 95, [(10, "M")])                                                # ... which this read and the 60-base one above cover
    return b.done()


def skipped_case():
    rng = np.random.default_rng(17)
    ents = [random_bases(rng, 100) for _ in range(2)]
    b = Builder("skipped", ents)
    al(b, 0, 10, split_at(50, 20, "D", 2))
    for r in V.invalid_kinds(b, 0):
        b.single(r)
    read = b.read(ents[1][0:40])
    b.single(b.rec(read, 1, 60, b.cigar([(10, "M"), (2, "D"), (5, "I"), (30, "M")])))     # holds nothing: M past the entry behind I and D
    dead = al(b, 1, 0, split_at(60, 30, "D", 3), single=False)
    b.group([(0, al(b, 0, 0, split_at(60, 30, "I", 2), fill=b"GG", single=False), None)], [(1, dead, None)])
    return b.done()


def random_case(name, seed, n_records, alphabet=b"AC", n_entries=4, max_len=120):
    """random alignments with I and D runs over entries of a small alphabet (every event lies in some repeat), with a few N and
    lower-case bytes in the entries and the insertions"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    entries = []
    for _ in range(n_entries):
        e = bytearray(rng.choice(letters, int(rng.integers(20, max_len + 1))).tobytes())
        for at in np.nonzero(rng.random(len(e)) < 0.02)[0]:
            e[int(at)] = b"Nac"[int(rng.integers(0, 3))]
        entries.append(bytes(e))
    b = Builder(name, entries)
    for _ in range(n_records):
        e = int(rng.integers(0, n_entries))
        n = len(entries[e])
        span = int(rng.integers(5, min(n, 60) + 1))
        begin = int(rng.integers(0, n - span + 1))
        ops, left = [], span
        if rng.random() < 0.05:
            ops.append((int(rng.integers(1, 3)), "I"))
        while left:
            m = int(min(left, rng.integers(1, 15)))
            ops.append((m, "M"))
            left -= m
            if left > 4 and rng.random() < 0.7:
                if rng.random() < 0.5:
                    ops.append((int(rng.integers(1, 5)), "I"))
                else:
                    d = int(rng.integers(1, 4))
                    ops.append((d, "D"))
                    left -= d
        fill = bytearray(rng.choice(letters, 8).tobytes())
        if rng.random() < 0.05:
            fill[int(rng.integers(0, 8))] = ord("N")
        al(b, e, begin, ops, rc=int(rng.random() < 0.5), fill=bytes(fill))
    return b.done()


def cases():
    out = [grid(n) for n in (1, 255, 256, 257)]
    out.append(repeat_case("homopolymer", b"A", 8, del_lens=(1,), ins_lens=(1,)))
    out.append(repeat_case("tandem-2", b"CA", 6, del_lens=(2,), ins_lens=(2,)))
    out.append(repeat_case("tandem-3", b"CAG", 6, del_lens=(3, 6), ins_lens=(3, 6)))
    out.append(repeat_case("entry-start", b"A", 8, del_lens=(1,), ins_lens=(1,), left=b""))
    out.append(repeat_case("entry-start-tandem", b"CA", 6, del_lens=(2,), ins_lens=(2,), left=b""))
    out.append(repeat_case("after-same-base", b"A", 8, del_lens=(1,), ins_lens=(1,), left=b"", before=[LEFT + b"AAAA"]))
    out.append(repeat_case("after-same-repeat", b"CA", 6, del_lens=(2,), ins_lens=(2,), left=b"", before=[LEFT + b"CACA", b""]))
    out += [alphabet_case(), limits_case(), long_shift_case(), strands_case(), depth_case(), skipped_case()]
    out.append(random_case("random-ac", 31, 300))
    out.append(random_case("random-acgt", 32, 300, alphabet=b"ACGT"))
    out.append(random_case("random-a", 33, 100, alphabet=b"AAAC", n_entries=2))
    return out
