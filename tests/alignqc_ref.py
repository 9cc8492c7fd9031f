"""The alignment QC report of include/kslam_alignqc.h, restated in plain Python / numpy from the header's text (every column of
every contributing record laid out flat, then counted with bincount), the writer of the file's bytes, and the builder of the cases
the host twin and the device are held to.  Shares no code with host/alignqc.cpp.

A case is a dict: name, batches.  A batch is a case of tests/variants_ref.py (gbases / goff, rbases / roff, pool, ov / rp / pr)
with rqual (the quality column laid out like rbases, or None for a batch without one) and paired.  The tables of a case are the
sums of its batches' tables; a table set is what kslam_amd.alignqc.unpack gives."""
import math

import numpy as np

import variants_ref as V
from coverage_ref import NO_OVERLAP, OVERLAP_DT, PAIRED_OVERLAP_DT, READ_PAIR_DT  # noqa: F401

QUAL_COLS, CYCLE_COLS, LEN_BINS, NM_BINS, IDENTITY_BINS, INSERT_BINS = 95, 4, 65, 65, 101, 1002
SCALARS = ("n_records", "n_reverse", "n_skipped", "n_without_quality", "m_columns", "compared", "mismatches", "ins_events", "ins_bases",
           "del_events", "del_bases", "unaligned_bases")
PAIR_SCALARS = ("n_read_pairs", "pairs_both", "pairs_r1_only", "pairs_r2_only", "insert_sum")
CYCLES = (4, 512)   # the numbers of per-cycle rows every case is counted with

_CODE = np.full(256, 4, dtype=np.int64)          # A 0, C 1, G 2, T 3, upper case only; anything else 4
_COMP = np.arange(256, dtype=np.uint8)           # the complement of upper-case ACGT; every other byte stays
for _k, (_a, _b) in enumerate(zip(b"ACGT", b"TGCA")):
    _CODE[_a] = _k
    _COMP[_a] = _b
_QCOL = np.full(256, 94, dtype=np.int64)          # a byte in 33..126 counts in b - 33, every other byte in column 94
_QCOL[33:127] = np.arange(94)


# ---------------------------------------------------------------- the definition

def _flat(runs):
    """runs [(start, length)] -> (the run's number, the offset inside the run) for every element, flat"""
    n = np.array([r[1] for r in runs], dtype=np.int64)
    which = np.repeat(np.arange(len(runs), dtype=np.int64), n)
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    return which, np.arange(int(n.sum()), dtype=np.int64) - np.repeat(first, n)


def _columns(b):
    """everything of a batch that does not depend on C; cached on the batch"""
    if "_aq" in b:
        return b["_aq"]
    ov, rp, pr, goff, roff, pool = b["ov"], b["rp"], b["pr"], b["goff"], b["roff"], b["pool"]
    n_entries, n_reads = len(goff) - 1, len(roff) - 1
    half = n_reads // 2
    out = {"pairs": np.zeros(5, dtype=np.int64), "insert": np.zeros(INSERT_BINS, dtype=np.int64)}
    named = set()
    for g in rp:
        if int(g["count"]) > 0:
            out["pairs"][0] += 1
        for p in pr[int(g["first"]):int(g["first"]) + int(g["count"])]:      # the records behind first + count are dead
            r1, r2 = int(p["r1"]), int(p["r2"])
            named.update(i for i in (r1, r2) if i != NO_OVERLAP)
            if r1 != NO_OVERLAP and r2 != NO_OVERLAP:
                out["pairs"][1] += 1
                out["pairs"][4] += int(p["insert_size"])
                out["insert"][min(int(p["insert_size"]), INSERT_BINS - 1)] += 1
            elif r1 != NO_OVERLAP:
                out["pairs"][2] += 1
            elif r2 != NO_OVERLAP:
                out["pairs"][3] += 1
    rec = []          # per non-skipped record: (stream, reverse, read length, M columns, inserted bases, deleted bases)
    m_runs, i_runs, d_runs = [], [], []   # (record number, first reference byte, read's first byte, first query position, length)
    n_records, n_skipped = [0, 0], [0, 0]
    for i in sorted(named):          # each contributes once, however many live pairs name it
        o = ov[i]
        read, entry, rb_, qb_, n_ops, off = int(o["read"]), int(o["entry"]), int(o["ref_begin"]), int(o["query_begin"]), int(o["cigar_len"]), int(o["cigar_off"])
        z = 1 if b["paired"] and read >= half else 0
        n_records[z] += 1
        fits = entry < n_entries and n_ops > 0 and rb_ >= 0
        if fits:
            ref_len, L = int(goff[entry + 1] - goff[entry]), int(roff[read + 1] - roff[read])
            ops = [(int(c) >> 4, int(c) & 15) for c in pool[off:off + n_ops]]
            rp_, qp = rb_, max(qb_, 0)
            for n, op in ops:      # the whole CIGAR first
                if op == 0:
                    fits = fits and rp_ + n <= ref_len and qp + n <= L
                    rp_, qp = rp_ + n, qp + n
                elif op == 1:
                    fits = fits and qp + n <= L
                    qp += n
                elif op == 2:
                    fits = fits and rp_ + n <= ref_len
                    rp_ += n
        if not fits:
            n_skipped[z] += 1
            continue
        k, rc = len(rec), int(o["revcomp"]) != 0
        rp_, qp, mcols, ins, dele = rb_, max(qb_, 0), 0, 0, 0
        for n, op in ops:
            if op == 0:
                if n:
                    m_runs.append((k, n, int(goff[entry]) + rp_, qp))
                rp_, qp, mcols = rp_ + n, qp + n, mcols + n
            elif op == 1:
                if n:
                    i_runs.append((k, n, 0, qp))
                qp, ins = qp + n, ins + n
            elif op == 2:
                if n:
                    d_runs.append((k, n, min(qp, L - 1)))
                rp_, dele = rp_ + n, dele + n
        rec.append((z, rc, L, mcols, ins, dele, int(roff[read])))
    R = np.array(rec, dtype=np.int64).reshape(-1, 7)
    out.update(n_records=n_records, n_skipped=n_skipped, rec=R)

    def cycles_of(runs):
        """-> (record, cycle, index of the read's byte in rbases) of every base of the runs"""
        if not runs:
            z = np.zeros(0, dtype=np.int64)
            return z, z, z, z
        a = np.array(runs, dtype=np.int64)
        which, j = _flat([(0, r[1]) for r in runs])
        k = a[which, 0]
        q = a[which, 3] + j
        cyc = np.where(R[k, 1] != 0, R[k, 2] - 1 - q, q)      # the index of the base in the read as sequenced
        return k, cyc, R[k, 6] + cyc, a[which, 2] + j

    k, cyc, at, g = cycles_of(m_runs)
    r = b["gbases"][g] if len(g) else np.zeros(0, dtype=np.uint8)
    q = b["rbases"][at] if len(at) else np.zeros(0, dtype=np.uint8)
    q = np.where(R[k, 1] != 0, _COMP[q], q) if len(k) else q
    rk, qk = _CODE[r], _CODE[q]
    cmp_ = (rk < 4) & (qk < 4)
    rev = R[k, 1] != 0 if len(k) else np.zeros(0, dtype=bool)
    out["m"] = {"rec": k[cmp_], "cyc": cyc[cmp_], "mis": (rk != qk)[cmp_],
                # in the orientation of the read as sequenced: both bases complemented for a reverse record
                "cell": np.where(rev, 4 * (3 - rk) + (3 - qk), 4 * rk + qk)[cmp_],
                "qcol": _QCOL[b["rqual"][at]][cmp_] if b["rqual"] is not None and len(at) else None}
    ki, cyci, _, _ = cycles_of(i_runs)
    out["i"] = {"rec": ki, "cyc": cyci, "runs": [(r_[0], r_[1]) for r_ in i_runs]}
    out["d"] = [(k_, n, (R[k_, 2] - 1 - qd if R[k_, 1] else qd) if R[k_, 2] > 0 else None) for k_, n, qd in d_runs]
    b["_aq"] = out
    return out


def empty(cycles, paired=False):
    s = lambda: dict({n: 0 for n in SCALARS}, subst=[0] * 16, ins_len=[0] * LEN_BINS, del_len=[0] * LEN_BINS, nm=[0] * NM_BINS,  # noqa: E731
                     identity=[0] * IDENTITY_BINS, cycle=[0] * ((cycles + 1) * CYCLE_COLS), cq_compared=[0] * ((cycles + 1) * QUAL_COLS),
                     cq_mismatch=[0] * ((cycles + 1) * QUAL_COLS))
    return dict({"max_cycles": cycles, "paired": bool(paired), "insert": [0] * INSERT_BINS, "streams": [s(), s()]}, **{n: 0 for n in PAIR_SCALARS})


def batch_tables(b, cycles):
    """one batch -> its tables"""
    C = cycles
    f = _columns(b)
    t = empty(C, b["paired"])
    for k, name in enumerate(PAIR_SCALARS):
        t[name] = int(f["pairs"][k])
    t["insert"] = f["insert"].tolist()
    R, m, ins = f["rec"], f["m"], f["i"]
    n_rec = len(R)
    compared = np.bincount(m["rec"], minlength=n_rec)
    miss = np.bincount(m["rec"][m["mis"]], minlength=n_rec)
    for z in range(2):
        s = t["streams"][z]
        mine = R[:, 0] == z
        s["n_records"], s["n_skipped"] = f["n_records"][z], f["n_skipped"][z]
        s["n_without_quality"] = f["n_records"][z] if b["rqual"] is None else 0
        s["n_reverse"] = int((R[mine, 1] != 0).sum())
        s["m_columns"], s["ins_bases"], s["del_bases"] = int(R[mine, 3].sum()), int(R[mine, 4].sum()), int(R[mine, 5].sum())
        s["compared"], s["mismatches"] = int(compared[mine].sum()), int(miss[mine].sum())
        s["unaligned_bases"] = int((R[mine, 2] - R[mine, 3] - R[mine, 4]).sum())
        edits = (miss + R[:, 4] + R[:, 5])[mine]
        s["nm"] = np.bincount(np.minimum(edits, NM_BINS - 1), minlength=NM_BINS).tolist()
        den = (compared + R[:, 4] + R[:, 5])[mine]
        good = (compared - miss)[mine]
        s["identity"] = np.bincount((100 * good[den > 0]) // den[den > 0], minlength=IDENTITY_BINS).tolist()
        mz = R[m["rec"], 0] == z if len(m["rec"]) else np.zeros(0, dtype=bool)
        row = np.minimum(m["cyc"], C)
        cyc_t = np.zeros((C + 1, CYCLE_COLS), dtype=np.int64)
        cyc_t[:, 0] = np.bincount(row[mz], minlength=C + 1)
        cyc_t[:, 1] = np.bincount(row[mz & m["mis"]], minlength=C + 1)
        s["subst"] = np.bincount(m["cell"][mz], minlength=16).tolist()
        if m["qcol"] is not None:
            s["cq_compared"] = np.bincount((row * QUAL_COLS + m["qcol"])[mz], minlength=(C + 1) * QUAL_COLS).tolist()
            s["cq_mismatch"] = np.bincount((row * QUAL_COLS + m["qcol"])[mz & m["mis"]], minlength=(C + 1) * QUAL_COLS).tolist()
        iz = R[ins["rec"], 0] == z if len(ins["rec"]) else np.zeros(0, dtype=bool)
        cyc_t[:, 2] = np.bincount(np.minimum(ins["cyc"], C)[iz], minlength=C + 1)
        for k, n in ins["runs"]:
            if R[k, 0] == z:
                s["ins_events"] += 1
                s["ins_len"][min(n, LEN_BINS) - 1] += 1
        for k, n, cyc in f["d"]:
            if R[k, 0] == z:
                s["del_events"] += 1
                s["del_len"][min(n, LEN_BINS) - 1] += 1
                if cyc is not None:       # (a read of no bases has no cycle)
                    cyc_t[min(int(cyc), C), 3] += 1
        s["cycle"] = cyc_t.reshape(-1).tolist()
    return t


def add_tables(a, b):
    out = {"max_cycles": a["max_cycles"], "paired": a["paired"] or b["paired"]}
    for n in PAIR_SCALARS:
        out[n] = a[n] + b[n]
    out["insert"] = [x + y for x, y in zip(a["insert"], b["insert"])]
    out["streams"] = [{k: (v + t[k] if isinstance(v, int) else [x + y for x, y in zip(v, t[k])]) for k, v in s.items()}
                      for s, t in zip(a["streams"], b["streams"])]
    return out


_MEMO = {}


def tables(case, cycles):
    """a case -> its tables at `cycles` rows, computed once"""
    key = (case["name"], cycles)
    if key not in _MEMO:
        t = None
        for b in case["batches"]:
            p = batch_tables(b, cycles)
            t = p if t is None else add_tables(t, p)
        _MEMO[key] = t if t is not None else empty(cycles)
    return _MEMO[key]


# ---------------------------------------------------------------- the file

def _ratio(num, den):
    return '"%.6f"' % (num / den if den else 0.0)


def _scalars(w, indent="    "):
    names = [n[2:] if n.startswith("n_") else n for n in SCALARS]
    out = []
    for n, v in zip(names, w):
        out.append('%s"%s": %d' % (indent, n, v))
        if n == "mismatches":
            out.append('%s"error_rate": %s' % (indent, _ratio(w[6], w[5])))
    out.append('%s"mean_identity": %s' % (indent, _ratio(w[5] - w[6], w[5] + w[8] + w[10])))
    return out


def _sparse(v, pool=None, base=0):
    return "{" + ", ".join('"%s": %d' % (pool if pool and i == len(v) - 1 else str(i + base), x) for i, x in enumerate(v) if x) + "}"


def _cut(v):
    n = max([i + 1 for i, x in enumerate(v) if x], default=0)
    return list(v[:n])


def _stream_text(name, s, C):
    cyc = np.array(s["cycle"], dtype=np.int64).reshape(C + 1, CYCLE_COLS)
    lines = _scalars([s[n] for n in SCALARS])
    rows = len(_cut(cyc[:C, 0].tolist()))
    lines.append('    "mismatch_rate_by_cycle": [%s]' % ", ".join(_ratio(int(cyc[r, 1]), int(cyc[r, 0])) for r in range(rows)))
    lines.append('    "mismatch_rate_tail": %s' % _ratio(int(cyc[C, 1]), int(cyc[C, 0])))
    for k, key in enumerate(("compared_by_cycle", "mismatches_by_cycle", "inserted_bases_by_cycle", "deletions_by_cycle")):
        lines.append('    "%s": [%s]' % (key, ", ".join(str(x) for x in _cut(cyc[:C, k].tolist()))))
    lines.append('    "tail": [%s]' % ", ".join(str(int(x)) for x in cyc[C]))
    sub = ['"%s>%s": %d' % ("ACGT"[r], "ACGT"[q], s["subst"][4 * r + q]) for r in range(4) for q in range(4) if r != q]
    lines.append('    "substitutions": {%s, "matches": %d}' % (", ".join(sub), sum(s["subst"][5 * k] for k in range(4))))
    n = np.array(s["cq_compared"], dtype=np.int64).reshape(C + 1, QUAL_COLS).sum(axis=0)
    m = np.array(s["cq_mismatch"], dtype=np.int64).reshape(C + 1, QUAL_COLS).sum(axis=0)
    byq = []
    for q in range(QUAL_COLS):
        if n[q]:
            emp = -10.0 * math.log10(int(m[q]) / int(n[q])) + 0.0 if m[q] else 0.0      # (+ 0.0: a rate of 1 gives -0.0)
            byq.append('"%s": [%d, %d, "%.6f"]' % (str(q) if q < 94 else "invalid", n[q], m[q], emp))
    lines.append('    "by_quality": {%s}' % ", ".join(byq))
    lines.append('    "insertion_lengths": %s' % _sparse(s["ins_len"], ">64", 1))
    lines.append('    "deletion_lengths": %s' % _sparse(s["del_len"], ">64", 1))
    lines.append('    "edit_distance_counts": %s' % _sparse(s["nm"], "64+"))
    lines.append('    "identity_counts": %s' % _sparse(s["identity"]))
    return '  "%s": {\n%s\n  }' % (name, ",\n".join(lines))


def text(t):
    """the file's bytes for a table set"""
    C = t["max_cycles"]
    total = [t["streams"][0][n] + t["streams"][1][n] for n in SCALARS]
    lines = _scalars(total)
    lines += ['    "read_pairs": %d' % t["n_read_pairs"], '    "pairs_both": %d' % t["pairs_both"], '    "pairs_r1_only": %d' % t["pairs_r1_only"],
              '    "pairs_r2_only": %d' % t["pairs_r2_only"], '    "insert_size_mean": %s' % _ratio(t["insert_sum"], t["pairs_both"])]
    median, seen = "0", 0
    if t["pairs_both"]:
        median = ">1000"
        for b in range(INSERT_BINS - 1):
            seen += t["insert"][b]
            if 2 * seen >= t["pairs_both"]:
                median = str(b)
                break
    lines.append('    "insert_size_median": "%s"' % median)
    parts = ['  "kslam_align_qc": 1', '  "paired": %s' % ("true" if t["paired"] else "false"), '  "max_cycles": %d' % C,
             '  "summary": {\n%s\n  }' % ",\n".join(lines), _stream_text("read1", t["streams"][0], C)]
    if t["paired"]:
        parts.append(_stream_text("read2", t["streams"][1], C))
    parts.append('  "insert_size_counts": %s' % _sparse(t["insert"], ">1000"))
    return ("{\n" + ",\n".join(parts) + "\n}\n").encode()


# ---------------------------------------------------------------- the cases

class Builder(V.Builder):
    """tests/variants_ref.py's builder with a quality byte per base (default 'I') and an insert size per alignment pair"""

    def __init__(self, name, entries):
        super().__init__(name, entries)
        self.quals = {}

    def quality(self, read, q):
        assert len(q) == len(self.reads[read])
        self.quals[read] = bytes(q)

    def pair(self, r1, r2, insert=0, entry=None):
        """an alignment-pair record for group(); r1 / r2: an overlap record's index or None"""
        return (self.ov[r1 if r1 is not None else r2][1] if entry is None else entry, r1, r2, insert)

    def single(self, r):
        self.group([self.pair(r, None)])

    def done(self, paired=False, quality=True):
        if paired and len(self.reads) & 1:
            self.read(b"")          # [R1 | R2]: an even number of reads
        groups = self.groups
        self.groups = [([p[:3] for p in live], [p[:3] for p in dead]) for live, dead in groups]
        base = super().done(single_end=not paired)
        self.groups = groups
        ins = [p[3] if len(p) > 3 else 0 for live, dead in self.groups for p in live + dead]
        base["pr"]["insert_size"] = np.asarray(ins, dtype=np.uint32) if ins else 0
        q = b"".join(self.quals.get(i, b"I" * len(r)) for i, r in enumerate(self.reads))
        base["rqual"] = np.frombuffer(q, dtype=np.uint8) if quality else None
        base["paired"] = bool(paired)
        return base


def case_of(name, *batches):
    return {"name": name, "batches": list(batches)}


def _columns_case(name, n, rng):
    """an M run of n columns on both strands with mismatches on its first, its last and its 64-column boundaries"""
    b = Builder(name, [V.random_bases(rng, n + 40)])
    at = sorted({0, n - 1} | {x for x in (63, 64, 65, 127, 128) if x < n})
    b.single(b.aligned(0, 20, [(n, "M")], 0, mismatch_at=at))
    b.single(b.aligned(0, 7, [(n, "M")], 1, mismatch_at=at))
    return case_of(name, b.done())


def random_batch(name, seed, n_pairs, n_entries=40, paired=True):
    """tests/variants_ref.py's random batch with random quality bytes, insert sizes around the pool's edge and both streams"""
    rng = np.random.default_rng(seed)
    v = V.random_case(name, seed, n_pairs, n_entries)
    if paired and (len(v["roff"]) - 1) & 1:
        v["roff"] = np.concatenate([v["roff"], v["roff"][-1:]])
    v["rqual"] = rng.choice(np.array([35, 44, 55, 58, 70, 73, 126, 10], dtype=np.uint8), len(v["rbases"]), p=[.05, .1, .1, .1, .3, .3, .03, .02])
    v["pr"]["insert_size"] = rng.integers(0, 1100, len(v["pr"]))
    v["paired"] = paired
    return v


def cases():
    rng = np.random.default_rng(20261)
    out = []
    for n in (1, 63, 64, 65, 128, 129):
        out.append(_columns_case("m-%d" % n, n, rng))
    # a read longer than a tile of cycle rows, both strands: at C = 4 row C takes 296 of its 300 columns
    b = Builder("long-300", [V.random_bases(rng, 700)])
    for rc in (0, 1):
        r = b.aligned(0, 100 + 50 * rc, [(130, "M"), (3, "I"), (100, "M"), (4, "D"), (67, "M")], rc, mismatch_at=range(0, 300, 7))
        b.quality(b.ov[r][0], bytes(33 + (x * 7) % 94 for x in range(300)))
        b.single(r)
    out.append(case_of("long-300", b.done()))
    # one read text on both strands: the entry holds the read and, further on, its reverse complement
    read = V.random_bases(rng, 70)
    ent = bytearray(V.random_bases(rng, 20) + read + V.random_bases(rng, 20) + V.reverse_complement(read) + V.random_bases(rng, 20))
    for at in (22, 50, 112, 170):
        ent[at] = V.other_base(ent[at])
    b = Builder("both-strands", [bytes(ent)])
    r = b.read(read)
    b.quality(r, bytes(40 + x for x in range(70)))
    cig = b.cigar([(70, "M")])
    b.group([b.pair(b.rec(r, 0, 20, cig, 0), b.rec(r, 0, 110, cig, 1), insert=160)])
    out.append(case_of("both-strands", b.done()))
    # an I run and a D run at the first, the last and a 64-column boundary of the read; a D run as the final operation
    shapes = {"i-first": [(2, "I"), (98, "M")], "i-last": [(98, "M"), (2, "I")], "i-at-64": [(64, "M"), (2, "I"), (34, "M")],
              "i-over-64": [(63, "M"), (2, "I"), (35, "M")], "d-first": [(2, "D"), (100, "M")], "d-last": [(100, "M"), (2, "D")],
              "d-at-64": [(64, "M"), (2, "D"), (36, "M")], "d-at-63": [(63, "M"), (1, "D"), (37, "M")]}
    ent = V.random_bases(rng, 200)
    for name, ops in shapes.items():
        b = Builder(name, [ent])
        for rc in (0, 1):
            b.single(b.aligned(0, 30 + rc, ops, rc, mismatch_at=(5, 70)))
        out.append(case_of(name, b.done()))
    for n in (1, 64, 65, 66):
        b = Builder("indel-len-%d" % n, [V.random_bases(rng, 200)])
        b.single(b.aligned(0, 10, [(10, "M"), (n, "I"), (10, "M")], 0))
        b.single(b.aligned(0, 10, [(10, "M"), (n, "D"), (10, "M")], 1))
        out.append(case_of("indel-len-%d" % n, b.done()))
    b = Builder("nm-identity", [V.random_bases(rng, 200)])
    for n in (63, 64, 65):
        b.single(b.aligned(0, n, [(100, "M")], n & 1, mismatch_at=range(n)))
    b.single(b.aligned(0, 0, [(100, "M")], 0))                                   # identity exactly 100
    b.single(b.aligned(0, 50, [(30, "M")], 1, mismatch_at=range(30)))            # ... and 0
    b.single(b.aligned(0, 50, [(3, "M"), (97, "I")], 0, mismatch_at=(0, 1, 2)))  # 0 with insertions in the denominator
    out.append(case_of("nm-identity", b.done()))
    # lower case and N on either side: M columns that are not compared
    e = bytearray(V.random_bases(rng, 100))
    e[10:14] = b"NaNg"
    for rc in (0, 1):
        b = Builder("alphabet-%s" % ("rev" if rc else "fwd"), [bytes(e)])
        q = bytearray(b.query(0, 5, [(60, "M")]))
        q[5:9] = b"CCNg"
        q[15], q[16] = ord("n"), ord("a")
        q[30] = V.other_base(q[30])
        b.single(b.rec(b.read(V.reverse_complement(q) if rc else bytes(q)), 0, 5, b.cigar([(60, "M")]), rc))
        out.append(case_of(b.name, b.done()))
    # the quality column's edges, on matches and on mismatches, both strands
    b = Builder("quality-bytes", [V.random_bases(rng, 80)])
    edge = bytes([33, 126, 32, 127, 0, 255])
    for rc in (0, 1):
        r = b.aligned(0, 10 + rc, [(12, "M")], rc, mismatch_at=(1, 3, 5, 6, 8, 10))
        b.quality(b.ov[r][0], edge + edge[::-1])
        b.single(r)
    out.append(case_of("quality-bytes", b.done()))
    # a batch without a quality column next to one with
    parts = []
    for with_q in (True, False, True):
        b = Builder("q", [ent])
        b.group([b.pair(b.aligned(0, 10, [(50, "M")], 0, mismatch_at=(3, 9)), b.aligned(0, 90, [(50, "M")], 1, mismatch_at=(0,)), insert=130)])
        parts.append(b.done(paired=True, quality=with_q))
    out.append(case_of("without-quality", *parts))
    # each skip reason alone, next to one valid record
    for k, why in enumerate(("no-cigar", "entry-outside", "negative-begin", "m-past-entry", "m-past-read", "i-past-read", "d-past-entry")):
        b = Builder("skip-" + why, [ent, V.random_bases(rng, 60)])
        b.single(b.aligned(0, 0, [(40, "M")], 0, mismatch_at=(39,)))
        b.single(V.invalid_kinds(b, 1)[k])
        out.append(case_of(b.name, b.done()))
    # one byte past the read and one past the entry, on the LAST read and the LAST entry of their arrays
    for rc in (0, 1):
        b = Builder("past-the-end-%s" % ("rev" if rc else "fwd"), [ent, V.random_bases(rng, 64)])
        b.single(b.aligned(0, 0, [(20, "M")], rc))
        last = b.read(V.reverse_complement(b.entries[1][4:64]) if rc else b.entries[1][4:64])
        b.single(b.rec(last, 1, 4, b.cigar([(61, "M")]), rc))      # past both by one
        b.single(b.rec(last, 1, 5, b.cigar([(60, "M")]), rc))      # past the entry alone
        b.single(b.rec(last, 1, 3, b.cigar([(60, "M"), (1, "I")]), rc))   # past the read alone
        b.single(b.rec(last, 1, 4, b.cigar([(60, "M")]), rc))      # exactly to the end of both: valid
        out.append(case_of(b.name, b.done()))
    # the contributing set and the pairs
    ents = [V.random_bases(rng, 100) for _ in range(4)]
    b = Builder("contributing", ents)
    dead = b.aligned(3, 0, [(50, "M")], 0, mismatch_at=(3, 4))
    a0 = b.aligned(0, 0, [(10, "M")], 0, mismatch_at=(2,))
    b.group([b.pair(a0, None)], [b.pair(dead, None, 7), b.pair(None, dead)])
    b.group([], [b.pair(dead, dead, 500)])                                   # count == 0
    thrice = b.aligned(1, 5, [(30, "M")], 1, mismatch_at=(0, 29))
    mate = b.aligned(1, 20, [(30, "M")], 0, mismatch_at=(14,))
    b.group([b.pair(thrice, None), b.pair(None, thrice), b.pair(thrice, mate, 45)], [b.pair(thrice, None)])   # three live pairs and a dead one: once
    b.group([b.pair(None, None, 9, entry=2)])                                # a live pair with neither mate
    out.append(case_of("contributing", b.done(paired=True)))
    b = Builder("insert-sizes", ents)
    r1, r2 = b.aligned(0, 0, [(30, "M")], 0), b.aligned(0, 60, [(30, "M")], 1, mismatch_at=(1,))
    for isz in (0, 1000, 1001, 1002, 2 ** 32 - 1, 300, 300):
        b.group([b.pair(r1, r2, isz)])
    b.group([b.pair(r1, None, 5), b.pair(None, r2, 6), b.pair(None, r2, 7)])
    out.append(case_of("insert-sizes", b.done(paired=True)))
    b = Builder("single-end", ents)
    b.single(b.aligned(0, 10, [(50, "M")], 0, mismatch_at=(0, 49)))
    b.group([b.pair(b.aligned(1, 0, [(100, "M")], 1, mismatch_at=(0, 50, 99)), None), b.pair(b.aligned(0, 50, [(20, "M")], 1, mismatch_at=(5,)), None)])
    out.append(case_of("single-end", b.done()))
    out.append(case_of("no-reads", Builder("no-reads", ents).done(paired=True)))
    b = Builder("empty-read", ents)                                            # a read of no bases under a deletion: no cycle
    b.single(b.rec(b.read(b""), 0, 3, b.cigar([(2, "D")])))
    out.append(case_of("empty-read", b.done()))
    out.append(case_of("random-20000", random_batch("random-20000", 515, 60000)))
    return out


PLANTED_R1_CYCLE, PLANTED_R2_CYCLE, PLANTED_INDEL_CYCLE, PLANTED_QUALITY, PLANTED_FRAGMENT = 30, 75, 20, ord("("), 320


def planted(seed=2027, n_pairs=240, read_len=100):
    """Read pairs cut from one entry, error-free but for what is planted: every R1 has a substitution at cycle 30 and every R2
    one at cycle 75, each with quality byte '(' (7) under it and 'I' (40) everywhere else; every fourth R2 has 3 inserted bases
    at cycle 20, every fourth (another) lacks 2 bases of the entry there.  Fragments of 320 bases; every other pair comes from
    the reverse strand.  Two decoy entries.
    -> (entries, R1 text, R2 text, want) with want = {"read1" / "read2": {"subst": the 16 cells of the planted substitutions as
    sequenced (reference base as sequenced -> planted base), "n": reads}, "ins": reads with the insertion, "del": with the deletion}"""
    rng = np.random.default_rng(seed)
    entry = V.random_bases(rng, 12000)
    entries = [entry, V.random_bases(rng, 4000), V.random_bases(rng, 4000)]
    F, L = PLANTED_FRAGMENT, read_len
    want = {"read1": {"subst": [0] * 16, "n": n_pairs}, "read2": {"subst": [0] * 16, "n": n_pairs}, "ins": 0, "del": 0}
    texts = [[], []]
    for i in range(n_pairs):
        at = int(rng.integers(0, len(entry) - F + 1))
        frag = entry[at:at + F]
        if i & 1:
            frag = V.reverse_complement(frag)
        mates = [bytearray(frag[:L]), None]
        tail = V.reverse_complement(frag)            # R2 reads the fragment's other end, from its other strand
        if i % 4 == 1:                               # 3 inserted bases at cycle 20: the read covers 3 fewer bases of the entry
            ins = bytes(V.other_base(tail[PLANTED_INDEL_CYCLE], 2) for _ in range(3))
            mates[1] = bytearray(tail[:PLANTED_INDEL_CYCLE] + ins + tail[PLANTED_INDEL_CYCLE:L - 3])
            want["ins"] += 1
        elif i % 4 == 3:                             # 2 bases of the entry are missing at cycle 20
            mates[1] = bytearray(tail[:PLANTED_INDEL_CYCLE] + tail[PLANTED_INDEL_CYCLE + 2:L + 2])
            want["del"] += 1
        else:
            mates[1] = bytearray(tail[:L])
        for z, cyc in ((0, PLANTED_R1_CYCLE), (1, PLANTED_R2_CYCLE)):
            was = mates[z][cyc]
            now = V.other_base(was, 1 + i % 3)
            mates[z][cyc] = now
            want["read%d" % (z + 1)]["subst"][4 * V.ACGT.index(was) + V.ACGT.index(now)] += 1
            q = bytearray(b"I" * L)
            q[cyc] = PLANTED_QUALITY
            texts[z].append(b"@p%d/%d\n%s\n+\n%s\n" % (i, z + 1, bytes(mates[z]), bytes(q)))
    return entries, b"".join(texts[0]), b"".join(texts[1]), want


def check_planted(doc, want, n_pairs):
    """the report of the planted reads (tests/alignqc_ref.py: planted) holds what was planted and nothing else, for at least 95 %
    of the read pairs (the others the aligner did not place)"""
    least = lambda n: -(-95 * n // 100)   # noqa: E731
    assert doc["paired"] is True and least(n_pairs) <= doc["summary"]["pairs_both"] <= n_pairs and doc["summary"]["skipped"] == 0
    for name, cycle in (("read1", PLANTED_R1_CYCLE), ("read2", PLANTED_R2_CYCLE)):
        s, w = doc[name], want[name]
        miss = s["mismatches_by_cycle"]
        assert len(miss) == cycle + 1 and not any(miss[:cycle]) and least(w["n"]) <= miss[cycle] <= w["n"]       # the planted cycle alone
        assert set(s["by_quality"]) == {PLANTED_QUALITY - 33, 40}
        low, high = s["by_quality"][PLANTED_QUALITY - 33], s["by_quality"][40]
        assert low[0] == low[1] == miss[cycle] and high[1] == 0 and high[0] == s["compared"] - low[0]          # the planted quality row alone
        cells = {"%s>%s" % (r, q): w["subst"][4 * i + j] for i, r in enumerate("ACGT") for j, q in enumerate("ACGT") if i != j}
        got = {k: v for k, v in s["substitutions"].items() if k != "matches"}
        assert all(got[k] <= cells[k] for k in cells) and sum(got.values()) == miss[cycle]                      # the planted cells alone
    assert doc["read1"]["insertion_lengths"] == {} and doc["read1"]["deletion_lengths"] == {}
    ins, dele = doc["read2"]["insertion_lengths"], doc["read2"]["deletion_lengths"]
    assert set(ins) == {3} and least(want["ins"]) <= ins[3] <= want["ins"] and set(dele) == {2} and least(want["del"]) <= dele[2] <= want["del"]
    # the insert size is counted from the reads' lengths: the fragment's, 3 more under the insertion, 2 fewer under the deletion
    F, sizes = PLANTED_FRAGMENT, doc["insert_size_counts"]
    assert set(sizes) == {F - 2, F, F + 3} and sizes[F + 3] == ins[3] and sizes[F - 2] == dele[2] and sum(sizes.values()) == doc["summary"]["pairs_both"]


def header_example():
    """the worked example of include/kslam_alignqc.h as a case"""
    b = Builder("header", [b"ACGTACGTAC"])
    r0, r1 = b.read(b"ACGATC"), b.read(b"GTGC")
    b.quality(r0, b"IIII#I")
    b.quality(r1, b"5555")
    b.group([b.pair(b.rec(r0, 0, 0, b.cigar([(3, "M"), (1, "I"), (2, "M")]), 0), b.rec(r1, 0, 4, b.cigar([(2, "M"), (1, "D"), (2, "M")]), 1), insert=9)])
    return case_of("header", b.done())
