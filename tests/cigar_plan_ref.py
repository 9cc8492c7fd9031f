"""A plain numpy / Python restatement of the host driver of the banded CIGAR stage, k-slam_amd/csrc/cigar.hip.

The DP itself is not restated here: the oracle's banded_sw export (oracle.banded_sw) says which band width reached the
score and what CIGAR the traceback left.  This module restates everything AROUND one attempt -- sw_epilogue's inline
<n>M rule, the initial band, the chain of doubled widths, the bin / class of every width, which of the three
implementations a tuning runs an attempt on, whether that implementation hands the candidate to the one-lane kernel,
the temp slot overflow that sends a candidate to the big rerun -- and from these the counts the library prints under
KSLAM_DEBUG=1, so that a test can name the candidate and the seam behind a wrong count.

Test infrastructure only (CPU, numpy); it works from the oracle's rows of a batch.
"""
import re

import numpy as np

import oracle as O
from sw_plan_ref import codes, window, short_cap   # noqa: F401  (short_cap: re-exported for the case builders)

CIG_CAP = 24                                  # common.h: cigar ops per small temp slot
CIG_BIN_MAX_BW = (1, 2, 4, 7, 15, 31, 63)     # cigar.hip: the widest band of bins 0..6


def cig_bin(bw):
    """cigar.hip cig_bin: 0: 1   1: 2   2: 3..4   3: 5..7   4: 8..15   5: 16..31   6: 32..63   7: >= 64"""
    return bw - 1 if bw <= 2 else 2 if bw <= 4 else 3 if bw <= 7 else 4 if bw <= 15 else 5 if bw <= 31 else \
        6 if bw <= 63 else 7


def band_class(bw):
    """cigar.hip band_class: floor(log2 bw), the classes of the generic loop"""
    return int(bw).bit_length() - 1


class Tuning:
    """What cigar_traceback reads from the tuning: KSLAM_CIGAR_SYS, KSLAM_CIGAR_REG and api_align.hip cigar_tuning
    (a chunk of long reads: no systolic and no register launch)."""

    def __init__(self, sys_mask=0xF8, reg=True, long_chunk=False, name=None):
        self.sys_mask, self.reg, self.long_chunk = (0, False, True) if long_chunk else (sys_mask, reg, False)
        self.name = name or "sys=%#x reg=%d long=%d" % (self.sys_mask, self.reg, self.long_chunk)

    @classmethod
    def of_env(cls, env, long_chunk=False):
        return cls(int(env.get("KSLAM_CIGAR_SYS", "0xF8"), 0), not env.get("KSLAM_CIGAR_REG", "1").startswith("0"),
                   long_chunk, name=" ".join("%s=%s" % kv for kv in sorted(env.items())) or "default")


# the four tunings every case runs under
TUNINGS = {
    "default": {},
    "lds_only": {"KSLAM_CIGAR_SYS": "0", "KSLAM_CIGAR_REG": "0"},
    "all_systolic": {"KSLAM_CIGAR_SYS": "255"},
    "registers": {"KSLAM_CIGAR_SYS": "0"},
}


# ---- one attempt: where it runs (cigar.hip launch_systolic / launch) --------------------------------------------------
def systolic_shape(slot_bw, sys_mask, bin_):
    """launch_systolic: (GL, DPL) of the kernel that takes a launch whose slots are sized for slot_bw, or None when the
    launch does not go to the systolic kernel (need > 256, or the bin's bit is clear)."""
    need = 2 * slot_bw + 1
    if need > 256 or not (sys_mask >> min(bin_, 7)) & 1:
        return None
    gl = 16 if need > 64 else 8
    dpl = (8 if need <= 128 else 16) if gl == 16 else (2 if need <= 16 else 4 if need <= 32 else 8)
    return gl, dpl


def reg_width(slot_bw, reg):
    """launch's reg_bw ladder: the template width of the band-in-registers kernel, 0: the rows-in-LDS kernel"""
    if not reg:
        return 0
    return 1 if slot_bw <= 1 else 2 if slot_bw <= 2 else 4 if slot_bw <= 4 else 8 if slot_bw <= 8 else \
        16 if slot_bw <= 16 else 0


def lm_of(lmax):
    """the LM template value of the systolic kernels for a chunk whose longest read has lmax bases"""
    return 160 if lmax <= 160 else 256 if lmax <= 256 else 512


class Attempt:
    """One banded_sw attempt of one candidate: width, where the driver lists it (bin 0..6 of the sweep, or a class of
    the generic loop), the kernel the tuning launches for that list, and whether that kernel hands the candidate to the
    one-lane kernel (impl then names the kernel that declined)."""
    __slots__ = ("bw", "bin", "cls", "slot_bw", "impl", "handed", "slack")

    def __repr__(self):
        return "bw %d (%s, slots for %d, refLen - (2 bw + 1) = %d): %s%s" % (
            self.bw, "bin %d" % self.bin if self.cls is None else "class %d" % self.cls, self.slot_bw, self.slack,
            self.impl, " -> handed to k_banded_lds<0>" if self.handed else "")


def attempt(bw, ref_len, read_len, tune, lmax, hand_le=True):
    """hand_le=False perturbs the hand-over rule to `refLen < 2 bw + 1` (for the tests of this module's own teeth)."""
    a = Attempt()
    a.bw, a.bin = bw, cig_bin(bw)
    a.cls = band_class(bw) if a.bin == 7 else None
    a.slot_bw = CIG_BIN_MAX_BW[a.bin] if a.bin < 7 else (2 << a.cls) - 1
    a.slack = ref_len - (2 * bw + 1)
    covered = ref_len <= 2 * bw + 1 if hand_le else ref_len < 2 * bw + 1
    shape = systolic_shape(a.slot_bw, tune.sys_mask, a.bin)
    if shape is not None:
        gl, dpl = shape
        lm = lm_of(lmax)
        a.impl = "k_cigar_systolic<%d, %d, %d>" % (lm, gl, dpl)
        a.handed = 2 * bw + 1 > gl * dpl or covered or read_len > lm or ref_len > lm or read_len < 1
        return a
    rw = reg_width(a.slot_bw, tune.reg)
    a.impl = "k_banded_lds<%d>" % rw
    a.handed = rw > 0 and not (bw <= rw and not covered)
    return a


# ---- candidates -------------------------------------------------------------------------------------------------------
class Cand:
    """What the CIGAR stage knows and does about one row."""
    __slots__ = ("row", "read", "rc", "ref_len", "read_len", "score", "want", "inline", "dsum", "bw0", "band", "ops",
                 "ends_on_indel", "status", "cigar", "q0", "r0", "shift_q", "shift_r")


def unflip(row, L, entry_len):
    """window-relative, un-flipped spans of a final row (the inverse of k_finalize / SmithWaterman.h:211-229):
    (ref_begin, ref_end, query_begin, query_end, wlen, s0)"""
    s0 = max(int(row["rel"]), 0)
    wlen = max(0, min(L, entry_len - s0))
    rb, re_ = int(row["ref_begin"]) - s0, int(row["ref_end"]) - s0
    qb, qe = int(row["query_begin"]), int(row["query_end"])
    if row["revcomp"]:
        rb, re_ = wlen - 1 - re_, wlen - 1 - rb
        qb, qe = L - 1 - qe, L - 1 - qb
    return rb, re_, qb, qe, wlen, s0


def candidates(rows, reads, entries, sc, read_off=None, entry_off=None):
    """Per row of the oracle's result: the spans, sw_epilogue's decision, and for the banded ones what the oracle's
    banded_sw does from bw0 on.  read_off / entry_off (byte offsets of every read / entry in the library's flat base
    arrays) add the 16-byte staging residues of both spans."""
    mat = O.build_matrix(sc[0], sc[1])
    rq = {}
    out = []
    for k in range(len(rows)):
        row = rows[k]
        r, e = int(row["read"]), int(row["entry"])
        L = len(reads[r])
        rb, re_, qb, qe, wlen, s0 = unflip(row, L, len(entries[e]))
        c = Cand()
        c.row, c.read, c.rc, c.score = k, r, bool(row["revcomp"]), int(row["score"])
        c.ref_len, c.read_len = re_ - rb + 1, qe - qb + 1
        c.want = c.score > 0                           # sw_epilogue: report_cigar, threshold 0
        c.inline, c.dsum, c.bw0, c.band, c.ops, c.ends_on_indel, c.status, c.cigar = False, None, 0, 0, 0, False, 0, None
        c.q0, c.r0 = qb, rb
        if read_off is not None:                       # k_banded_lds: qsrc and rsrc
            c.shift_q = (int(read_off[r]) + qb) & 15
            c.shift_r = (int(entry_off[e]) + s0 + (wlen - 1 - re_ if c.rc else rb)) & 15
        else:
            c.shift_q = c.shift_r = None
        if c.want:
            if r not in rq:
                rq[r] = codes(reads[r])
            q = rq[r][qb:qe + 1]
            w = window(L, entries[e], int(row["rel"]), c.rc)[rb:re_ + 1]
            if c.ref_len == c.read_len:
                c.dsum = int(np.where((q > 3) | (w > 3), 0, np.where(q == w, sc[0], -sc[1])).sum())
                c.inline = c.dsum == c.score
            if c.inline:
                c.ops, c.cigar = 1, np.array([c.read_len << 4], dtype=np.uint32)
            else:
                c.bw0 = abs(c.ref_len - c.read_len) + 1
                c.cigar, c.status, c.band = O.banded_sw(q, w, c.score, mat, sc[2], sc[3], c.bw0)
                c.ops = len(c.cigar)
                # the walk ended on an indel (ssw.c:757-761: `<cnt><op>` and a closing 1M, first in alignment order)
                c.ends_on_indel = c.ops >= 2 and int(c.cigar[0]) == 16 and (int(c.cigar[1]) & 15) != 0
        out.append(c)
    return out


def overflows(c, cap=CIG_CAP):
    """banded_traceback's *ovf for a temp slot of cap ops: every op but the last is written at its index l < cap; the
    final fix-up writes one op at l (l < cap) after a match, two at l and l + 1 (l + 1 < cap) after an indel."""
    if c.ends_on_indel:
        l = c.ops - 2
        return not l + 1 < cap
    l = c.ops - 1
    return not l < cap


def widths(c):
    """bw0 2^r up to the band that reached the score"""
    w, out = c.bw0, []
    while w <= c.band:
        out.append(w)
        w *= 2
    assert out and out[-1] == c.band, (c.bw0, c.band)
    return out


def sentinel_rows(c, bw):
    """rows i >= 1 where the sentinel write h_b[edge] = e_b[edge] = 0 of ssw.c:655 lands on a live cell of row i - 1:
    the band is clipped by the reference end (refLen - 1 < i + bw) while the row array is still anchored at column 0
    (i - 1 <= bw)."""
    return [i for i in range(1, c.read_len) if i - 1 <= bw and c.ref_len - 1 < i + bw]


# ---- the plan of a batch ----------------------------------------------------------------------------------------------
class Plan:
    """cand: every row; attempts[row]: the Attempt list of a banded row; and the counts of the debug lines:
    bins0 (8), handed (sum over the sweep's rounds), classes {c: n}, arrivals (7: what doubling sent to bins 0..6),
    big (n, band) or None."""

    def describe(self, c):
        s = "row %d read %d%s (refLen %d, readLen %d, bw0 %d, final band %d, ops %d%s)" % (
            c.row, c.read, " rc" if c.rc else "", c.ref_len, c.read_len, c.bw0, c.band, c.ops,
            ", ends on an indel" if c.ends_on_indel else "")
        if c.row in self.attempts:
            s += " attempts: " + "; ".join(map(repr, self.attempts[c.row]))
        return s


def plan(cand, tune, lmax, hand_le=True, cap=CIG_CAP):
    p = Plan()
    p.cand, p.attempts = cand, {}
    p.bins0 = [0] * 8
    p.handed, p.classes, p.arrivals = 0, {}, [0] * 7
    big = []
    for c in cand:
        if not c.want or c.inline:
            continue
        p.bins0[cig_bin(c.bw0)] += 1
        at = [attempt(w, c.ref_len, c.read_len, tune, lmax, hand_le) for w in widths(c)]
        p.attempts[c.row] = at
        for r, a in enumerate(at):
            if a.cls is None:
                p.handed += a.handed               # (the generic loop prints no hand-over count)
                p.arrivals[a.bin] += r > 0
            else:
                p.classes[a.cls] = p.classes.get(a.cls, 0) + 1
        if overflows(c, cap):
            big.append(c)
    p.big_rows = [c.row for c in big]
    p.big = (len(big), max(c.band for c in big)) if big else None
    return p


# ---- the debug lines --------------------------------------------------------------------------------------------------
def parse_debug(err):
    """The counts of one align call's KSLAM_DEBUG=1 lines, in the shape of Plan's."""
    bins = [list(map(int, m.split())) for m in re.findall(r"\[kslam\] cigar bins as the SW stage asked for them: ([\d ]+)\n", err)]
    handed = sum(int(x) for x in re.findall(r"\[kslam\]   handed to the one-lane kernel: (\d+)\n", err))
    classes = {}
    for c, n in re.findall(r"\[kslam\] cigar class (\d+) \(band <= \d+\): (\d+) candidates\n", err):
        classes[int(c)] = classes.get(int(c), 0) + int(n)
    arrivals = [0] * 7
    for b, w, n in re.findall(r"\[kslam\] cigar round \d+ bin (\d+) \(band <= (\d+)\): (\d+) candidates left over\n", err):
        assert CIG_BIN_MAX_BW[int(b)] == int(w)
        arrivals[int(b)] += int(n)
    big = [(int(n), int(b)) for n, b in re.findall(r"\[kslam\] cigar big rerun: (\d+) candidates at band (\d+)\n", err)]
    return dict(bins=bins, handed=handed, classes=classes, arrivals=arrivals, big=big)


def explain(p, got, room0):
    """The differences between a plan and the parsed counts of a run, each with the candidates behind the count;
    empty when they agree.  room0: the run had KSLAM_SWEEP_ROOM=0 (only then are the arrivals printed exactly)."""
    bad = []
    banded = [c for c in p.cand if c.row in p.attempts]

    def members(pred, limit=4, key=None):
        rows = [p.describe(c) for c in sorted((c for c in banded if pred(c)), key=key or (lambda c: c.row))]
        return "\n    " + "\n    ".join(rows[:limit]) + ("\n    ... %d in all" % len(rows) if len(rows) > limit else "")

    want_bins = [p.bins0]                      # (printed for every chunk that has a candidate)
    if got["bins"] != want_bins:
        bad.append("bins as asked for: printed %s, restated %s" % (got["bins"], want_bins))
    if got["handed"] != p.handed:
        bad.append("handed over: printed %d, restated %d; the restatement's:%s" % (
            got["handed"], p.handed, members(lambda c: any(a.handed and a.cls is None for a in p.attempts[c.row]), 8,
                                             lambda c: min(abs(a.slack) for a in p.attempts[c.row]))))   # nearest the rule's edge first
    if got["classes"] != p.classes:
        for k in sorted(set(got["classes"]) | set(p.classes)):
            if got["classes"].get(k, 0) != p.classes.get(k, 0):
                bad.append("class %d: printed %d, restated %d; the restatement's:%s" % (
                    k, got["classes"].get(k, 0), p.classes.get(k, 0),
                    members(lambda c: any(a.cls == k for a in p.attempts[c.row]))))
    if room0 and got["arrivals"] != p.arrivals:
        for b in range(7):
            if got["arrivals"][b] != p.arrivals[b]:
                bad.append("bin %d arrivals by doubling: printed %d, restated %d; the restatement's:%s" % (
                    b, got["arrivals"][b], p.arrivals[b],
                    members(lambda c: any(a.bin == b and r > 0 for r, a in enumerate(p.attempts[c.row])))))
    want_big = [p.big] if p.big else []
    if got["big"] != want_big:
        bad.append("big rerun: printed %s, restated %s; the restatement's:%s" % (
            got["big"], want_big, members(lambda c: c.row in p.big_rows, 8, lambda c: c.ops)))   # nearest the cap first
    return bad
