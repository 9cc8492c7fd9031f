"""FASTQ texts laid out against the tiling of csrc/fastq_index.hip, and the plain reader they are checked with (no library,
no numpy arrays of masks: bytes and loops).

  records()   the reference of tests/test_gpu_fastq_index.py: a byte loop that cuts lines at "\\n", "\\r\\n" and a lone "\\r",
              four lines per record, the rules of include/kslam_fastq.h.
  build()     one or two streams, built record by record in step (record k of R1 is the mate of record k of R2), in which
              chosen terminators of chosen lines start at chosen offsets.  The slack is taken up by the read lengths, by
              header text behind a space and by filler records (empty and short reads, odd headers); planted reads are exact
              copies of genome windows, proper pairs at one fragment length, and are never cut.
  census()    which cells of the seam matrix a text hits, found from the text alone.

The geometry (csrc/fastq_index.hip): a lane's piece is 16 bytes, 64 lanes make 1 024 bytes, four pieces per lane one 4 096-byte
tile (one wave), four tiles one 16 384-byte workgroup.  A seam belongs to the LARGEST of these that divides its offset: the
offset 8 192 is a 4 096 seam, not a 16 seam, because the code that handles it is the tile's, not the lane's."""
import numpy as np

SEAMS = (16384, 4096, 1024, 16)
KINDS = ("LF", "CRLF", "CR", "CRCRLF", "LFCR")
PLACEMENTS = ("last", "first")      # the terminator's first byte is the last byte before the seam / the first byte after it
ROLES = (0, 1, 2, 3)                # header, bases, '+', quality
MATRIX = [(k, s, p, r) for k in KINDS for s in SEAMS for p in PLACEMENTS for r in ROLES]
_FIRST = {"LF": b"\n", "CRLF": b"\r\n", "CR": b"\r", "CRCRLF": b"\r", "LFCR": b"\n"}
_SECOND = {"CRCRLF": b"\r\n", "LFCR": b"\r"}     # ends the EMPTY line that follows
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ---------------------------------------------------------------- the plain reader
def lines(text, at_eof=True):
    """-> ([(start, end, start of the next line)] of the terminated lines, start of the unterminated rest)"""
    out, start, p, n = [], 0, 0, len(text)
    while p < n:
        c = text[p]
        if c == 10:
            out.append((start, p, p + 1))
            p += 1
            start = p
        elif c == 13:
            if p + 1 < n:
                nx = p + 2 if text[p + 1] == 10 else p + 1
            elif at_eof:
                nx = p + 1
            else:
                break           # the last byte of a prefix: it may be half of "\r\n", so it ends no line yet
            out.append((start, p, nx))
            p = nx
            start = p
        else:
            p += 1
    return out, start


def identifier(header):
    if len(header) <= 1:
        return b""
    sp = header.find(b" ")
    end = len(header) if sp < 0 else (1 if sp == 0 else sp)
    body = header[1:end]
    sl = body.find(b"/")
    return body if sl < 0 else body[:sl]


def records(text, max_records=0, at_eof=True):
    """-> (identifiers, bases, qualities, consumed)"""
    ls, rest = lines(text, at_eof)
    if at_eof:
        if rest < len(text):
            ls.append((rest, len(text), len(text)))      # the unterminated rest
        ls.append((len(text), len(text), len(text)))      # and the empty line read at the end of the stream
    n = len(ls) // 4
    if max_records and n > max_records:
        n = max_records
    ids = [identifier(text[ls[4 * r][0]:ls[4 * r][1]]) for r in range(n)]
    bases = [text[ls[4 * r + 1][0]:ls[4 * r + 1][1]] for r in range(n)]
    quals = [text[ls[4 * r + 3][0]:ls[4 * r + 3][1]] for r in range(n)]
    if at_eof and (not max_records or n < max_records):
        consumed = len(text)
    else:
        consumed = ls[4 * n - 1][2] if n else 0
    return ids, bases, quals, consumed


# ---------------------------------------------------------------- the census
def seam_of(offset):
    for s in SEAMS:
        if offset and offset % s == 0:
            return s
    return None


def census(text, at_eof=True):
    """-> {(kind, seam, placement, role): times hit} over the terminated lines of the text's records"""
    ls, _ = lines(text, at_eof)
    n, hits = len(text), {}

    def at(p):
        return text[p] if p < n else -1
    for i, (_, p, _) in enumerate(ls):
        if text[p] == 10:
            if at(p + 1) == 13:
                kind = "LFCR" if at(p + 2) not in (10, 13, -1) else None
            else:
                kind = "LF" if p + 1 < n else None
        elif p and text[p - 1] == 13:
            kind = None         # the second half of "\r\r\n" / "\n\r": counted with its first half
        elif at(p + 1) == 10:
            kind = "CRLF"
        elif at(p + 1) == 13:
            kind = "CRCRLF" if at(p + 2) == 10 else None
        else:
            kind = "CR" if p + 1 < n else None
        if kind is None:
            continue
        for placement, s in (("last", p + 1), ("first", p)):
            seam = seam_of(s)
            if seam:
                cell = (kind, seam, placement, i % 4)
                hits[cell] = hits.get(cell, 0) + 1
    return hits


def missing_cells(text, at_eof=True):
    hits = census(text, at_eof)
    return [c for c in MATRIX if c not in hits]


def matrix_targets():
    """one target per cell: the 16 384 seams from 16 384 up, and in every 16 KiB block a 1 024 seam at +2 048, a 4 096 seam at
    +4 096 and a 16 seam at +6 160; the cells of a seam class dealt over the blocks"""
    cells = [(k, p, r) for k in KINDS for p in PLACEMENTS for r in ROLES]
    out = []
    for b, (kind, placement, role) in enumerate(cells):
        for seam in (16384 * (b + 1), 16384 * b + 2048, 16384 * b + 4096, 16384 * b + 6160):
            out.append(Target(seam - 1 if placement == "last" else seam, kind, role))
    return sorted(out, key=lambda t: t.T)


# ---------------------------------------------------------------- the builder
class Target:
    """the terminator of the line `role` of some record starts at offset T; L: that record's read length, if it matters"""

    def __init__(self, T, kind="LF", role=3, L=None):
        self.T, self.kind, self.role, self.L = T, kind, role, L


class Planter:
    """exact copies of genome windows: a fragment of `frag` bases, R1 from its start, R2 reverse-complemented from its end
    (or the other way round); single end: mate 0 only"""

    def __init__(self, genomes, frag, rng):
        self.g, self.frag, self.rng = genomes, frag, rng

    def fragment(self):
        gi = int(self.rng.integers(0, len(self.g)))
        start = int(self.rng.integers(0, len(self.g[gi]) - self.frag))
        return self.g[gi][start:start + self.frag], bool(self.rng.random() < 0.5)

    @staticmethod
    def read(fragment, mate, L):
        f, flip = fragment
        assert L <= len(f)
        return f[:L] if (mate == 0) != flip else f[len(f) - L:].translate(_COMP)[::-1]


PLANTED_HEADS = [b"@p%d", b"@p%d/1", b"@p%d extra", b"@p%d/2 x/y", b"@p%d x\tTAB"]
FILLER_HEADS = [b"@f%d", b"@f%d d t", b"@ f%d", b"@a/b/c%d", b"@/f%d", b"@f%d\tT/9", b"@", b"x", b""]
_PAD = b"pad/ text:" * 8


def _pad_header(base, h):
    need = h - len(base)
    assert need >= 0
    if need == 0:
        return base
    if b" " in base:
        return base + (_PAD * (need // len(_PAD) + 1))[:need]
    return base + b" " + (_PAD * (need // len(_PAD) + 1))[:need - 1]


class Stream:
    def __init__(self, rng, mate, targets, lens, fill_lens, max_pad, final_mod=None):
        self.rng, self.mate, self.targets, self.ti = rng, mate, targets, 0
        self.lens, self.fill_lens, self.max_pad, self.final_mod = lens, fill_lens, max_pad, final_mod
        self.near = 2 * max(max(lens), max([t.L or 0 for t in targets] + [0])) + max_pad + 32 + 450
        self.out, self.pos = [], 0
        self.pending = None            # the next record starts with an empty header ended by this terminator
        self.header_nonempty = False   # the next record's header must not be empty
        self.hits = []                 # (record, target) as laid out

    def target(self):
        return self.targets[self.ti] if self.ti < len(self.targets) else None

    def at_target(self):
        t = self.target()
        return t is not None and t.T - self.pos <= self.near

    def need(self):
        if self.pending is not None:
            return "filler"
        t = self.target()
        if self.at_target() and t.kind in _SECOND and t.role in (0, 2):
            return "filler"            # the empty line after the terminator is the bases or the quality line
        if self.at_target() and t.L:
            return "planted"           # a read of that length is wanted here
        return None

    def emit(self, k, rtype, fragment, final=False, L=None, pad=None):
        rng, t = self.rng, self.target()
        hit = self.at_target()
        pend, self.pending = self.pending, None
        assert not (hit and pend is not None)
        multi = hit and t.kind in _SECOND
        if rtype == "planted":
            assert pend is None and not (multi and t.role in (0, 2))
            if L is None:
                L = t.L if hit and t.L else int(rng.choice(self.lens))
            base = PLANTED_HEADS[int(rng.integers(0, len(PLANTED_HEADS)))] % k
        else:
            if multi and t.role in (0, 2):
                L = 0
            else:
                L = int(rng.choice(self.fill_lens))
                if (hit or pend is not None) and L == 0:
                    L = 1 + int(rng.integers(0, 31))
            base = FILLER_HEADS[int(rng.integers(0, len(FILLER_HEADS)))]
            base = base % k if b"%d" in base else base
        pick = [b"\n", b"\r\n", b"\r"]
        term = [pick[int(rng.integers(0, 3 if L else 2))], pick[int(rng.integers(0, 3))], pick[int(rng.integers(0, 3 if L else 2))],
                pick[int(rng.integers(0, 2))]]
        plus = b"+"
        extra = int(rng.integers(0, self.max_pad + 1)) if pad is None else pad
        if pend is not None:
            base, extra, term[0] = b"", 0, pend
        elif self.header_nonempty and not base:
            base = b"@"
        self.header_nonempty = False
        quality_empty = False
        if hit:
            r = t.role
            term[r] = _FIRST[t.kind]
            if multi:
                if r == 0:
                    term[1] = _SECOND[t.kind]
                elif r == 1:
                    plus, term[2] = b"", _SECOND[t.kind]
                elif r == 2:
                    term[3] = _SECOND[t.kind]
                    quality_empty = True
                else:
                    self.pending = _SECOND[t.kind]
            if (r == 3 and not multi) or (r == 2 and t.kind == "LFCR"):
                self.header_nonempty = True
            g = t.T - self.pos
            fixed = sum(len(term[i]) for i in range(r)) + (len(plus) if r >= 2 else 0)
            n_l = (1 if r >= 1 else 0) + (1 if r >= 3 else 0)
            if rtype == "planted" and n_l:
                L = max(min(self.lens), min(max(self.lens), (g - fixed - len(base) - extra) // n_l))
            h = g - fixed - n_l * L
            if rtype != "planted" and h < len(base):
                base = b"@"
            assert h >= max(len(base), 1), (h, base, g)
        else:
            h = len(base) + extra
        if rtype == "planted":
            seq = Planter.read(fragment, self.mate, L)
        else:
            seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), L))
        qual = bytes(rng.integers(33, 75, L, dtype=np.uint8))
        if rtype != "planted" and L == 2 and rng.random() < 0.5:
            qual = b"//"
        assert not quality_empty or L == 0
        if final and self.final_mod is not None:
            size = h + len(seq) + len(plus) + len(qual) + sum(len(x) for x in term)
            h += (self.final_mod - (self.pos + size)) % 16
        rec = _pad_header(base, h) + term[0] + seq + term[1] + plus + term[2] + qual + term[3]
        if hit:
            self.hits.append((k, t))
            self.ti += 1
        else:
            assert t is None or self.pos + len(rec) + 100 < t.T, "an ordinary record ran into the next target"
        self.out.append(rec)
        self.pos += len(rec)


def build(seed, genomes, frag, targets, lens=(50, 64, 100, 150, 255, 256, 257, 271, 272, 273, 300), fill_lens=(0, 0, 1, 2, 15, 16, 17, 31),
          planted_frac=0.75, max_pad=40, final_mod=(None, None), min_records=0, plan=None, twins=False, end_at_targets=False):
    """targets: one list per stream (so: one list = single end).  plan: [(type, L of R1, L of R2[, header pad])] for the first
    records.
    twins: both streams draw the same layout (lengths, pads, terminators), so their targets fall on the same records.
    -> (texts, planted record numbers, the Stream objects)"""
    rng = np.random.default_rng(seed)
    planter = Planter(genomes, frag, np.random.default_rng(seed + 1))
    plan = list(plan or [])
    lens = tuple(lens) + tuple(x for p in plan for x in p[1:3] if x and p[0] == "planted")
    max_pad = max([max_pad] + [p[3] for p in plan if len(p) > 3])
    streams = [Stream(np.random.default_rng(seed + 2 + (0 if twins else m)), m, list(ts), lens, fill_lens, max_pad, final_mod[m])
               for m, ts in enumerate(targets)]
    planted, k, at = [], 0, 0
    while True:
        busy = any(s.target() is not None or s.pending is not None for s in streams) or k + 1 < min_records or at < len(plan)
        needs = [s.need() for s in streams]
        final = not busy or (end_at_targets and all(s.ti + 1 >= len(s.targets) and s.at_target() for s in streams))
        spec = None
        assert not ("filler" in needs and "planted" in needs)
        if "filler" in needs:
            rtype = "filler"
        elif "planted" in needs:
            rtype = "planted"
        elif at < len(plan):
            spec, at = plan[at], at + 1
            rtype = spec[0]
        else:
            rtype = "planted" if rng.random() < planted_frac else "filler"
        fragment = planter.fragment() if rtype == "planted" else None
        for m, s in enumerate(streams):
            s.emit(k, rtype, fragment, final=final, L=spec[1 + m] if spec and rtype == "planted" else None,
                   pad=spec[3] if spec and len(spec) > 3 else None)
        if rtype == "planted":
            planted.append(k)
        k += 1
        if final:
            break
    return [b"".join(s.out) for s in streams], planted, streams


# ---------------------------------------------------------------- the cases of tests/test_gpu_fastq_index.py
GENOMES = {"small": (501, 2, 60000), "big": (502, 4, 500000)}   # seed, genomes, bases each: i.i.d., so a window of 50 occurs once


def genomes(synth, which):
    seed, n, length = GENOMES[which]
    return synth.to_bytes(synth.make_genomes(seed, n, 1, length))


def _case(name, texts, planted=(), at_eof=True, max_pairs=0, genome="small", matrix=False, error=None):
    return {"name": name, "r1": texts[0], "r2": texts[1] if len(texts) > 1 else None, "planted": list(planted), "at_eof": at_eof,
            "max_pairs": max_pairs, "genome": genome, "matrix": matrix, "error": error}


R2_STARTS = (0, 1, 7, 8, 15)     # len1 mod 16: where R2's first tile starts inside the device text


def matrix_cases(g):
    for i, mod in enumerate(R2_STARTS):
        texts, planted, _ = build(100 + 10 * i, g, 500, [matrix_targets(), matrix_targets()], final_mod=(mod, None))
        assert len(texts[0]) % 16 == mod
        yield _case("matrix_r2_at_%d_mod_16" % mod, texts, planted, matrix=True)
    texts, planted, _ = build(160, g, 500, [matrix_targets()])
    yield _case("matrix_single_end", texts, planted, matrix=True)


def long_line_cases(g):
    """reads of 600 - 4 097 bases at one fragment length; a header of 9 000 bytes (three tiles without a terminator); a
    4 097-base line that starts on the last byte of a tile, fills the next and is ended on the first byte of the third; the
    gather's 16- and 256-byte steps (k_gather_fields: 16 lanes x 16 bytes) among the planted and the filler lengths"""
    plan = [("planted", 600, 4000), ("planted", 4095, 4096), ("planted", 255, 256, 9000), ("planted", 4096, 4097), ("planted", 257, 271),
            ("planted", 4097, 4095), ("planted", 272, 273), ("planted", 3000, 1000), ("planted", 273, 255), ("planted", 256, 257),
            ("planted", 271, 272), ("planted", 2048, 4064), ("planted", 4080, 2047)]
    t1 = [Target(4096 * 14 - 2, "LF", 0, L=4097)]
    t2 = [Target(4096 * 17 - 3, "CRLF", 0, L=4097)]
    texts, planted, streams = build(200, g, 4300, [t1, t2], lens=(600, 1500, 4000), plan=plan, min_records=40)
    yield _case("long_lines", texts, planted)
    texts, planted, _ = build(201, g, 4300, [t1], lens=(600, 1500, 4000), plan=plan, min_records=40)
    yield _case("long_lines_single_end", texts, planted)


def end_cases(g):
    def twins(seed, T, kind, role=3, more=0):
        return build(seed, g, 500, [[Target(T, kind, role)]] * 2, twins=True, end_at_targets=not more, min_records=more)
    for name, T in (("ends_at_a_tile_seam", 8191), ("ends_a_byte_before_a_tile_seam", 8190), ("ends_a_byte_after_a_tile_seam", 8192)):
        texts, planted, _ = twins(300 + T, T, "LF")
        assert len(texts[0]) == T + 1 == len(texts[1])
        for at_eof in (True, False):
            yield _case("%s_eof_%d" % (name, at_eof), texts, planted, at_eof=at_eof)
    # the last byte is "\r" and len - 1 is two tiles: as a prefix the scan stops a whole tile short, the record stays open
    texts, planted, _ = twins(310, 8192, "CR")
    assert len(texts[0]) == 8193 and texts[0][-1:] == b"\r" and texts[1][-1:] == b"\r"
    yield _case("prefix_ends_in_cr_behind_a_tile_seam", texts, planted, at_eof=False)
    yield _case("stream_ends_in_a_lone_cr_behind_a_tile_seam", texts, planted, at_eof=True)
    texts, planted, _ = twins(311, 8191, "CR")
    yield _case("prefix_ends_in_cr_on_a_tile_s_last_byte", texts, planted, at_eof=False)
    # the empty line read at the end of the stream completes the last record
    texts, planted, _ = twins(312, 8191, "LF")
    texts = [t + b"@last\n\n+\n" for t in texts]
    yield _case("last_record_completed_by_the_empty_line", texts, planted)
    yield _case("last_record_left_open_in_a_prefix", texts, planted, at_eof=False)
    # max_pairs cuts behind a "\r\n" that a tile seam splits: consumed is the seam's offset + 1
    for kind, T in (("CRLF", 4095), ("CRLF", 4096), ("CR", 4095), ("LF", 4095)):
        texts, planted, streams = twins(320 + T + len(kind), T, kind, more=30)
        cut = streams[0].hits[0][0] + 1
        assert streams[1].hits[0][0] + 1 == cut
        yield _case("max_pairs_cuts_behind_%s_at_%d" % (kind, T), texts, planted, max_pairs=cut)
        yield _case("max_pairs_cuts_behind_%s_at_%d_in_a_prefix" % (kind, T), texts, planted, max_pairs=cut, at_eof=False)
    texts, planted, _ = twins(330, 8191, "LF")
    yield _case("blank_lines_behind_the_last_record", [texts[0] + b"\n\n", texts[1] + b"\r\n\r"], planted)


def id_window_cases():
    """find_byte's 16-byte windows over the header: lengths, the first space and the first '/' at every offset, and both bytes
    within the 15 bytes BEHIND a header's end (they must not cut the identifier), in R1's last record too, where those bytes
    are R2's"""
    long = b"@abcdefghijklmnopqrstuvwxyzABCDEFGHI"
    heads = [(b"@" + b"h" * 40)[:n] for n in (0, 1, 2, 15, 16, 17, 18, 31, 32, 33, 34)] + [long]
    for k in range(34):
        heads += [long[:k] + b" " + long[k + 1:], long[:k] + b"/" + long[k + 1:]]
    for i, j in ((5, 3), (3, 5), (16, 15), (15, 16), (17, 33), (33, 17), (0, 1), (1, 0), (31, 32), (32, 31), (16, 32), (32, 16)):
        h = bytearray(long)
        h[i], h[j] = 32, 47
        heads.append(bytes(h))
    recs = [(h, b"ACGTACGTAC"[:k % 11], b"IIIIIIIIII"[:k % 11]) for k, h in enumerate(heads)]
    for n in (1, 2, 3, 14, 15, 16, 17, 18, 30, 31, 32, 33, 34):      # '/' and ' ' just behind the header's end
        recs += [((b"@" + b"k" * 40)[:n], b"", b""), ((b"@" + b"k" * 40)[:n], b"AC", b"//"), (b"@ sp/ace", b"", b"")]
    eols = (b"\n", b"\r\n", b"\r")

    def text(rs, shift):
        out = []
        for k, (h, s, q) in enumerate(rs):
            quiet = not s or h.startswith(b"@k")      # (a lone "\r" before an empty line would fuse with its terminator)
            e = [b"\n"] * 4 if quiet else [eols[(k + shift + i) % 3] for i in range(3)] + [eols[(k + shift) % 2]]
            out.append(h + e[0] + s + e[1] + b"+" + e[2] + q + e[3])
        return b"".join(out)
    r1 = text(recs, 0) + b"@" + b"z" * 15 + b"\n\n+\n"                  # its quality line is the empty line at the end
    r2 = b"@q/2 x\n\n+\n\n" + text(recs[::-1], 1)
    yield _case("identifier_windows", [r1, r2])
    yield _case("identifier_windows_single_end", [r1 + b"\n" + r2])      # (the empty quality line written out)


def error_cases(g):
    texts, planted, _ = build(400, g, 500, [[Target(4095, "LF", 1)]] * 2, twins=True, end_at_targets=True)
    bad = texts[0].rstrip(b"\r\n") + b"I\n"
    yield _case("quality_line_of_another_length_in_a_record_cut_by_a_tile_seam", [bad, texts[1]], planted, error="quality line")
    yield _case("the_same_in_r2", [texts[1], bad], planted, error="quality line")
    texts, planted, _ = build(401, g, 500, [[Target(8191, "LF", 3)]] * 2, twins=True, end_at_targets=True)
    n = len(records(texts[1])[0])
    short = texts[1][:records(texts[1], n - 1)[3]]
    yield _case("r2_one_record_short", [texts[0], short], planted, error="mismatch in R1 and R2 size")
    yield _case("r1_one_record_short", [short, texts[1]], planted, error="mismatch in R1 and R2 size")


def small_cases(synth):
    """every case but the 16 MiB one"""
    g = genomes(synth, "small")
    for gen in (matrix_cases(g), long_line_cases(g), end_cases(g), id_window_cases(), error_cases(g)):
        for c in gen:
            yield c


def big_case(synth):
    """past the first scan tile: the scan of csrc/scan.hip takes SCAN_TILE = 4 096 values per tile and the index counts one
    value per FQ_TILE = 4 096 bytes of text (csrc/fastq_index.hip), so a stream of more than 4 096 x 4 096 bytes = 16 MiB
    sends the scan of the tile counts to its second tile; more than 4 096 records do the same to the two length scans"""
    g = genomes(synth, "big")
    targets = [[Target(16384 * 1030 - 1, "CRLF", 3), Target(16384 * 1040, "CR", 1)], [Target(16384 * 1035 - 1, "CR", 0)]]
    texts, planted, _ = build(500, g, 500, targets, max_pad=700, min_records=0, planted_frac=0.5)
    assert min(len(t) for t in texts) > 4096 * 4096 and len(planted) > 4096
    return _case("past_the_first_scan_tile", texts, planted, genome="big")
