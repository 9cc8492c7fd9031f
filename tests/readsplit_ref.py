"""The reads split (include/kslam_readsplit.h) restated in plain Python: the reader's line rule, the record rule, the partition;
and the texts the host and the device tests both run."""
import re

import numpy as np

READ_PAIR_DT = np.dtype([("r1_read", "<u4"), ("r2_read", "<u4"), ("first", "<u8"), ("count", "<u8")])


def lines(text, at_eof=True):
    """the lines the reader takes from `text`: a line ends at "\\r\\n", a lone "\\r" or "\\n"; at the true end of the stream the
    unterminated rest (if any) and then one more, empty, line are read; before it, a closing "\\r" may be half a "\\r\\n" and is
    not looked at"""
    if not at_eof and text.endswith(b"\r"):
        text = text[:-1]
    parts = re.split(rb"\r\n|\r|\n", text)
    if not at_eof:
        return parts[:-1]
    return parts + ([b""] if parts[-1] else [])


def records(text, max_pairs=0, at_eof=True):
    """the records taken: four lines each, whatever they hold, every line followed by one "\\n" """
    ln = lines(text, at_eof)
    n = len(ln) // 4
    if max_pairs:
        n = min(n, max_pairs)
    return [b"".join(x + b"\n" for x in ln[4 * r:4 * r + 4]) for r in range(n)]


def split(r1, r2, classified, which=3, max_pairs=0, at_eof=True):
    """-> ([classified R1, classified R2, unclassified R1, unclassified R2], (n classified, n unclassified)); None for a stream
    that is not asked for; r2 None: single-end.  `classified`: the record numbers in the final read pairs."""
    streams = [records(r1, max_pairs, at_eof)] + ([records(r2, max_pairs, at_eof)] if r2 is not None else [])
    assert all(len(s) == len(streams[0]) for s in streams)
    sel = set(int(c) for c in classified)
    out = [None] * 4
    for k, recs in enumerate(streams):
        if which & 1:
            out[k] = b"".join(x for r, x in enumerate(recs) if r in sel)
        if which & 2:
            out[2 + k] = b"".join(x for r, x in enumerate(recs) if r not in sel)
    n = len(streams[0])
    n_sel = sum(1 for r in range(n) if r in sel)
    return out, (n_sel, n - n_sel)


def merge(classified_block, unclassified_block, classified, n):
    """the partition property's other direction: the two streams merged back by record number"""
    def cut(block):
        ln = block.split(b"\n")[:-1]
        assert len(ln) % 4 == 0
        return [b"".join(x + b"\n" for x in ln[4 * r:4 * r + 4]) for r in range(len(ln) // 4)]
    c, u = cut(classified_block), cut(unclassified_block)
    sel = set(int(x) for x in classified)
    assert len(c) == len(sel) and len(c) + len(u) == n
    ci, ui = iter(c), iter(u)
    return b"".join(next(ci) if r in sel else next(ui) for r in range(n))


def read_pairs(classified, n, paired=True):
    """read pairs in the block layout [R1 | R2] (single-end: r2_read = 0, as pairs.hip leaves it)"""
    rp = np.zeros(len(classified), dtype=READ_PAIR_DT)
    rp["r1_read"] = np.asarray(classified, dtype=np.uint32)
    rp["r2_read"] = rp["r1_read"] + n if paired else 0
    rp["count"] = 1
    rp["first"] = np.arange(len(classified))
    return rp


def record(header, n_bases, term, seed=0):
    rng = np.random.default_rng(1000 * n_bases + seed)
    bases = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n_bases))
    qual = bytes(rng.integers(33, 74, n_bases, dtype=np.uint8))
    return header + term + bases + term + b"+" + term + qual + term


def text_of(n, term=b"\n", n_bases=37, mate=1, header=None):
    return b"".join(record(header if header is not None else b"@r%d/%d" % (r, mate), n_bases + (r % 5 if n_bases > 4 else 0),
                           term[r % len(term)] if isinstance(term, list) else term, seed=mate) for r in range(n))


BASES_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65]


def cases():
    """(name, r1, r2 or None, max_pairs, at_eof)"""
    out = []
    for name, term in [("lf", b"\n"), ("crlf", b"\r\n"), ("cr", b"\r"), ("mixed", [b"\n", b"\r\n", b"\r"])]:
        out.append((name, text_of(7, term), text_of(7, term, mate=2), 0, True))
    # the last record without its terminator (R1), and with one (R2)
    out.append(("unterminated", text_of(5)[:-1], text_of(5, mate=2), 0, True))
    out.append(("unterminated_crlf", text_of(5, b"\r\n")[:-2], text_of(5, b"\r\n", mate=2)[:-2], 0, True))
    # three lines, then the end of the stream: its empty line completes the record (empty bases, empty quality)
    out.append(("completed_by_eof", text_of(3) + b"@last\n\n+\n", text_of(3, mate=2) + b"@last\r\n\r\n+\r\n", 0, True))
    heads = [b"", b"@", b"@read 1:N:0 comment", b"@read/1", b"@r/1 x/y"]
    out.append(("headers", b"".join(record(h, 20, b"\n") for h in heads), b"".join(record(h, 21, b"\n", 2) for h in heads), 0, True))
    out.append(("headers_crlf", b"".join(record(h, 20, b"\r\n") for h in heads), b"".join(record(h, 21, b"\n", 2) for h in heads), 0, True))
    out.append(("bases_lengths", b"".join(record(b"@b%d" % n, n, b"\n") for n in BASES_LENGTHS),
                b"".join(record(b"@b%d/2" % n, n, b"\n", 2) for n in reversed(BASES_LENGTHS)), 0, True))
    out.append(("bases_lengths_crlf", b"".join(record(b"@b%d" % n, n, b"\r\n") for n in BASES_LENGTHS),
                b"".join(record(b"@b%d/2" % n, n, b"\r", 2) for n in BASES_LENGTHS), 0, True))
    # max_pairs cuts the text in the middle; not at the end of the stream (and a closing "\r" that may be half a "\r\n")
    out.append(("max_pairs_mid", text_of(9), text_of(9, mate=2), 4, False))
    out.append(("not_eof_trailing_cr", text_of(7, b"\r"), text_of(6, b"\r\n", mate=2) + b"@x\r", 0, False))
    out.append(("single_end", text_of(7), None, 0, True))
    out.append(("single_end_mixed", text_of(8, [b"\r\n", b"\n"])[:-1], None, 3, True))
    # long records: the copy takes a whole wavefront per record
    out.append(("long_records", text_of(5, n_bases=1500), text_of(5, [b"\n", b"\r\n"], n_bases=1300, mate=2), 0, True))
    out.append(("empty", b"", b"", 0, True))
    return out


def patterns(n):
    """none classified, all classified, alternating, and one of every three"""
    return {"none": [], "all": list(range(n)), "alternating": list(range(0, n, 2)), "odd": list(range(1, n, 2))}
