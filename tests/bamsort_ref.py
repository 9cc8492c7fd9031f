"""The coordinate-sorted BAM of include/kslam_bamsort.h restated in plain Python: records cut out of a block_size chain, the
stable sort by (refID as unsigned, pos + 1 as unsigned), the header's sort order, and the BAI bytes from the definition, given the
compressed size of every member.  A yardstick, not the code under test: nothing here is shared with the library."""
import struct

MEMBER_IN = 65280
PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def record(ref, pos, name=b"r", flag=0, cigar=(), seq_len=0, tags=b"", mapq=0, next_ref=-1, next_pos=-1, tlen=0):
    """one BAM record; cigar: [(length, op number)]; SEQ is seq_len 'A's with quality 30; bin by the definition"""
    span = sum(n for n, op in cigar if op in REF_OPS) if cigar and not flag & 4 else 0
    name = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name), mapq, reg2bin(pos, pos + max(1, span)) if pos >= 0 else 4680, len(cigar), flag, seq_len,
                       next_ref, next_pos, tlen)
    body += name + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + b"\x11" * ((seq_len + 1) // 2) + b"\x1e" * seq_len + tags
    return struct.pack("<i", len(body)) + body


def split(data):
    """the records of a chain, as bytes; ValueError when the chain does not end at the end"""
    out, pos = [], 0
    while pos < len(data):
        if len(data) - pos < 4:
            raise ValueError("block_size chain")
        (bs,) = struct.unpack_from("<I", data, pos)
        if bs < 32 or pos + 4 + bs > len(data):
            raise ValueError("block_size chain")
        out.append(bytes(data[pos:pos + 4 + bs]))
        pos += 4 + bs
    return out


def fields(rec):
    """-> dict(ref, pos, flag, span, unmapped): span = max(1, reflen)"""
    ref, pos, l_name, _, _, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    ops = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    reflen = 0 if flag & 4 or not n_cig else sum(c >> 4 for c in ops if c & 15 in REF_OPS)
    return {"ref": ref, "pos": pos, "flag": flag, "span": max(1, reflen), "unmapped": bool(flag & 4)}


def key(rec):
    ref, pos = struct.unpack_from("<ii", rec, 4)
    return (ref & 0xFFFFFFFF, (pos + 1) & 0xFFFFFFFF)


def sort_batches(batches):
    """batches in seq order -> the sorted record stream (Python's sort is stable)"""
    recs = [r for b in batches for r in split(b)]
    return b"".join(sorted(recs, key=key))


def coordinate_header(text):
    if not (text.startswith(b"@HD") and text[3:4] in (b"\t", b"\n", b"")):
        return b"@HD\tVN:1.0\tSO:coordinate\n" + text
    line, nl, rest = text.partition(b"\n")
    f = line.split(b"\t")
    if any(x.startswith(b"SO:") for x in f[1:]):
        k = next(i for i, x in enumerate(f) if i and x.startswith(b"SO:"))
        f[k] = b"SO:coordinate"
    else:
        f.append(b"SO:coordinate")
    return b"\t".join(f) + nl + rest


def bam_header(text, refs):
    """refs: [(name, length)]"""
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def voff_of(member_sizes, header_clen, total):
    """-> f(stream offset) = virtual offset"""
    starts = [header_clen]
    for m in member_sizes:
        starts.append(starts[-1] + m)
    assert len(member_sizes) == (total + MEMBER_IN - 1) // MEMBER_IN

    def f(o):
        if o >= total:
            return starts[len(member_sizes)] << 16
        return starts[o // MEMBER_IN] << 16 | o % MEMBER_IN
    return f


def bai(stream, n_ref, member_sizes, header_clen):
    """the BAI bytes of a sorted record stream, from the definition"""
    voff = voff_of(member_sizes, header_clen, len(stream))
    recs, at = [], 0
    for r in split(stream):
        f = fields(r)
        f["start"], f["end_v"] = voff(at), voff(at + len(r))
        at += len(r)
        recs.append(f)
    out = b"BAI\x01" + struct.pack("<i", n_ref)
    for ref in range(n_ref):
        mine = [(i, f) for i, f in enumerate(recs) if f["ref"] == ref]
        if not mine:
            out += struct.pack("<ii", 0, 0)
            continue
        bins = {}
        for i, f in mine:
            if f["pos"] < 0:
                continue
            b = reg2bin(f["pos"], f["pos"] + f["span"])
            before = recs[i - 1] if i else None
            joins = before is not None and before["ref"] == ref and before["pos"] >= 0 and reg2bin(before["pos"], before["pos"] + before["span"]) == b
            if joins:
                bins[b][-1][1] = f["end_v"]
            else:
                bins.setdefault(b, []).append([f["start"], f["end_v"]])
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b])
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, mine[0][1]["start"], mine[-1][1]["end_v"], sum(not f["unmapped"] for _, f in mine),
                           sum(f["unmapped"] for _, f in mine))
        placed = [f for _, f in mine if f["pos"] >= 0]
        n_intv = 1 + max((f["pos"] + f["span"] - 1) >> 14 for f in placed) if placed else 0
        io = [None] * n_intv
        for f in placed:
            for w in range(f["pos"] >> 14, ((f["pos"] + f["span"] - 1) >> 14) + 1):
                io[w] = f["start"] if io[w] is None else min(io[w], f["start"])
        for w in range(n_intv - 2, -1, -1):
            if io[w] is None:
                io[w] = io[w + 1]
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in io)
    return out + struct.pack("<Q", sum(f["ref"] < 0 for f in recs))
