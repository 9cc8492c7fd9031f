"""A strict reader for the output of include/kslam_samseq.h: SAM text whose rows may carry SEQ and QUAL, and BAM records with
l_seq >= 0, rendered back as the SAM text `samtools view` prints.  (bam_check.py stays the reader for switch-off output.)"""
import re
import struct

import bam_check as B
import bgzf_check

BamError = B.BamError
NT16 = b"=ACMGRSVTWYHKDBN"
_CIGAR = re.compile(rb"(\d+)([MIDNSHP=X])")


class SamError(ValueError):
    pass


def query_length(ops):
    """[(length, op letter)] -> the M + I + S (+ = X) lengths: what SEQ must be as long as"""
    return sum(n for n, op in ops if op in "MIS=X")


def parse_cigar(text):
    ops = [(int(n), op.decode()) for n, op in _CIGAR.findall(text)]
    if b"".join(b"%d%s" % (n, op.encode()) for n, op in ops) != text:
        raise SamError("malformed CIGAR %r" % text)
    return ops


def sam_rows(text):
    """SAM text (no header) -> list of field lists, every row checked: >= 11 columns, SEQ / QUAL of one length (or QUAL "*"),
    SEQ as long as the CIGAR's M + I + S when both are there, QUAL within phred+33 0..93"""
    if text and not text.endswith(b"\n"):
        raise SamError("the text does not end with a newline")
    rows = []
    for k, line in enumerate(text.split(b"\n")[:-1]):
        f = line.split(b"\t")
        if len(f) < 11:
            raise SamError("row %d has %d columns" % (k, len(f)))
        seq, qual = f[9], f[10]
        if seq == b"":
            raise SamError("row %d: empty SEQ" % k)
        if seq == b"*":
            if qual != b"*":
                raise SamError("row %d: QUAL without SEQ" % k)
        else:
            if qual != b"*" and len(qual) != len(seq):
                raise SamError("row %d: SEQ has %d bases, QUAL %d" % (k, len(seq), len(qual)))
            if qual != b"*" and not all(33 <= c <= 126 for c in qual):
                raise SamError("row %d: QUAL outside phred+33 0..93" % k)
            if f[5] not in (b"*", b""):
                want = query_length(parse_cigar(f[5]))
                if want != len(seq):
                    raise SamError("row %d: SEQ has %d bases, the CIGAR %d" % (k, len(seq), want))
        rows.append(f)
    return rows


def records(data, pos, refs):
    """-> list of SAM lines (without their newline) with SEQ / QUAL decoded, checking every record"""
    names = [n for n, _ in refs]
    lines = []
    n = len(data)
    while pos < n:
        raw, at = B._take(data, pos, 4, "block_size")
        (block_size,) = struct.unpack("<i", raw)
        end = at + block_size
        if block_size < 32 or end > n:
            raise BamError("block_size %d does not fit at %d" % (block_size, pos))
        (ref_id, p, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen) = struct.unpack_from("<iiBBHHHiiii", data, at)
        at += 32
        if l_seq < 0:
            raise BamError("negative l_seq at %d" % pos)
        if at + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > end:
            raise BamError("block_size %d does not cover read name, CIGAR, seq and qual at %d" % (block_size, pos))
        name = data[at:at + l_name]
        if l_name < 1 or name[-1:] != b"\0" or b"\0" in name[:-1]:
            raise BamError("read name without its NUL at %d" % pos)
        at += l_name
        ops = struct.unpack_from("<%dI" % n_cig, data, at)
        at += 4 * n_cig
        if n_cig and l_seq:
            want = query_length([(c >> 4, B.CIGAR_OPS[c & 15]) for c in ops])
            if want != l_seq:
                raise BamError("l_seq %d, the CIGAR's M + I + S lengths %d at %d" % (l_seq, want, pos))
        packed = data[at:at + (l_seq + 1) // 2]
        at += (l_seq + 1) // 2
        if l_seq & 1 and packed[-1] & 15:
            raise BamError("odd l_seq %d with a non-zero last nibble at %d" % (l_seq, pos))
        seq = bytes(NT16[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq)) or b"*"
        q = data[at:at + l_seq]
        at += l_seq
        if l_seq and q == b"\xff" * l_seq:
            qual = b"*"
        else:
            if any(c > 93 for c in q):
                raise BamError("QUAL byte above 93 at %d" % pos)
            qual = bytes(c + 33 for c in q) or b"*"
        span = sum(c >> 4 for c in ops if B.CIGAR_OPS[c & 15] in "MDN=X") if n_cig else 0
        if (flag & 0x4) or not n_cig:
            span = 0
        if bin_ != B.reg2bin(p, p + max(1, span)):
            raise BamError("bin %d, expected %d at %d" % (bin_, B.reg2bin(p, p + max(1, span)), pos))
        if not (0 <= ref_id < len(names)) or not (-1 <= nref < len(names)):
            raise BamError("reference id outside the header at %d" % pos)
        tags = B._tags(data, at, end)
        cigar = b"".join(b"%d%s" % (c >> 4, B.CIGAR_OPS[c & 15].encode()) for c in ops) or b"*"
        rnext = b"*" if nref < 0 else b"=" if nref == ref_id else names[nref]
        fields = [name[:-1], b"%d" % flag, names[ref_id], b"%d" % (p + 1), b"%d" % mapq, cigar, rnext, b"%d" % (npos + 1),
                  b"%d" % tlen, seq, qual] + tags
        lines.append(b"\t".join(fields))
        pos = end
    return lines


def decode(data):
    """uncompressed BAM -> (header text, SAM lines joined with newlines)"""
    text, refs, pos = B.parse_header(data)
    return text, b"".join(line + b"\n" for line in records(data, pos, refs))


def check(blob):
    """a BAM file (BGZF) -> the SAM text samtools view -h prints for it"""
    text, body = decode(bgzf_check.check(blob))
    return text + body


def strip_text(text):
    """SAM text -> the same with columns 10 and 11 replaced by "*": what the switch-off route writes"""
    out = []
    for f in sam_rows(text):
        out.append(b"\t".join(f[:9] + [b"*", b"*"] + f[11:]) + b"\n")
    return b"".join(out)


def strip_records(data):
    """BAM records (no header) -> the same with seq / qual removed and l_seq, block_size patched"""
    out, pos = [], 0
    while pos < len(data):
        (block_size,) = struct.unpack_from("<i", data, pos)
        rec = data[pos + 4:pos + 4 + block_size]
        l_name, n_cig = rec[8], struct.unpack_from("<H", rec, 12)[0]
        (l_seq,) = struct.unpack_from("<i", rec, 16)
        at = 32 + l_name + 4 * n_cig
        body = rec[:16] + struct.pack("<i", 0) + rec[20:at] + rec[at + (l_seq + 1) // 2 + l_seq:]
        out.append(struct.pack("<i", len(body)) + body)
        pos += 4 + block_size
    return b"".join(out)
