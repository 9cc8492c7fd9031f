"""A strict BAM reader (SAMv1 section 4.2) for the files include/kslam_bam.h writes: every record checked field by field,
rendered back as the SAM text `samtools view -h` prints."""
import struct

import bgzf_check

MAGIC = b"BAM\x01"
CIGAR_OPS = "MIDNSHP=X"
INT_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class BamError(ValueError):
    pass


def reg2bin(beg, end):
    """htslib's hts_reg2bin(beg, end, 14, 5)"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def int_type(v):
    """the width htslib's sam_parse1 gives an integer tag"""
    if v >= 0:
        return "C" if v <= 0xFF else "S" if v <= 0xFFFF else "I"
    return "c" if v >= -0x80 else "s" if v >= -0x8000 else "i"


def _take(data, pos, n, what):
    if pos + n > len(data):
        raise BamError("truncated %s at %d" % (what, pos))
    return data[pos:pos + n], pos + n


def parse_header(data):
    """-> (header text, [(name, length)], offset of the first record)"""
    if data[:4] != MAGIC:
        raise BamError("bad magic")
    raw, pos = _take(data, 4, 4, "l_text")
    (l_text,) = struct.unpack("<i", raw)
    text, pos = _take(data, pos, l_text, "header text")
    raw, pos = _take(data, pos, 4, "n_ref")
    (n_ref,) = struct.unpack("<i", raw)
    refs = []
    for _ in range(n_ref):
        raw, pos = _take(data, pos, 4, "l_name")
        (l_name,) = struct.unpack("<i", raw)
        name, pos = _take(data, pos, l_name, "reference name")
        if l_name < 1 or name[-1:] != b"\0" or b"\0" in name[:-1]:
            raise BamError("reference name without its NUL")
        raw, pos = _take(data, pos, 4, "l_ref")
        refs.append((name[:-1], struct.unpack("<i", raw)[0]))
    sq = []
    for line in text.split(b"\n"):
        if line.startswith(b"@SQ\t"):
            f = dict((t[:2], t[3:]) for t in line.split(b"\t")[1:])
            sq.append((f.get(b"SN"), int(f.get(b"LN", b"-1"))))
    if sq != refs:
        raise BamError("the header's @SQ lines disagree with the reference list")
    return text, refs, pos


def _tags(data, pos, end):
    out = []
    while pos < end:
        if end - pos < 3:
            raise BamError("truncated tag at %d" % pos)
        tag, t = data[pos:pos + 2].decode(), chr(data[pos + 2])
        pos += 3
        if t in INT_TYPES:
            fmt = INT_TYPES[t]
            k = struct.calcsize(fmt)
            if pos + k > end:
                raise BamError("truncated integer tag %s" % tag)
            (v,) = struct.unpack_from(fmt, data, pos)
            if int_type(v) != t:
                raise BamError("tag %s: %d stored as %s, htslib stores it as %s" % (tag, v, t, int_type(v)))
            pos += k
            out.append(b"%s:i:%d" % (tag.encode(), v))
        elif t == "Z":
            z = data.find(b"\0", pos, end)
            if z < 0:
                raise BamError("Z tag %s without its NUL" % tag)
            out.append(b"%s:Z:%s" % (tag.encode(), data[pos:z]))
            pos = z + 1
        else:
            raise BamError("unknown tag type %r" % t)
    return out


def records(data, pos, refs):
    """-> list of SAM lines (without their newline), checking every record"""
    names = [n for n, _ in refs]
    lines = []
    n = len(data)
    while pos < n:
        raw, at = _take(data, pos, 4, "block_size")
        (block_size,) = struct.unpack("<i", raw)
        end = at + block_size
        if block_size < 32 or end > n:
            raise BamError("block_size %d does not fit at %d" % (block_size, pos))
        (ref_id, p, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen) = struct.unpack_from("<iiBBHHHiiii", data, at)
        at += 32
        if l_seq != 0:
            raise BamError("l_seq %d: this product writes no SEQ / QUAL" % l_seq)
        if at + l_name + 4 * n_cig > end:
            raise BamError("read name / CIGAR past block_size at %d" % pos)
        name = data[at:at + l_name]
        if l_name < 1 or name[-1:] != b"\0" or b"\0" in name[:-1]:
            raise BamError("read name without its NUL at %d" % pos)
        at += l_name
        ops = struct.unpack_from("<%dI" % n_cig, data, at)
        at += 4 * n_cig
        span = sum(c >> 4 for c in ops if CIGAR_OPS[c & 15] in "MDN=X") if n_cig else 0
        if (flag & 0x4) or not n_cig:
            span = 0
        if bin_ != reg2bin(p, p + max(1, span)):
            raise BamError("bin %d, expected %d at %d" % (bin_, reg2bin(p, p + max(1, span)), pos))
        if not (0 <= ref_id < len(names)) or not (-1 <= nref < len(names)):
            raise BamError("reference id outside the header at %d" % pos)
        tags = _tags(data, at, end)
        cigar = b"".join(b"%d%s" % (c >> 4, CIGAR_OPS[c & 15].encode()) for c in ops) or b"*"
        rnext = b"*" if nref < 0 else b"=" if nref == ref_id else names[nref]
        fields = [name[:-1], b"%d" % flag, names[ref_id], b"%d" % (p + 1), b"%d" % mapq, cigar, rnext, b"%d" % (npos + 1),
                  b"%d" % tlen, b"*", b"*"] + tags
        lines.append(b"\t".join(fields))
        pos = end
    return lines


def decode(data):
    """uncompressed BAM -> (header text, SAM lines joined with newlines)"""
    text, refs, pos = parse_header(data)
    lines = records(data, pos, refs)
    return text, b"".join(line + b"\n" for line in lines)


def check(blob):
    """a BAM file (BGZF) -> the SAM text samtools view -h prints for it"""
    text, body = decode(bgzf_check.check(blob))
    return text + body
