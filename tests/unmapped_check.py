"""A strict reader for BAM written with include/kslam_samunmapped.h on: samseq_check's record reader, which also accepts an
unplaced record -- refID -1 -- but only together with all of: FLAG 0x4, pos -1, n_cigar_op 0, mapq 0, bin 4680, no tags (and
next_refID -1, next_pos -1, tlen 0).  Such a record renders as `samtools view` prints it: RNAME "*", POS 0, RNEXT "*".
(bam_check.py and samseq_check.py refuse refID < 0, and stay the readers for switch-off output.)"""
import struct

import bam_check as B
import bgzf_check
import samseq_check as S

BamError = B.BamError
UNPLACED_BIN = 4680   # htslib's reg2bin(-1, 0)


def records(data, pos, refs):
    """-> list of SAM lines (without their newline), checking every record"""
    lines = []
    n = len(data)
    while pos < n:
        raw, at = B._take(data, pos, 4, "block_size")
        (block_size,) = struct.unpack("<i", raw)
        end = at + block_size
        if block_size < 32 or end > n:
            raise BamError("block_size %d does not fit at %d" % (block_size, pos))
        (ref_id, p, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen) = struct.unpack_from("<iiBBHHHiiii", data, at)
        if ref_id >= 0:   # a placed record: samseq_check's rules
            lines += S.records(data[pos:end], 0, refs)
            pos = end
            continue
        if ref_id != -1:
            raise BamError("refID %d at %d" % (ref_id, pos))
        for what, got, want in (("pos", p, -1), ("n_cigar_op", n_cig, 0), ("mapq", mapq, 0), ("bin", bin_, UNPLACED_BIN),
                                ("next_refID", nref, -1), ("next_pos", npos, -1), ("tlen", tlen, 0)):
            if got != want:
                raise BamError("unplaced record at %d: %s is %d, not %d" % (pos, what, got, want))
        if not flag & 0x4:
            raise BamError("unplaced record at %d without FLAG 0x4 (%d)" % (pos, flag))
        at += 32
        if l_seq < 0 or at + l_name + (l_seq + 1) // 2 + l_seq != end:
            raise BamError("unplaced record at %d: block_size %d is not read name + seq + qual (tags?)" % (pos, block_size))
        name = data[at:at + l_name]
        if l_name < 1 or name[-1:] != b"\0" or b"\0" in name[:-1]:
            raise BamError("read name without its NUL at %d" % pos)
        at += l_name
        packed = data[at:at + (l_seq + 1) // 2]
        at += (l_seq + 1) // 2
        if l_seq & 1 and packed[-1] & 15:
            raise BamError("odd l_seq %d with a non-zero last nibble at %d" % (l_seq, pos))
        seq = bytes(S.NT16[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq)) or b"*"
        q = data[at:at + l_seq]
        if l_seq and q == b"\xff" * l_seq:
            qual = b"*"
        else:
            if any(c > 93 for c in q):
                raise BamError("QUAL byte above 93 at %d" % pos)
            qual = bytes(c + 33 for c in q) or b"*"
        lines.append(b"\t".join([name[:-1], b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, qual]))
        pos = end
    return lines


def decode(data):
    """uncompressed BAM -> (header text, SAM lines joined with newlines)"""
    text, refs, pos = B.parse_header(data)
    return text, b"".join(line + b"\n" for line in records(data, pos, refs))


def decode_records(data):
    """BAM records without a header and without placed records -> SAM lines joined with newlines"""
    return b"".join(line + b"\n" for line in records(data, 0, []))


def check(blob):
    """a BAM file (BGZF) -> the SAM text samtools view -h prints for it"""
    text, body = decode(bgzf_check.check(blob))
    return text + body
