"""A strict BGZF validator (the framing of bgzip / htslib, SAMv1 section 4.1) for the files include/kslam_bgzf.h writes."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_INPUT = 65280      # htslib's BGZF_BLOCK_SIZE
MAX_MEMBER = 65536


class BgzfError(ValueError):
    pass


def members(blob):
    """-> list of (offset, size, btype, isize); raises BgzfError on the first thing that is not strict BGZF as
    include/kslam_bgzf.h promises it: one deflate block per member, BTYPE 00 or 01, ending in exactly one EOF marker."""
    out, pos, n = [], 0, len(blob)
    while pos < n:
        if n - pos < 28:
            raise BgzfError("truncated member at %d" % pos)
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", blob, pos)
        if (id1, id2, cm, flg, xlen) != (0x1F, 0x8B, 8, 4, 6):
            raise BgzfError("bad gzip header at %d" % pos)
        si1, si2, slen, bsize = struct.unpack_from("<BBHH", blob, pos + 12)
        if (si1, si2, slen) != (ord("B"), ord("C"), 2):
            raise BgzfError("no BC extra field at %d" % pos)
        size = bsize + 1
        if size > MAX_MEMBER or pos + size > n or size < 26:
            raise BgzfError("BSIZE %d does not fit at %d" % (bsize, pos))
        body = blob[pos + 18:pos + size - 8]
        crc, isize = struct.unpack_from("<II", blob, pos + size - 8)
        if not body:
            raise BgzfError("no deflate data at %d" % pos)
        bfinal, btype = body[0] & 1, (body[0] >> 1) & 3
        if bfinal != 1 or btype not in (0, 1):
            raise BgzfError("first block at %d: BFINAL %d BTYPE %d" % (pos, bfinal, btype))
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(body)
        except zlib.error as e:
            raise BgzfError("inflate failed at %d: %s" % (pos, e))
        if not d.eof or d.unused_data or d.unconsumed_tail:
            raise BgzfError("member at %d does not end where BSIZE says" % pos)
        if zlib.crc32(data) != crc or len(data) != isize:
            raise BgzfError("CRC32 / ISIZE mismatch at %d" % pos)
        if isize > MAX_INPUT:
            raise BgzfError("ISIZE %d > %d at %d" % (isize, MAX_INPUT, pos))
        out.append((pos, size, btype, isize))
        pos += size
    if not out or blob[out[-1][0]:] != EOF_MARKER:
        raise BgzfError("the file does not end in the EOF marker")
    for off, _size, _btype, isize in out[:-1]:
        if isize == 0:
            raise BgzfError("empty member at %d before the end" % off)
    return out


def check(blob):
    """validate and return the decompressed bytes"""
    ms = members(blob)
    return b"".join(zlib.decompressobj(-15).decompress(blob[o + 18:o + s - 8]) for o, s, _, _ in ms)
