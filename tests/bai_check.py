"""A strict checker of a coordinate-sorted BAM file and its BAI index (include/kslam_bamsort.h), independent of the library and
of tests/bamsort_ref.py: it does not rebuild the index, it checks what an index must mean.
  - the record stream is non-decreasing in (refID as unsigned, pos + 1 as unsigned);
  - every record with refID >= 0 and pos >= 0 lies in exactly one chunk, a chunk of its own bin; records without lie in none;
  - a bin's chunks ascend and are disjoint, begin and end on record boundaries, and hold records of that (reference, bin) only;
  - every ioffset[w] is, by brute force, the smallest start of a record overlapping window w, or the next higher window's value;
  - the pseudo-bins' spans and counts and n_no_coor are right by counting;
  - seeking to every chunk start -- inflating the member at its coffset alone -- lands on a record's first byte.
Members are inflated with tests/inflate_ref.py, the header is read with tests/bam_check.py."""
import struct

import bam_check
import inflate_ref

PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)


class BaiError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise BaiError(what)


def _parse(bai):
    _need(bai[:4] == b"BAI\x01", "magic")
    pos = 4

    def get(fmt):
        nonlocal pos
        _need(pos + struct.calcsize(fmt) <= len(bai), "truncated index")
        v = struct.unpack_from(fmt, bai, pos)
        pos += struct.calcsize(fmt)
        return v
    (n_ref,) = get("<i")
    refs = []
    for _ in range(n_ref):
        (n_bin,) = get("<i")
        bins = []
        for _ in range(n_bin):
            b, n_chunk = get("<Ii")
            bins.append((b, [get("<QQ") for _ in range(n_chunk)]))
        (n_intv,) = get("<i")
        refs.append((bins, [get("<Q")[0] for _ in range(n_intv)]))
    (n_no_coor,) = get("<Q")
    _need(pos == len(bai), "bytes behind the index")
    return refs, n_no_coor


def check(bam, bai):
    """-> dict(n_records, n_chunks, n_no_coor); BaiError (or the readers' errors) on the first thing that is wrong"""
    ms = inflate_ref.members(bam)
    _need(ms and bam[ms[-1][0]:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"), "no EOF marker at the end")
    data, _ = inflate_ref.inflate(bam)
    ustart, u = {}, 0                         # member offset -> (start in the inflated data, isize)
    for at, size in ms:
        (isize,) = struct.unpack_from("<I", bam, at + size - 4)
        ustart[at] = (u, isize)
        u += isize

    def absolute(v):
        c, uo = v >> 16, v & 0xFFFF
        _need(c in ustart, "coffset %d is not the start of a member" % c)
        s, isize = ustart[c]
        _need(uo < isize or (uo == 0 and c == ms[-1][0]), "uoffset %d at or behind its member's end (a position at a member's end belongs to the next)" % uo)
        return s + uo

    _, names, pos = bam_check.parse_header(data)
    recs = []
    while pos < len(data):
        _need(len(data) - pos >= 36, "truncated record")
        bs, ref, p, l_name, _, _, n_cig, flag = struct.unpack_from("<iiiBBHHH", data, pos)
        _need(bs >= 32 and pos + 4 + bs <= len(data) and 32 + l_name + 4 * n_cig <= bs, "block_size")
        _need(-1 <= ref < len(names), "refID")
        ops = struct.unpack_from("<%dI" % n_cig, data, pos + 36 + l_name)
        span = max(1, 0 if flag & 4 or not n_cig else sum(c >> 4 for c in ops if c & 15 in REF_OPS))
        recs.append({"at": pos, "ref": ref, "pos": p, "end": p + span, "flag": flag,
                     "bin": bam_check.reg2bin(p, p + span) if ref >= 0 and p >= 0 else None})
        pos += 4 + bs
    starts = {r["at"]: i for i, r in enumerate(recs)}
    keys = [(r["ref"] & 0xFFFFFFFF, (r["pos"] + 1) & 0xFFFFFFFF) for r in recs]
    _need(all(a <= b for a, b in zip(keys, keys[1:])), "the records are not sorted")

    refs, n_no_coor = _parse(bai)
    _need(len(refs) == len(names), "n_ref")
    _need(n_no_coor == sum(r["ref"] < 0 for r in recs), "n_no_coor")
    covered = [0] * len(recs)
    n_chunks = 0
    seek_cache = {}
    for ref, (bins, ioffset) in enumerate(refs):
        mine = [r for r in recs if r["ref"] == ref]
        if not mine:
            _need(not bins and not ioffset, "reference %d has no record but an index" % ref)
            continue
        numbers = [b for b, _ in bins]
        _need(numbers[-1] == PSEUDO_BIN and numbers[:-1] == sorted(set(numbers[:-1])) and all(b < PSEUDO_BIN for b in numbers[:-1]), "bin order")
        for b, chunks in bins[:-1]:
            _need(chunks, "a bin without chunks")
            last_end = 0
            for beg, end in chunks:
                n_chunks += 1
                a, z = absolute(beg), absolute(end)
                _need(last_end <= a < z, "chunks out of order or overlapping")
                last_end = z
                _need(a in starts and (z in starts or z == len(data)), "a chunk that does not begin and end on record boundaries")
                i = starts[a]
                while i < len(recs) and recs[i]["at"] < z:
                    _need(recs[i]["ref"] == ref and recs[i]["bin"] == b, "a chunk of bin %d holds a record of another bin" % b)
                    covered[i] += 1
                    i += 1
                # the seek: the member at coffset alone, inflated, holds the record's first bytes at uoffset
                c, uo = beg >> 16, beg & 0xFFFF
                if c not in seek_cache:
                    size = dict(ms)[c]
                    seek_cache[c] = inflate_ref.inflate(bam[c:c + size])[0]
                got = seek_cache[c][uo:uo + 36]
                _need(got == data[a:a + len(got)] and len(got) > 0, "seeking to a chunk start does not land on its record")
        (beg, end), (n_mapped, n_unmapped) = bins[-1][1]
        _need(len(bins[-1][1]) == 2, "pseudo-bin chunks")
        _need(absolute(beg) == mine[0]["at"], "pseudo-bin start")
        nxt = starts[mine[-1]["at"]] + 1
        _need(absolute(end) == (recs[nxt]["at"] if nxt < len(recs) else len(data)), "pseudo-bin end")
        _need(n_mapped == sum(not r["flag"] & 4 for r in mine) and n_unmapped == sum(bool(r["flag"] & 4) for r in mine), "pseudo-bin counts")
        placed = [r for r in mine if r["pos"] >= 0]
        _need(len(ioffset) == (1 + max((r["end"] - 1) >> 14 for r in placed) if placed else 0), "n_intv")
        expect = [None] * len(ioffset)
        for w in range(len(ioffset)):
            hits = [r["at"] for r in placed if r["pos"] >> 14 <= w <= (r["end"] - 1) >> 14]
            expect[w] = min(hits) if hits else None
        for w in range(len(ioffset) - 1, -1, -1):
            if expect[w] is None:
                expect[w] = expect[w + 1]
            _need(absolute(ioffset[w]) == expect[w], "ioffset[%d] of reference %d" % (w, ref))
    for i, r in enumerate(recs):
        _need(covered[i] == (1 if r["bin"] is not None else 0), "record %d lies in %d chunks" % (i, covered[i]))
    return {"n_records": len(recs), "n_chunks": n_chunks, "n_no_coor": n_no_coor}
