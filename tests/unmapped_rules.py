"""The rules of include/kslam_samunmapped.h restated for the tests (no library involved): the rows a batch's reads without
alignment get, built from the FASTQ columns and the set of rowless records, as text and as BAM records; and the partition
property a SAM file written with the switch on must have."""
import struct

import samseq_check as S
import samseq_rules as R

NT16 = S.NT16


def flags_of(paired):
    """FLAG of a record's rows: R1 and R2 of a pair, or the one row of a single-end read"""
    return (77, 141) if paired else (4,)


def columns(bases, qual, seq):
    """-> (SEQ, QUAL) of a row (0x10 is never set: nothing is reversed); qual None: the batch has no qualities"""
    if not seq or not bases:
        return b"*", b"*"
    return bases, (qual if qual is not None else b"*")


def rowless_of(read_pairs, n_records):
    """the records (read pairs; single-end: reads) without a row: not among the final read pairs, or a group without alignment pairs"""
    with_rows = {int(g["r1_read"]) for g in read_pairs if int(g["count"]) > 0}
    return [p for p in range(n_records) if p not in with_rows]


def _reads_of(p, n_records, paired):
    return (p, p + n_records) if paired else (p,)


def expected_text(ids, bases, quals, rowless, n_records, paired, seq):
    """ids / bases / quals by read ([R1 block | R2 block] when paired; quals None: no qualities); rowless ascending"""
    out = []
    for p in rowless:
        for read, flag in zip(_reads_of(p, n_records, paired), flags_of(paired)):
            s, q = columns(bases[read], quals[read] if quals is not None else None, seq)
            out.append(b"\t".join([ids[read], b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", s, q]) + b"\n")
    return b"".join(out)


def nibble(c):
    """the index of c in "=ACMGRSVTWYHKDBN", either case; every other byte 15"""
    if c == ord("="):
        return 0
    k = NT16.find(bytes([c]).upper())
    return k if k > 0 else 15


def expected_records(ids, bases, quals, rowless, n_records, paired, seq):
    out = []
    for p in rowless:
        for read, flag in zip(_reads_of(p, n_records, paired), flags_of(paired)):
            b = bases[read] if seq else b""
            codes = [nibble(c) for c in b] + ([0] if len(b) & 1 else [])
            packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))
            qual = bytes(c - 33 for c in quals[read]) if quals is not None else b"\xff" * len(b)
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(ids[read]) + 1, 0, 4680, 0, flag, len(b), -1, -1, 0)
            body += ids[read] + b"\0" + packed + (qual if b else b"")
            out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


def is_new_row(f):
    """a row of the new kind: FLAG 4 / 77 / 141 on RNAME "*" (the writer's own 0x4 rows sit at their mate's coordinates)"""
    return f[2] == b"*" and int(f[1]) in (4, 77, 141)


def check_partition(off_text, on_text, ids, bases, quals, n_records, paired, seq, batches=None):
    """off_text / on_text: the rows (no header) of the same run without and with the switch (SEQ / QUAL on or off in both alike).
    ids by read, unique per record.
    batches: [(first record, records)] when the run cut its input (each batch's mapped rows, then its new rows); None: one batch.
    Checks, leaving no read out:
      - without the new rows, on_text is off_text;
      - over the rows without 0x100, every consumed read appears exactly once per mate;
      - the new rows are exactly the reads without a row in off_text, in input order, batch by batch;
      - with seq, un-reversing the 0x10 rows gives back every read's (id, bases, qualities).
    -> the number of new rows"""
    read_of = R.name_reads(ids, paired)
    on_rows = S.sam_rows(on_text)
    assert on_text_without_new(on_text) == off_text
    seen = {}
    for f in on_rows:
        flag = int(f[1])
        if flag & 0x100:
            continue
        read = read_of[f[0]] + (n_records if paired and flag & 0x80 else 0)
        assert read not in seen, ("a read with two primary rows", f[0], flag)
        seen[read] = f
    n_reads = 2 * n_records if paired else n_records
    assert sorted(seen) == list(range(n_reads)), "reads without a row: %r" % sorted(set(range(n_reads)) - set(seen))[:5]
    had_row = {read_of[f[0]] for f in S.sam_rows(off_text)}
    rowless = [p for p in range(n_records) if p not in had_row]
    # the order of the file: per batch the old rows, then the new ones in input order
    order = []
    for first, count in (batches or [(0, n_records)]):
        order += [p for p in rowless if first <= p < first + count]
    assert order == sorted(order)
    new = [f for f in on_rows if is_new_row(f)]
    want = S.sam_rows(expected_text(ids, bases, quals, order, n_records, paired, seq))
    assert new == want
    if batches:   # each batch's new rows stand behind that batch's mapped rows and before the next batch's
        at = 0
        for first, count in batches:
            inside = lambda f: first <= read_of[f[0]] < first + count   # noqa: E731
            run = []
            while at < len(on_rows) and inside(on_rows[at]):
                run.append(is_new_row(on_rows[at]))
                at += 1
            assert run == sorted(run), "a new row in front of a mapped row of its batch"
        assert at == len(on_rows)
    else:
        k = len(on_rows) - len(new)
        assert all(not is_new_row(f) for f in on_rows[:k]) and all(is_new_row(f) for f in on_rows[k:])
    if seq:
        for read, f in seen.items():
            flag = int(f[1])
            s, q = f[9], f[10]
            if flag & 0x10 and s != b"*":
                s, q = s.translate(R.COMP)[::-1], (q[::-1] if q != b"*" else q)
            assert (s, q) == columns(bases[read], quals[read] if quals is not None else None, True), (f[0], flag)
            assert f[0] == ids[read]
    return len(new)


def on_text_without_new(on_text):
    return b"".join(b"\t".join(f) + b"\n" for f in S.sam_rows(on_text) if not is_new_row(f))
