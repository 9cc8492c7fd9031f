"""The rules of include/kslam_samseq.h restated for the tests (no library involved): what a row must carry, from the FASTQ
record itself, and what its SEQ must say about the genome."""
import re

import samseq_check as S

COMP = bytes.maketrans(b"ACGTMKRYVBHDacgtmkryvbhd", b"TGCAKMYRBVDHtgcakmyrbvdh")   # W, S, N and everything else: unchanged
_MD = re.compile(rb"(\d+)|\^([A-Za-z]+)|([A-Za-z])")


def expected_columns(flag, bases, qual):
    """-> (SEQ, QUAL) a row with this FLAG carries for a read with these FASTQ lines (qual None: no qualities)"""
    if flag & 0x100 or not bases:
        return b"*", b"*"
    if flag & 0x10:
        return bases.translate(COMP)[::-1], (qual[::-1] if qual is not None else b"*")
    return bases, (qual if qual is not None else b"*")


def bam_view(seq, qual):
    """what the BAM record of a text row decodes to: upper case, anything that is no IUPAC letter N"""
    if seq == b"*":
        return seq, qual
    return bytes(c if c in S.NT16 else ord("N") for c in seq.upper()), qual


def check_rows(text, read_of, bases, quals, paired, through_bam=False, seen=None):
    """checks 2 and 3 on SAM text: every row against the read it names (read_of: name_reads' map; the batch is
    [R1 block | R2 block] when paired).  seen: a set that collects (read length, FLAG 0x10 set) of the rows that carry SEQ.
    -> (primary rows, secondary rows)"""
    half = len(bases) // 2 if paired else 0
    n_primary = n_secondary = 0
    for f in S.sam_rows(text):
        flag = int(f[1])
        read = read_of[f[0]] + (half if flag & 0x80 else 0)
        b, q = bases[read], (quals[read] if quals is not None else None)
        want = expected_columns(flag, b, q)
        if through_bam:
            want = bam_view(*want)
        assert (f[9], f[10]) == want, (f[0], flag)
        if flag & 0x100:
            n_secondary += 1
            assert (f[9], f[10]) == (b"*", b"*")
        else:
            n_primary += 1
            assert b == b"" or f[9] != b"*"
            if seen is not None and f[9] != b"*":
                seen.add((len(b), bool(flag & 0x10)))
    return n_primary, n_secondary


def name_reads(ids, paired):
    """QNAME -> read number of R1 (of the read, single end) for check_rows: ids must be unique per read pair"""
    n = len(ids) // 2 if paired else len(ids)
    read_of = {}
    for i in range(n):
        assert ids[i] not in read_of, "read ids must be unique for this check"
        read_of[ids[i]] = i
    return read_of


def check_against_genome(text, genomes, locus):
    """check 4: for each mapped row with a CIGAR, M + I + S == len(SEQ); walking SEQ along the entry's bases from POS, the
    mismatching M columns plus the I and D lengths equal NM (a column mismatches when the two bytes differ, N included:
    tests/rowdetails_ref.py), and MD names exactly those reference bases.  -> (rows checked, primary mapped rows skipped for
    want of a CIGAR, primary mapped rows)"""
    checked = skipped = primary_mapped = 0
    for f in S.sam_rows(text):
        flag = int(f[1])
        tags = dict((t[:2], t[5:]) for t in f[11:])
        mapped = b"AS" in tags          # the rows of a mapped mate carry the tags; FLAG 0x4 marks the other mate's rows
        if flag & 0x100 or not mapped:
            continue
        primary_mapped += 1
        if f[5] in (b"*", b""):
            skipped += 1
            continue
        seq, ops = f[9], S.parse_cigar(f[5])
        assert S.query_length(ops) == len(seq)
        ref = genomes[locus[f[2]]]
        rp, qp, nm, md, run = int(f[3]) - 1, 0, 0, [], 0
        for n, op in ops:
            if op == "S":
                qp += n
            elif op == "I":
                qp += n
                nm += n
            elif op == "D":
                md.append(b"%d" % run)
                run = 0
                md.append(b"^" + ref[rp:rp + n])
                nm += n
                rp += n
            else:
                for _ in range(n):
                    if ref[rp] == seq[qp]:
                        run += 1
                    else:
                        if md and md[-1].startswith(b"^") and run == 0:
                            md.append(b"0")
                        elif run or not md:
                            md.append(b"%d" % run)
                        elif not md[-1].startswith(b"^"):
                            md.append(b"0")
                        md.append(ref[rp:rp + 1])
                        nm += 1
                        run = 0
                    rp += 1
                    qp += 1
        md.append(b"%d" % run)
        assert nm == int(tags[b"NM"]), (f[0], flag, nm, tags[b"NM"])
        assert _md_events(b"".join(md)) == _md_events(tags[b"MD"]), (f[0], flag, b"".join(md), tags[b"MD"])
        checked += 1
    return checked, skipped, primary_mapped


def _md_events(md):
    """MD text -> [(reference offset, kind, bases)]: the reference bases it names and where, whatever zeros it writes between"""
    out, at = [], 0
    for num, dele, mis in _MD.findall(md):
        if num:
            at += int(num)
        elif dele:
            out.append((at, "D", dele))
            at += len(dele)
        else:
            out.append((at, "X", mis))
            at += 1
    return out, at
