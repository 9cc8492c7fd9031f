"""A plain-Python restatement of include/kslam_readqc.h: the tables of a set of reads and the bytes of the JSON file.  Written
from the header's words alone; it shares nothing with the product (no numpy, no ctypes)."""

DEFAULT_CYCLES = 512
A_TO_OTHER = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3, ord("N"): 4, ord("n"): 4}


def empty_stream(cycles):
    return {"n_reads": 0, "n_bases": 0, "min_len": 0, "max_len": 0, "len_hist": [0] * (cycles + 2), "base": [0] * ((cycles + 1) * 6),
            "qual": [0] * ((cycles + 1) * 95), "mean_q": [0] * 94, "gc": [0] * 101}


def count_read(s, cycles, bases, quality):
    assert len(bases) == len(quality)
    n = len(bases)
    if s["n_reads"] == 0 or n < s["min_len"]:
        s["min_len"] = n
    if n > s["max_len"]:
        s["max_len"] = n
    s["n_reads"] += 1
    s["n_bases"] += n
    s["len_hist"][n if n <= cycles else cycles + 1] += 1
    g = acgt = q_n = q_sum = 0
    for c in range(n):
        row = c if c < cycles else cycles
        k = A_TO_OTHER.get(bases[c], 5)
        s["base"][row * 6 + k] += 1
        if k in (1, 2):
            g += 1
        if k < 4:
            acgt += 1
        b = quality[c]
        if 33 <= b <= 126:
            s["qual"][row * 95 + b - 33] += 1
            q_n += 1
            q_sum += b - 33
        else:
            s["qual"][row * 95 + 94] += 1
    if q_n:
        s["mean_q"][q_sum // q_n] += 1
    if acgt:
        s["gc"][(200 * g + acgt) // (2 * acgt)] += 1


def tables(bases, quality, paired=False, cycles=0):
    """bases / quality: lists of bytes, [R1 | R2] when paired"""
    cycles = cycles or DEFAULT_CYCLES
    assert len(bases) == len(quality) and not (paired and len(bases) % 2)
    streams = [empty_stream(cycles), empty_stream(cycles)]
    half = len(bases) // 2 if paired else len(bases)
    for i in range(len(bases)):
        count_read(streams[0 if i < half else 1], cycles, bases[i], quality[i])
    return {"max_cycles": cycles, "paired": bool(paired), "streams": streams}


def _ratio(num, den):
    return '"%.6f"' % (float(num) / float(den) if den else 0.0)


def _array(v):
    return "[" + ", ".join(str(x) for x in v) + "]"


def _cut(v):
    """v up to its last non-zero entry"""
    n = len(v)
    while n and not v[n - 1]:
        n -= 1
    return v[:n]


def _sums(s, cycles):
    col = [sum(s["base"][r * 6 + k] for r in range(cycles + 1)) for k in range(6)]
    q20 = sum(s["qual"][r * 95 + q] for r in range(cycles + 1) for q in range(20, 94))
    q30 = sum(s["qual"][r * 95 + q] for r in range(cycles + 1) for q in range(30, 94))
    invalid = sum(s["qual"][r * 95 + 94] for r in range(cycles + 1))
    return col, q20, q30, invalid


def _row_mean(row):
    return _ratio(sum(q * row[q] for q in range(94)), sum(row[:94]))


def _stream_text(name, s, cycles):
    col, q20, q30, invalid = _sums(s, cycles)
    L = ['  "%s": {' % name]
    L.append('    "total_reads": %d,' % s["n_reads"])
    L.append('    "total_bases": %d,' % s["n_bases"])
    L.append('    "min_length": %d,' % s["min_len"])
    L.append('    "max_length": %d,' % s["max_len"])
    L.append('    "mean_length": %s,' % _ratio(s["n_bases"], s["n_reads"]))
    L.append('    "q20_bases": %d,' % q20)
    L.append('    "q30_bases": %d,' % q30)
    L.append('    "gc_content": %s,' % _ratio(col[1] + col[2], col[0] + col[1] + col[2] + col[3]))
    L.append('    "n_bases": %d,' % col[4])
    L.append('    "other_bases": %d,' % col[5])
    L.append('    "invalid_quality_bytes": %d,' % invalid)
    lens = ['"%s": %d' % (str(n) if n <= cycles else ">%d" % cycles, v) for n, v in enumerate(s["len_hist"]) if v]
    L.append('    "length_counts": {%s},' % ", ".join(lens))
    L.append('    "content": {')
    for k, key in enumerate(("A", "C", "G", "T", "N", "other")):
        L.append('      "%s": %s,' % (key, _array(_cut([s["base"][r * 6 + k] for r in range(cycles)]))))
    L.append('      "tail": %s' % _array(s["base"][cycles * 6:cycles * 6 + 6]))
    L.append('    },')
    rows = [s["qual"][r * 95:(r + 1) * 95] for r in range(cycles + 1)]
    used = len(_cut([1 if any(row) else 0 for row in rows[:cycles]]))
    L.append('    "quality_mean": [%s],' % ", ".join(_row_mean(row) for row in rows[:used]))
    L.append('    "quality_tail_mean": %s,' % _row_mean(rows[cycles]))
    qc = []
    for q in range(95):
        column = _cut([row[q] for row in rows])
        if column:
            qc.append('"%s": %s' % (str(q) if q < 94 else "invalid", _array(column)))
    L.append('    "quality_counts": {%s},' % ", ".join(qc))
    L.append('    "mean_quality_counts": {%s},' % ", ".join('"%d": %d' % (i, v) for i, v in enumerate(s["mean_q"]) if v))
    L.append('    "gc_counts": {%s}' % ", ".join('"%d": %d' % (i, v) for i, v in enumerate(s["gc"]) if v))
    L.append('  }')
    return "\n".join(L)


def text(t):
    """the file's bytes for tables t"""
    cycles, s0, s1 = t["max_cycles"], t["streams"][0], t["streams"][1]
    a, b = _sums(s0, cycles), _sums(s1, cycles)
    col = [x + y for x, y in zip(a[0], b[0])]
    total = s0["n_bases"] + s1["n_bases"]
    L = ["{", '  "kslam_read_qc": 1,', '  "paired": %s,' % ("true" if t["paired"] else "false"), '  "max_cycles": %d,' % cycles, '  "summary": {']
    L.append('    "total_reads": %d,' % (s0["n_reads"] + s1["n_reads"]))
    L.append('    "total_bases": %d,' % total)
    L.append('    "q20_bases": %d,' % (a[1] + b[1]))
    L.append('    "q30_bases": %d,' % (a[2] + b[2]))
    L.append('    "q20_rate": %s,' % _ratio(a[1] + b[1], total))
    L.append('    "q30_rate": %s,' % _ratio(a[2] + b[2], total))
    L.append('    "gc_content": %s,' % _ratio(col[1] + col[2], col[0] + col[1] + col[2] + col[3]))
    L.append('    "n_bases": %d,' % col[4])
    L.append('    "other_bases": %d,' % col[5])
    L.append('    "invalid_quality_bytes": %d' % (a[3] + b[3]))
    L.append('  },')
    body = "\n".join(L) + "\n" + _stream_text("read1", s0, cycles)
    if t["paired"]:
        body += ",\n" + _stream_text("read2", s1, cycles)
    return (body + "\n}\n").encode()


def fastq_reads(fastq):
    """the (bases, quality) lists of a four-line FASTQ text; LF or CRLF, the last line with or without its terminator"""
    lines = fastq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    lines = [x[:-1] if x.endswith(b"\r") else x for x in lines]
    assert len(lines) % 4 == 0
    return lines[1::4], lines[3::4]


def of_fastq(r1, r2=None, cycles=0):
    """the tables of whole FASTQ files (r2 None: single-end)"""
    b1, q1 = fastq_reads(r1)
    if r2 is None:
        return tables(b1, q1, False, cycles)
    b2, q2 = fastq_reads(r2)
    assert len(b1) == len(b2)
    return tables(b1 + b2, q1 + q2, True, cycles)


# ---- the case set the host twin and the device are held to (tests/test_readqc_host.py, tests/test_gpu_readqc.py) ----

def _rand(seed):
    """a small generator of its own: the same reads everywhere"""
    state = [seed * 2654435761 % (1 << 32) or 1]

    def nxt(n):
        x = state[0]
        x ^= (x << 13) & 0xFFFFFFFF
        x ^= x >> 17
        x ^= (x << 5) & 0xFFFFFFFF
        state[0] = x
        return x % n
    return nxt


def _reads(lengths, seed, alphabet=b"ACGTNacgtn*", quals=b"!#5?FI~"):
    r = _rand(seed)
    bases = [bytes(alphabet[r(len(alphabet))] for _ in range(n)) for n in lengths]
    quality = [bytes(quals[r(len(quals))] for _ in range(n)) for n in lengths]
    return bases, quality


def cases(reads_per_workgroup=256):
    """dicts {name, bases, quality, paired, cycles}"""
    out = []

    def case(name, lengths, cycles=0, paired=False, seed=1, **kw):
        b, q = _reads(lengths, seed, **kw)
        out.append({"name": name, "bases": b, "quality": q, "paired": paired, "cycles": cycles})

    case("empty", [])
    case("empty_paired", [], paired=True)
    case("only_empty_reads", [0] * 5)
    case("wave_seams", [1, 63, 64, 65, 127, 128, 129, 0, 64, 129, 1], seed=2)
    case("wave_seams_paired", [1, 63, 64, 65, 127, 128, 129, 0, 64, 129, 1, 200], seed=3, paired=True)
    case("around_c64", [63, 64, 65, 1000, 64, 63], cycles=64, seed=4)
    case("c1", [3, 4, 5, 6, 7, 8, 9], cycles=1, seed=5)
    case("c5", [3, 4, 5, 6, 7, 8, 9, 5], cycles=5, seed=6, paired=True)
    case("tile_seams_c300", [127, 128, 129, 255, 256, 257, 299, 300, 301, 700], cycles=300, seed=7)
    case("one_long_read_c64", [300000], cycles=64, seed=8)
    for n in sorted({1, 255, 256, 257, reads_per_workgroup - 1, reads_per_workgroup, reads_per_workgroup + 1}):
        r = _rand(100 + n)
        case("reads_%d" % n, [20 + r(90) for _ in range(n)], seed=200 + n)
    every = bytes(range(256))
    out.append({"name": "all_byte_values", "bases": [every, every[::-1], b"ACGT"], "quality": [every[::-1], every, b"IIII"], "paired": False, "cycles": 0})
    out.append({"name": "all_byte_values_c100", "bases": [every, every], "quality": [every, every], "paired": True, "cycles": 100})
    out.append({"name": "many_identical", "bases": [b"GAT"] * 140000, "quality": [b"FFF"] * 140000, "paired": False, "cycles": 0})
    out.append({"name": "one_pair", "bases": [b"ACGTN", b"GGC"], "quality": [b"IIII#", b"5?~"], "paired": True, "cycles": 4})
    case("single_end", [100, 101, 99, 150, 151], seed=9)
    return out
