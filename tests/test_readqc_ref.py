"""tests/readqc_ref.py, the plain-Python restatement of include/kslam_readqc.h, pinned on cases computed by hand and written out
here; the header's example file, byte for byte; and the library exports what the header declares.  No GPU."""
import json
import os

import readqc_ref as R


def _nonzero(v):
    return {i: x for i, x in enumerate(v) if x}


def test_one_read_of_every_base_kind_and_quality_kind():
    bases = b"ACGTNa*"
    quality = b"!5?~\x20\x7fI"
    t = R.tables([bases], [quality])
    assert t["max_cycles"] == 512 and t["paired"] is False
    s, other = t["streams"]
    assert other == R.empty_stream(512)
    assert (s["n_reads"], s["n_bases"], s["min_len"], s["max_len"]) == (1, 7, 7, 7)
    assert _nonzero(s["len_hist"]) == {7: 1} and len(s["len_hist"]) == 514
    # row * 6 + column: A C G T N, then a in column 0 again, then * in "other"
    assert _nonzero(s["base"]) == {0 * 6 + 0: 1, 1 * 6 + 1: 1, 2 * 6 + 2: 1, 3 * 6 + 3: 1, 4 * 6 + 4: 1, 5 * 6 + 0: 1, 6 * 6 + 5: 1}
    # '!' = 0, '5' = 20, '?' = 30, '~' = 93, 0x20 and 0x7F in column 94, 'I' = 40
    assert _nonzero(s["qual"]) == {0 * 95 + 0: 1, 1 * 95 + 20: 1, 2 * 95 + 30: 1, 3 * 95 + 93: 1, 4 * 95 + 94: 1, 5 * 95 + 94: 1, 6 * 95 + 40: 1}
    assert _nonzero(s["mean_q"]) == {36: 1}   # (0 + 20 + 30 + 93 + 40) // 5 = 183 // 5
    assert _nonzero(s["gc"]) == {40: 1}       # G and C of A C G T a: 2 of 5 = 40 %


def test_gc_rounds_half_up_and_leaves_n_out():
    for bases, want in ((b"GAAAAAAA", 13), (b"GCGAAAAA", 38), (b"GNNAAAAAAA", 13), (b"gc", 100), (b"AT", 0), (b"GAA", 33), (b"GGA", 67)):
        s = R.tables([bases], [b"I" * len(bases)])["streams"][0]
        assert _nonzero(s["gc"]) == {want: 1}, bases   # 12.5 -> 13, 37.5 -> 38, 33.3 -> 33, 66.7 -> 67
    assert _nonzero(R.tables([b"NNN**"], [b"IIIII"])["streams"][0]["gc"]) == {}   # no A, C, G or T: no count


def test_mean_quality_is_floored_over_the_valid_bytes():
    for quality, want in ((b"!\"", {0: 1}), (b"II5", {33: 1}), (b"I\x20", {40: 1}), (b"~~", {93: 1}), (b"\x00\xff", {})):
        s = R.tables([b"A" * len(quality)], [quality])["streams"][0]
        assert _nonzero(s["mean_q"]) == want, quality
    s = R.tables([b"AA"], [b"\x00\xff"])["streams"][0]
    assert _nonzero(s["qual"]) == {94: 1, 95 + 94: 1}


def test_a_read_of_length_zero_and_the_minimum():
    s = R.tables([b""], [b""])["streams"][0]
    assert (s["n_reads"], s["n_bases"], s["min_len"], s["max_len"]) == (1, 0, 0, 0)
    assert _nonzero(s["len_hist"]) == {0: 1} and not any(s["base"]) and not any(s["qual"]) and not any(s["mean_q"]) and not any(s["gc"])
    s = R.tables([b"ACG", b"", b"ACGTA"], [b"III", b"", b"IIIII"])["streams"][0]
    assert (s["n_reads"], s["n_bases"], s["min_len"], s["max_len"]) == (3, 8, 0, 5)
    s = R.tables([b"ACG", b"AC"], [b"III", b"II"])["streams"][0]
    assert (s["min_len"], s["max_len"]) == (2, 3)
    assert R.tables([], [])["streams"][0] == R.empty_stream(512)


def test_the_pooled_row_and_the_streams():
    t = R.tables([b"ACGT", b"TT"], [b"II5!", b"##"], paired=True, cycles=2)
    s0, s1 = t["streams"]
    assert len(s0["len_hist"]) == 4 and len(s0["base"]) == 18 and len(s0["qual"]) == 3 * 95
    assert _nonzero(s0["len_hist"]) == {3: 1}            # 4 bases > C = 2: the entry C + 1
    assert _nonzero(s0["base"]) == {0: 1, 6 + 1: 1, 12 + 2: 1, 12 + 3: 1}   # G and T pooled in row 2
    assert _nonzero(s0["qual"]) == {40: 1, 95 + 40: 1, 190 + 20: 1, 190 + 0: 1}
    assert _nonzero(s1["len_hist"]) == {2: 1} and _nonzero(s1["base"]) == {3: 1, 6 + 3: 1} and _nonzero(s1["qual"]) == {2: 1, 95 + 2: 1}


HEADER_EXAMPLE = b"""{
  "kslam_read_qc": 1,
  "paired": true,
  "max_cycles": 4,
  "summary": {
    "total_reads": 2,
    "total_bases": 8,
    "q20_bases": 7,
    "q30_bases": 6,
    "q20_rate": "0.875000",
    "q30_rate": "0.750000",
    "gc_content": "0.714286",
    "n_bases": 1,
    "other_bases": 0,
    "invalid_quality_bytes": 0
  },
  "read1": {
    "total_reads": 1,
    "total_bases": 5,
    "min_length": 5,
    "max_length": 5,
    "mean_length": "5.000000",
    "q20_bases": 4,
    "q30_bases": 4,
    "gc_content": "0.500000",
    "n_bases": 1,
    "other_bases": 0,
    "invalid_quality_bytes": 0,
    "length_counts": {">4": 1},
    "content": {
      "A": [1],
      "C": [0, 1],
      "G": [0, 0, 1],
      "T": [0, 0, 0, 1],
      "N": [],
      "other": [],
      "tail": [0, 0, 0, 0, 1, 0]
    },
    "quality_mean": ["40.000000", "40.000000", "40.000000", "40.000000"],
    "quality_tail_mean": "2.000000",
    "quality_counts": {"2": [0, 0, 0, 0, 1], "40": [1, 1, 1, 1]},
    "mean_quality_counts": {"32": 1},
    "gc_counts": {"50": 1}
  },
  "read2": {
    "total_reads": 1,
    "total_bases": 3,
    "min_length": 3,
    "max_length": 3,
    "mean_length": "3.000000",
    "q20_bases": 3,
    "q30_bases": 2,
    "gc_content": "1.000000",
    "n_bases": 0,
    "other_bases": 0,
    "invalid_quality_bytes": 0,
    "length_counts": {"3": 1},
    "content": {
      "A": [],
      "C": [0, 0, 1],
      "G": [1, 1],
      "T": [],
      "N": [],
      "other": [],
      "tail": [0, 0, 0, 0, 0, 0]
    },
    "quality_mean": ["20.000000", "30.000000", "93.000000"],
    "quality_tail_mean": "0.000000",
    "quality_counts": {"20": [1], "30": [0, 1], "93": [0, 0, 1]},
    "mean_quality_counts": {"47": 1},
    "gc_counts": {"100": 1}
  }
}
"""


def test_the_file_of_the_headers_example():
    """R1 = ACGTN / IIII#, R2 = GGC / 5?~, C = 4: every number below was worked out by hand from the header's definitions"""
    t = R.tables([b"ACGTN", b"GGC"], [b"IIII#", b"5?~"], paired=True, cycles=4)
    assert R.text(t) == HEADER_EXAMPLE
    doc = json.loads(HEADER_EXAMPLE)
    assert doc["summary"]["total_bases"] == 8 and list(doc) == ["kslam_read_qc", "paired", "max_cycles", "summary", "read1", "read2"]
    # single-end: no read2, an invalid byte under its own key, zero denominators
    t = R.tables([b"A"], [b"\x7f"], cycles=1)
    doc = json.loads(R.text(t))
    assert "read2" not in doc and doc["paired"] is False
    assert doc["read1"]["quality_counts"] == {"invalid": [1]} and doc["read1"]["quality_mean"] == ["0.000000"]
    assert doc["summary"]["invalid_quality_bytes"] == 1 and doc["summary"]["q20_rate"] == "0.000000"
    empty = json.loads(R.text(R.tables([], [])))
    assert empty["summary"]["gc_content"] == "0.000000" and empty["read1"]["mean_length"] == "0.000000" and empty["read1"]["length_counts"] == {}


def test_the_header_shows_the_example():
    """the example in include/kslam_readqc.h is the file above, up to where it abbreviates read2"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "kslam_readqc.h")).read()
    shown = "\n".join(line[5:] if line.startswith(" *   ") else line for line in h.split("\n"))
    upto = HEADER_EXAMPLE.decode().split('  "read2"')[0]
    assert upto in shown


def test_fastq_reads_takes_lf_crlf_and_a_missing_last_terminator():
    lf = b"@a\nACG\n+\nIII\n@b\n\n+\n\n@c\nAC\n+\n!!\n"
    want = ([b"ACG", b"", b"AC"], [b"III", b"", b"!!"])
    assert R.fastq_reads(lf) == want
    assert R.fastq_reads(lf.replace(b"\n", b"\r\n")) == want
    assert R.fastq_reads(lf[:-1]) == want
    assert R.of_fastq(lf, lf)["streams"][1] == R.of_fastq(lf)["streams"][0]
