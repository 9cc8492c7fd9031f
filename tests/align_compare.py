"""Row-by-row comparison of two alignment results (overlap rows + CIGAR pools), shared by the GPU test modules."""
import numpy as np


def compare_alignments(got, gcig, exp, ecig):
    assert len(got) == len(exp)
    for f in ("read", "entry", "rel", "revcomp", "score", "ref_begin", "ref_end", "query_begin",
              "query_end", "cigar_len"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, "%s differs at %s: got %s exp %s" % (f, bad[:5], got[bad[:5]], exp[bad[:5]])
    for i in range(len(got)):
        a = gcig[int(got["cigar_off"][i]):int(got["cigar_off"][i]) + int(got["cigar_len"][i])]
        b = ecig[int(exp["cigar_off"][i]):int(exp["cigar_off"][i]) + int(exp["cigar_len"][i])]
        assert (a == b).all(), "cigar %d" % i
