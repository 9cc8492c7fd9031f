"""The banded CIGAR stage (k-slam_amd/csrc/cigar.hip, banded_core.h) candidate by candidate, at every seam.

Each case of tests/cigar_seams.py -- a few hundred reads from closed-form families, both strands -- runs on one context
under four tunings (reload_tuning between them):
  default                                   registers up to band 4, systolic from band 5, rows in LDS beyond 255 slots;
  KSLAM_CIGAR_SYS=0 KSLAM_CIGAR_REG=0       the literal row arrays in LDS for everything;
  KSLAM_CIGAR_SYS=255                       systolic from band 1;
  KSLAM_CIGAR_SYS=0                         registers up to band 15 (k_banded_lds<8> and <16>), rows in LDS beyond.
For every run: rows and CIGARs equal the oracle's; the counts KSLAM_DEBUG=1 prints -- the bins as the SW stage asked for
them, the candidates handed to the one-lane kernel, every class of the generic loop, the big rerun, and with
KSLAM_SWEEP_ROOM=0 what doubling sent to every bin -- equal the restatement tests/cigar_plan_ref.py; no traceback error
(align_batch raises on one).  A mismatch names the family member, its (refLen, readLen, bw0, final band, ops) and the
kernel every attempt ran on.  tests/test_cigar_plan_ref.py checks on the CPU that the families reach the seams, and the
restatement against tests/golden/cigar_seams_counts.json: after a change to the families, run this module with
KSLAM_RECORD_CIGAR_COUNTS=tests/golden/cigar_seams_counts.json to record the printed counts afresh.
"""
import json
import os

import numpy as np
import pytest

import cigar_plan_ref as P
import cigar_seams as S
from align_compare import compare_alignments

pytestmark = pytest.mark.gpu

FIELDS = ("read", "entry", "rel", "revcomp", "score", "ref_begin", "ref_end", "query_begin", "query_end", "cigar_len")


def _record(name, tn, counts):
    path = os.environ.get("KSLAM_RECORD_CIGAR_COUNTS")
    if not path:
        return
    z = json.load(open(path)) if os.path.exists(path) else {}
    z["%s/%s" % (name, tn)] = dict(counts, classes={str(k): v for k, v in counts["classes"].items()})
    json.dump(z, open(path, "w"), indent=0, sort_keys=True)


def _wrong_rows(c, plan, got, gcig):
    """the rows whose record or CIGAR differs from the oracle's, described"""
    if len(got) != len(c.rows):
        return ["%d rows, the oracle has %d" % (len(got), len(c.rows))]
    bad = np.zeros(len(got), bool)
    for f in FIELDS:
        bad |= got[f] != c.rows[f]
    for i in np.nonzero(~bad)[0]:
        n = int(got["cigar_len"][i])
        a = gcig[int(got["cigar_off"][i]):int(got["cigar_off"][i]) + n]
        b = c.cig[int(c.rows["cigar_off"][i]):int(c.rows["cigar_off"][i]) + n]
        bad[i] = not np.array_equal(a, b)
    return ["%s: %s" % (c.fam[c.cand[i].read], plan.describe(c.cand[i])) for i in np.nonzero(bad)[0]]


@pytest.mark.parametrize("name", list(S.CASES))
def test_cigar_seams(kslam, oracle, monkeypatch, capfd, name):
    c = S.case(name, oracle)
    sc = c.sc
    monkeypatch.setenv("KSLAM_DEBUG", "1")
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    room0 = c.env.get("KSLAM_SWEEP_ROOM") == "0"
    ctx = kslam.Context(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
    try:
        ctx.set_index(c.entries)
        for tn, env in P.TUNINGS.items():
            for k in ("KSLAM_CIGAR_SYS", "KSLAM_CIGAR_REG"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            ctx.reload_tuning()
            capfd.readouterr()
            got, gcig = ctx.align_batch(c.reads)          # raises on a traceback error
            err = capfd.readouterr().err
            plan = S.plan_of(c, tn)
            wrong = _wrong_rows(c, plan, got, gcig)
            assert not wrong, "%s under %s: %d rows differ from the oracle\n  %s" % (name, tn, len(wrong), "\n  ".join(wrong[:6]))
            compare_alignments(got, gcig, c.rows, c.cig)
            counts = P.parse_debug(err)
            _record(name, tn, counts)
            told = P.explain(plan, counts, room0)
            assert not told, "%s under %s:\n  %s" % (name, tn, "\n  ".join(told))
            if c.long_chunk:
                assert plan.handed == 0 and "handed to the one-lane kernel" not in err
    finally:
        ctx.close()
