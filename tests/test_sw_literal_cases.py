"""The families of tests/sw_literal_cases.py reach what they are built for -- judged on the CPU, by the oracle's emulation of
the reference's striped passes, by the real ssw.c where oracle/_ref is built, and by the answers of the real ssw.c stored in
tests/golden/ssw_saturation_vectors.npz.  tests/test_gpu_sw_literal_seams.py runs the same batches through the library.

Two of the hand-over preconditions cannot hold for every scoring, by arithmetic rather than by construction:
  * a candidate exists because 32 bases of the read equal the entry, so it scores at least 32 x match: with match 40 and 127
    no candidate stays below 255 - bias, and the byte pass gives up on every one of them (asserted as such);
  * every score is a multiple of gcd(match, mismatch, gapO, min(gapO, gapE)) (where gapE > gapO a gap opens again at every
    base): under (2, 40, 30, 20) and (2, 8, 2, 3) all scores are even and the odd one of 254 - bias, 255 - bias cannot occur;
    the exact values asked for are those of the two that can (sw_literal_cases.handover_targets).
"""
import os

import numpy as np
import pytest

import cigar_plan_ref as P
import sw_literal_cases as C
from sw_plan_ref import codes, window

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssw_saturation_vectors.npz")
_rows = {}


def rows_of(oracle, name, plain=False, sc=None):
    """the oracle's rows and CIGAR pool for a case (striped emulation unless plain), computed once"""
    sc = sc or C.CASES[name][1]
    key = (name, plain, sc)
    if key not in _rows:
        B = C.build(name)
        p = oracle.Params.default(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
        al, cg, _ = oracle.align_to_database(B.reads, B.entries, p, plain=plain)
        _rows[key] = (al, cg)
    return _rows[key]


def pair_of(B, row):
    """(read codes, window codes) of a row's candidate, as ssw_align takes them"""
    r, e = int(row["read"]), int(row["entry"])
    return (codes(B.reads[r]).astype(np.int8),
            window(len(B.reads[r]), B.entries[e], int(row["rel"]), bool(row["revcomp"])).astype(np.int8))


def ssw_view(B, al, cg, k):
    """row k as ssw_align returned it: (score, ref_begin, ref_end, read_begin, read_end) relative to the window, CIGAR in
    its order"""
    row = al[k]
    L, E = len(B.reads[int(row["read"])]), len(B.entries[int(row["entry"])])
    rb, re_, qb, qe, _, _ = P.unflip(row, L, E)
    cig = cg[int(row["cigar_off"]):int(row["cigar_off"]) + int(row["cigar_len"])]
    if int(row["score"]) == 0:
        return (0, int(row["ref_begin"]), int(row["ref_end"]), int(row["query_begin"]), int(row["query_end"])), cig
    return (int(row["score"]), rb, re_, qb, qe), (cig[::-1] if row["revcomp"] else cig)


def same_rows(a, ca, b, cb):
    """per row: every field and every CIGAR word equal"""
    out = np.ones(len(a), dtype=bool)
    for f in ("score", "ref_begin", "ref_end", "query_begin", "query_end", "cigar_len"):
        out &= a[f] == b[f]
    for k in np.nonzero(out)[0]:
        x = ca[int(a["cigar_off"][k]):int(a["cigar_off"][k]) + int(a["cigar_len"][k])]
        y = cb[int(b["cigar_off"][k]):int(b["cigar_off"][k]) + int(b["cigar_len"][k])]
        out[k] = np.array_equal(x, y)
    return out


@pytest.mark.parametrize("sc", C.OUTSIDE, ids=C._tag)
def test_seam_families_straddle_the_hand_over(oracle, sc):
    """S1 to S5 of a scoring: candidates on both sides of the byte pass's `best + bias >= 255`, at the two values next to
    it, gapped ones, and ones with an N inside the aligned span."""
    name = C.names("S1-5", sc)[0]
    B = C.build(name)
    al, cg = rows_of(oracle, name)
    assert 250 <= len(al) <= 600
    per_read = np.bincount(al["read"], minlength=len(B.reads))
    assert per_read.max() <= 2
    assert [len(B.reads[r]) for r in np.nonzero(per_read == 0)[0]] == [0, 31]      # the two reads without a seed
    score = al["score"].astype(np.int64)
    edge = 255 - sc[1]
    if 32 * sc[0] < edge:
        assert (score < edge).sum() >= 20 and (score >= edge).sum() >= 20, ((score < edge).sum(), (score >= edge).sum())
        wanted = [t for t in (edge - 1, edge) if t in C.handover_targets(sc)]
        assert wanted
        for t in wanted:
            assert (score == t).sum() >= 3, (t, (score == t).sum())
    else:                                            # the seed alone overflows the byte pass
        assert (score >= edge).all() and len(score) >= 20 and C.handover_targets(sc) == []
    assert (al["cigar_len"] > 1).sum() >= 10
    with_n = 0
    for k in range(len(al)):
        rd, win = pair_of(B, al[k])
        (s, rb, re_, qb, qe), _ = ssw_view(B, al, cg, k)
        with_n += bool(s > 0 and ((rd[qb:qe + 1] > 3).any() or (win[rb:re_ + 1] > 3).any()))
    assert with_n >= 5, with_n


def _saturation_cases():
    return C.names("S6") + C.names("S9")


def test_saturation_families_saturate(oracle):
    """S6 and S9: candidates the word pass cuts at 32 767, candidates just below it, saturated ones with a gapped CIGAR,
    and -- inside the envelope -- candidates on which the plain two-pass recurrence answers something else."""
    cut = near = gapped = differ = 0
    for name in _saturation_cases():
        B, sc = C.build(name), C.CASES[name][1]
        al, cg = rows_of(oracle, name)
        L = np.array([len(B.reads[int(r)]) for r in al["read"]])
        sat = al["score"] == C.SAT
        cut += int((sat & (al["query_end"] - al["query_begin"] + 1 < L)).sum())
        near += int(((al["score"] >= 32000) & (al["score"] < C.SAT)).sum())
        gapped += int((sat & (al["cigar_len"] > 1)).sum())
        assert (int(al["score"].max()) < C.SAT) == (name in C.BELOW_SATURATION), (name, int(al["score"].max()))
        assert int(al["score"].max()) <= C.SAT
        if C.in_envelope(sc):
            pl, pc = rows_of(oracle, name, plain=True)
            differ += int((~same_rows(al, cg, pl, pc)).sum())
    assert cut >= 10 and near >= 5 and gapped >= 5 and differ >= 8, (cut, near, gapped, differ)


def test_banded_family_reaches_every_bin(oracle):
    """S10: every bin of initial bands, attempts that double, a span its band covers, a CIGAR beyond the small slot."""
    bins, doubled, covered, big = set(), 0, 0, 0
    for name in C.names("S10"):
        B, sc = C.build(name), C.CASES[name][1]
        al, cg = rows_of(oracle, name)
        for c in P.candidates(al, B.reads, B.entries, sc):
            if not c.want or c.inline:
                continue
            bins.add(P.cig_bin(c.bw0))
            doubled += c.band > c.bw0
            covered += any(c.ref_len <= 2 * w + 1 and P.sentinel_rows(c, w) for w in P.widths(c))
            big += P.overflows(c)
    assert bins == set(range(8)), bins
    assert doubled >= 5 and covered >= 2 and big >= 1, (doubled, covered, big)


def test_long_read_geometry_of_the_cases():
    """S7 and S8 sit on both sides of the kernels' 64 KiB LDS opt-in (the lengths come from sw_scores' own formulas), S9 on
    both sides of the routing's cut, and the mixed batches hold class runs of length one first, inside and last."""
    assert C.sw_striped_lds(C.lcap_of(C._S7_EDGE)) <= 65536 < C.sw_striped_lds(C.lcap_of(C._S7_EDGE + 1))
    assert C.sw_long_lds(C.lcap_of(C._S8_EDGE)) <= 65536 < C.sw_long_lds(C.lcap_of(C._S8_EDGE + 1))
    longest = sorted(max(len(r) for r in C.build(n).reads) for n in C.names("S7"))
    assert longest == [C._S7_EDGE - 16, C._S7_EDGE, C._S7_EDGE + 16, C._S7_EDGE + 32, 9000]
    sides = {C.saturates(C.CASES[n][1], max(len(r) for r in C.build(n).reads)) for n in C.names("S9")}
    assert sides == {False, True}
    assert not C.saturates((7, 3, 5, 2), 4681) and C.saturates((7, 3, 5, 2), 4682)
    for n in C.names("S8")[:2]:
        lens = [len(r) > 511 for r in C.build(n).reads]
        runs = [i for i in range(len(lens)) if lens[i] and (i == 0 or not lens[i - 1]) and (i + 1 == len(lens) or not lens[i + 1])]
        assert runs[0] == 0 and runs[-1] == len(lens) - 1 and len(runs) >= 3, runs


def test_against_real_ssw_when_present(oracle):
    """The emulation the GPU test compares with equals the real ssw.c on every S6 and S9 vector and on a sample of 20 of
    every other family: ends and CIGAR."""
    if not oracle.have_ref_ssw():
        pytest.skip("oracle/_ref/libssw_ref.so not built (no /root/reference)")
    rng = np.random.default_rng(5)
    checked = 0
    for name in C.CASES:
        B, sc = C.build(name), C.CASES[name][1]
        al, cg = rows_of(oracle, name)
        mat = oracle.build_matrix(sc[0], sc[1])
        fams = np.array([B.fam[int(r)].split()[0] for r in al["read"]])
        pick = []
        for f in sorted(set(fams)):
            idx = np.nonzero(fams == f)[0]
            pick += list(idx if f in ("S6", "S9") else rng.choice(idx, size=min(20, len(idx)), replace=False))
        for k in pick:
            rd, win = pair_of(B, al[k])
            if len(win) == 0:
                continue
            r0, c0 = oracle.ref_ssw_align(rd, win, mat, sc[2], sc[3])
            r1, c1 = ssw_view(B, al, cg, k)
            assert r0 == r1, (name, k, r0, r1)
            assert np.array_equal(c0, c1), (name, k)
            checked += 1
    assert checked >= 500, checked


def saturation_vectors(oracle, names_short, names_long):
    """(scoring, read codes, window codes) of the stored vectors: every candidate of the short cases, the first of the long"""
    out = []
    for name in names_short + names_long:
        B, sc = C.build(name), C.CASES[name][1]
        recs = np.concatenate([oracle.extract_kmers(B.reads, False, 1), oracle.extract_kmers(B.entries, True, 16)])
        cand, _ = oracle.find_overlaps(oracle.sort_kmers(recs), [len(r) for r in B.reads])
        for k in range(len(cand) if name in names_short else 1):
            rd, win = pair_of(B, cand[k])
            out.append((sc, rd, win))
    return out


STORED_SHORT = [n for n in _saturation_cases() if max(len(r) for r in C.build(n).reads) <= 1200]
STORED_LONG = ["S9 5_3_5_2 L9000 AB", "S9 8_3_5_2 L9000 C"]


def _split(flat, lens):
    out, p = [], 0
    for n in lens:
        out.append(flat[p:p + int(n)])
        p += int(n)
    return out


def test_emulation_equals_the_stored_answers_of_the_real_ssw(oracle):
    """tests/golden/ssw_saturation_vectors.npz (tests/golden/make_golden.py --saturation): the S6 and S9 vectors of up to
    1200 bases and two of 9000, with what the real ssw.c answered.  Holds where oracle/_ref is absent."""
    z = np.load(GOLD)
    reads, refs = _split(z["reads"], z["read_len"]), _split(z["refs"], z["ref_len"])
    cigs = _split(z["cigars"], z["cigar_len"])
    assert len(reads) >= 40 and (z["results"][:, 0] == C.SAT).sum() >= 20
    assert ((z["cigar_len"] > 1) & (z["results"][:, 0] == C.SAT)).sum() >= 3
    made = saturation_vectors(oracle, STORED_SHORT, STORED_LONG)      # the stored inputs are the builder's
    assert len(made) == len(reads)
    for i in range(len(reads)):
        sc = tuple(int(v) for v in z["params"][i])
        assert sc == made[i][0] and np.array_equal(reads[i], made[i][1]) and np.array_equal(refs[i], made[i][2]), i
        res, cig = oracle.ssw_align(reads[i], refs[i], oracle.build_matrix(sc[0], sc[1]), sc[2], sc[3])
        got = (res.score1, res.ref_begin1, res.ref_end1, res.read_begin1, res.read_end1)
        assert got == tuple(int(v) for v in z["results"][i]), (i, sc, got)
        assert np.array_equal(cig, cigs[i]), (i, sc)
