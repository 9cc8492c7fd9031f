"""The per-row walk (csrc/details.hip) and the device SAM text, BAM records and per-read lines (csrc/samtext.hip) alone, at every
hand-over inside them: the cases of tests/details_seams.py -- match runs of 999 / 1000 columns, MD texts of 48 / 49 bytes at
thread 0 / 255 / 256, mismatches in column 15 / 16 of a chunk, read 0 on the reverse strand, rows at the ends of the arrays,
odd characters and quality bytes, CIGARs that run past the read or the entry, POS / TLEN / NM / XT of up to 10 digits, groups
whose per-pair sort permutes, log-probabilities around the mapping-quality plan's bar of -300, every early-out of the LCA --
adopted as a context's result and compared with tests/rowdetails_ref.py bit for bit and with the host tail's text byte for
byte.  tests/test_details_seams.py proves on the CPU that every case sits where it claims and that the host tail equals the
oracle's restatement there."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import details_seams as S  # noqa: E402
import test_details_seams as H  # noqa: E402
from test_gpu_tail import _compacted  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = S.all_cases()
NONE = 0xFFFFFFFF


def _name(case):
    return case["name"]


@pytest.fixture(scope="module")
def mods(kslam):
    return [importlib.import_module("kslam_amd." + m) for m in ("tail", "taxonomy", "samtext", "bam")]


@pytest.fixture(scope="module")
def contexts(kslam):
    """one context per parameter set (score threshold, CIGARs reported or not)"""
    made = {}

    def get(case):
        key = (case["score_threshold"], case["report_cigar"])
        if key not in made:
            made[key] = kslam.Context(score_threshold=key[0], report_cigar=key[1])
        return made[key]
    yield get
    for c in made.values():
        c.close()


def adopt(c, case, index=True):
    """the case's rows and CIGAR pool become the context's last result (uploaded through torch, as a gathered result would be)"""
    import torch
    if index:
        c.set_index(case["entries"])
    c.load_reads(case["reads"])
    ov, pool = case["ov"], case["pool"]
    d_ov = torch.from_numpy(np.ascontiguousarray(ov).view(np.uint8).copy()).cuda() if len(ov) else torch.zeros(48, dtype=torch.uint8, device="cuda")
    d_cig = torch.from_numpy(pool.view(np.int32).copy()).cuda() if len(pool) else torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.adopt_results_device(d_ov.data_ptr(), len(ov), d_cig.data_ptr(), len(pool))
    c.load_qualities(case["quals"])


def md_of(det, md, i):
    return md[int(det["md_off"][i]):int(det["md_off"][i]) + int(det["md_len"][i])].tobytes()


def assert_details(case, det, md, edet, emd, walked):
    """walked: the rows the device was asked to walk.  Bit-exact on every one of them; all-zero records for the others.  A
    row without CIGAR has no MD text: its md_off names an empty slice, the restatement leaves it 0 and the device's scan puts
    it where the next text starts -- it is held to lie inside the pool, everything else about the row to be zero"""
    name = case["name"]
    has = case["ov"]["cigar_len"] != 0
    assert np.asarray(det[~walked]).tobytes() == bytes(32 * int((~walked).sum())), name
    for f in ("nm", "md_len", "flags"):
        assert (det[f] == edet[f]).all(), (name, f)
    assert (det["logp"].view(np.uint64) == edet["logp"].view(np.uint64)).all(), name
    assert (det["md_off"][has & walked] == edet["md_off"][has & walked]).all(), name
    assert (det["md_off"] <= len(md)).all() and (det["md_len"][~has] == 0).all(), name
    assert md.tobytes() == emd.tobytes(), name


# ---- W: the walk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["W"], ids=_name)
def test_row_details_equal_the_restatement_at_every_seam_of_the_walk(kslam, contexts, case):
    """k_row_details / k_md_gather on every row: the 16-column chunk loop and its run carry, the MD number paths below and from
    1000, the 48-byte slot and the second walk, the byte-wise load before the array, the ends of the arrays, raw-byte
    columns, quality bytes at the edges of the tables, rows without CIGAR in between, 1 / 255 / 256 / 257 rows"""
    c = contexts(case)
    adopt(c, case)
    n_md = c.row_details()
    det, md = c.take_row_details(len(case["ov"]))
    edet, emd = H.ref_details(kslam, case)
    assert n_md == len(emd)
    assert_details(case, det, md, edet, emd, np.ones(len(det), dtype=bool))
    for key, want in case["claim"].items():        # the seam itself, on the device's answer
        if key.startswith("md_len_of_row_"):
            assert int(det["md_len"][int(key[14:])]) == want
        elif key.startswith("md_of_row_"):
            assert md_of(det, md, int(key[10:])) == want
        elif key.startswith("flags_of_row_"):
            assert int(det["flags"][int(key[13:])]) == want


# ---- F: CIGARs that run past -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["F"], ids=_name)
def test_a_cigar_one_column_past_the_read_or_the_entry_is_flagged_and_refused(kslam, mods, contexts, case):
    T, X, ST, M = mods
    c = contexts(case)
    adopt(c, case)
    c.row_details()
    det, md = c.take_row_details(len(case["ov"]))
    bad = np.zeros(len(det), dtype=bool)
    bad[case["claim"]["bad_rows"]] = True
    assert ((det["flags"] & 2) != 0).tolist() == bad.tolist()
    edet, emd = H.ref_details(kslam, case)          # (the bad rows left out)
    for i in np.nonzero(~bad)[0]:                   # the rows before and after are intact
        assert (int(det["nm"][i]), int(det["md_len"][i]), int(det["flags"][i])) == (int(edet["nm"][i]), int(edet["md_len"][i]), int(edet["flags"][i]))
        assert det["logp"][i:i + 1].view(np.uint64)[0] == edet["logp"][i:i + 1].view(np.uint64)[0]
        assert md_of(det, md, i) == md_of(edet, emd, i)
    c.pair_screen(paired=case["paired"], score_threshold=case["score_threshold"], score_fraction=0.0, stages=2)
    c.row_details(of_pairs=True)
    R, I = H.tail_inputs(T, case)
    ST.set_annotations(c, I, None)
    ST.load_read_ids(c, case["ids"])
    with pytest.raises(kslam.KslamError, match="cigar runs past the end of the read or the entry"):
        ST.sam_text(c, paired=case["paired"], num_alignments=case["num_alignments"], sam_xa=case["sam_xa"])


# ---- L: the row list -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["L"], ids=_name)
def test_row_details_of_pairs_walks_the_referenced_rows_and_zeroes_the_others(kslam, mods, contexts, case):
    T = mods[0]
    c = contexts(case)
    adopt(c, case)
    c.pair_screen(paired=case["paired"], score_threshold=case["score_threshold"], score_fraction=0.0, stages=2)
    n_md = c.row_details(of_pairs=True)
    det, md = c.take_row_details(len(case["ov"]))
    rp, pr = H.host_pairs(T, case)
    listed = np.zeros(len(det), dtype=bool)
    for f in ("r1", "r2"):
        listed[pr[f][pr[f] != NONE]] = True
    assert {"none": 0, "all": len(det)}.get(case["claim"]["listed"], int(listed.sum())) == int(listed.sum())
    only = dict(case, ov=case["ov"].copy())
    only["ov"]["cigar_len"][~listed] = 0
    edet, emd = H.ref_details(kslam, only)
    assert n_md == len(emd)
    assert_details(case, det, md, edet, emd, listed)


# ---- W, T, X: the text -----------------------------------------------------------------------------------------------------
def device_text(c, mods, case, bam=False):
    T, X, ST, M = mods
    adopt(c, case)
    st = c.pair_screen(paired=case["paired"], score_threshold=case["score_threshold"], score_fraction=case["score_fraction"],
                       stages=case["stages"])
    assert st["stages_done"] & 4 == case["stages"] & 4, case["name"]
    c.row_details(of_pairs=True)          # (also when the CIGAR column is not reported: NM and the qualities come from the walk)
    R, I = H.tail_inputs(T, case)
    tax = X.TaxDB(case["taxdb"])
    try:
        ST.set_annotations(c, I, tax)
        ST.load_read_ids(c, case["ids"])
        if bam:
            return M.sam_bam(c, paired=case["paired"], num_alignments=case["num_alignments"], sam_xa=case["sam_xa"])
        sam, per, tids = ST.sam_text(c, paired=case["paired"], num_alignments=case["num_alignments"], sam_xa=case["sam_xa"], want_sam=True,
                                     want_per_read=True)
        rp, pr = c.take_pairs()
        return sam, per, tids, rp, pr
    finally:
        tax.close()


TEXT_CASES = CASES["W"] + CASES["T"] + CASES["X"]


@pytest.mark.parametrize("case", TEXT_CASES, ids=_name)
def test_device_text_per_read_lines_and_sorted_pairs_equal_the_host_tail(kslam, mods, contexts, case):
    """k_sam_plan / k_sam_collect / k_sam_lengths / k_sam_write / k_lca / k_per_read_write on the crafted rows: numbers of 1 ..
    10 digits through the two-register digit buffer, lines at every phase of the 8-byte sink, read pairs without records, 1 /
    255 / 256 / 257 read pairs, groups of 16 / 17 / 200 tied records, --num-alignments 0 .. 500, --sam-xa, single-end data,
    lone rows around -300, gene ties and empty columns, every branch of the LCA"""
    T, X, ST, M = mods
    c = contexts(case)
    if case["refusal"]:
        with pytest.raises(kslam.KslamError, match=case["refusal"].replace("+", r"\+")):
            device_text(c, mods, case)
        return
    exp, hrp, hpr = H.host_text(T, case)
    exp_tax, exp_per = H.host_classify(T, X, case, hrp, hpr)
    sam, per, tids, rp, pr = device_text(c, mods, case)
    assert sam == exp, case["name"]
    assert per == exp_per and tids.tolist() == exp_tax.tolist(), case["name"]
    if case["stages"] & 4:                # (the device's second screen leaves the survivors where they are, the host packs them)
        rp, pr = _compacted(rp, pr)
    assert rp.tobytes() == hrp.tobytes() and pr.tobytes() == hpr.tobytes(), case["name"]
    for key in ("groups", "groups_with_count_0"):
        if key in case["claim"]:          # the seam itself, on the device's groups
            assert {"groups": len(rp), "groups_with_count_0": int((rp["count"] == 0).sum())}[key] == case["claim"][key]


@pytest.mark.parametrize("case", CASES["T"] + CASES["X"], ids=_name)
def test_device_bam_records_equal_the_host_records(kslam, mods, contexts, case):
    """put_record on the same rows: tag_int's C / S / I widths at 255 / 256 and 65535 / 65536 for AS, XS, NM, X0 and XT"""
    T, X, ST, M = mods
    c = contexts(case)
    if case["refusal"]:
        with pytest.raises(kslam.KslamError, match=case["refusal"].replace("+", r"\+")):
            device_text(c, mods, case, bam=True)
        return
    if max(len(x) for x in case["ids"]) > 254:      # an id a record cannot hold: refused; the same rows with it cut to 254 bytes
        with pytest.raises(kslam.KslamError, match="longer than 254 bytes"):
            device_text(c, mods, case, bam=True)
        case = dict(case, ids=[x[:254] for x in case["ids"]])
        assert sorted({len(x) for x in case["ids"]}) == list(range(1, 18)) + [254]
    R, I = H.tail_inputs(T, case)
    rp, pr = H.host_pairs(T, case)
    det, md = H.ref_details(kslam, case)
    exp, _ = M.tail_finish_rows_bam(H.tail_params(T, case), R, I, case["ov"], case["pool"], det, md, rp, pr)
    assert device_text(c, mods, case, bam=True) == exp, case["name"]


# ---- the guard -------------------------------------------------------------------------------------------------------------
def test_row_details_without_an_index_is_refused_when_the_result_holds_cigars(kslam):
    """kslam_adopt_results_device on a context that never had kslam_set_index: the walk would read entry bases that are not
    there.  Refused before any kernel; rows without CIGAR need no index; with the index the answers are the W answers"""
    W = {c["name"]: c for c in CASES["W"]}
    case, plain = W["W-indels-clips-and-zero-length-runs"], W["W-257-rows"]
    bare = dict(plain, ov=plain["ov"].copy(), pool=np.zeros(0, dtype=np.uint32))
    bare["ov"]["cigar_len"] = 0
    bare["ov"]["cigar_off"] = 0
    c = kslam.Context()
    try:
        adopt(c, bare, index=False)
        assert c.row_details() == 0
        det, md = c.take_row_details(len(bare["ov"]))
        assert len(md) == 0 and not det["md_len"].any() and not det["nm"].any() and not det["flags"].any() and not det["logp"].any()
        adopt(c, case, index=False)
        for of_pairs in (False, True):
            if of_pairs:
                c.pair_screen(paired=True, score_fraction=0.0, stages=2)
            with pytest.raises(kslam.KslamError, match="kslam_set_index") as e:
                c.row_details(of_pairs=of_pairs)
            assert kslam.STATUS[e.value.status] == "ERR_STATE"
        with pytest.raises(kslam.KslamError):
            c.take_row_details(len(case["ov"]))           # nothing was computed
        adopt(c, case, index=True)
        c.row_details()
        det, md = c.take_row_details(len(case["ov"]))
        edet, emd = H.ref_details(kslam, case)
        assert_details(case, det, md, edet, emd, np.ones(len(det), dtype=bool))
    finally:
        c.close()
