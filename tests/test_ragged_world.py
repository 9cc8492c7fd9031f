"""CPU proof of tests/ragged_world.py: through the oracle (oracle.align_to_database, oracle.tail_pairs) every batch kind is the
kind it claims -- its overlap records, its read pairs, the insert sizes that feed its limit, its r2 column -- and the FASTQ rules
the project pins take its texts, the empty bases lines included.  Where oracle/_ref/libslam_ref.so is built, the reference's OWN
loop (metagenomicAnalysis_Low_Mem, as in tests/test_reference_loop.py) runs every order and the single-end twin with the same batch
size and score threshold, and the oracle chain, batch by batch, must write its SAM, _PerRead and _abbreviated bytes.  The
reference's loop takes every kind -- the batches without an overlap record, the reads shorter than k and the empty bases lines
too -- so no kind is left to the oracle chain alone."""
import importlib
import os

import pytest

import ragged_world as W
import ref_loop_case as RL

NO_OVERLAP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def world(synth):
    return W.make(synth)


def test_the_orders_are_cut_into_their_kinds(world):
    for name, kinds in W.ORDERS.items():
        sizes = W.plan(world, kinds)
        assert sizes == [W.PAIRS_PER_BATCH] * 5 + [1], name           # every batch but the last is full: a batch is a kind
        assert [len(world["kinds"][k]) for k in kinds] == sizes
    assert W.ORDERS["empty_first"][0] == "nowhere" and W.ORDERS["empty_last"][-1] == "single_nowhere"
    ids = [p[0] for pairs in world["kinds"].values() for p in pairs]
    assert len(set(ids)) == len(ids)
    assert len(world["entries"]) == 4 and all(abs(len(e["bases"]) - W.GENOME_LEN) < 100 and e["genes"] and e["locusTag"] for e in world["entries"])


@pytest.mark.parametrize("kind", W.KINDS)
def test_the_fastq_rules_take_every_kind(kslam, oracle, world, kind):
    """kslam_fastq_parse_pair and the oracle's reader give back the builder's reads, an empty bases line as a read of no bases"""
    F = importlib.import_module("kslam_amd.fastq")
    for eol2 in (b"\n", b"\r\n"):
        case = W.case_of(world, [kind], eol2=eol2)
        batch, u1, u2 = F.parse_pair(case["r1"], case["r2"])
        assert (u1, u2) == (len(case["r1"]), len(case["r2"]))
        assert batch.bases == case["bases"] and batch.quality == case["quals"] and batch.ids == case["ids"] * 2
        n = case["n_pairs"]
        for text, lo in ((case["r1"], 0), (case["r2"], n)):      # the reference's reader, restated (oracle/fastq_oracle.cpp)
            bases, quality, ids, _ = oracle.fastq_read(text)
            assert bases == case["bases"][lo:lo + n] and quality == case["quals"][lo:lo + n] and ids == case["ids"]


@pytest.mark.parametrize("kind", W.KINDS)
def test_every_kind_is_what_it_claims(oracle, world, kind):
    b = W.chain_batch(oracle, world, kind)
    ov, rp, pr, st = b["ov"], b["rp"], b["pr"], b["st"]
    for got, want, what in zip((len(ov), len(rp), st["n_insert_sizes"]), W.CLAIMS[kind], ("overlap records", "read pairs", "insert sizes")):
        assert (got > 0) if want is None else (got == want), (kind, what, got)
    print(kind, "overlaps", len(ov), "past the threshold", st["n_overlaps_screened"], "read pairs", len(rp), "alignment pairs", len(pr),
          "insert sizes", st["n_insert_sizes"], "limit", st["max_insert_size"])
    lengths = sorted({len(x) for x in b["bases"]})
    if kind == "ordinary":
        assert len(rp) > W.PAIRS_PER_BATCH // 2 and st["n_insert_sizes"] > W.PAIRS_PER_BATCH // 2
        assert 0 < int(ov["revcomp"].sum()) < len(ov)                                  # both strands
        named = {int(i) for f in ("r1", "r2") for i in pr[f] if int(i) != NO_OVERLAP}
        assert any(int(ov[i]["cigar_len"]) > 1 for i in named)                         # indels: the pile-up reports have events
        assert any(int(c) & 15 == 1 for c in b["pool"]) and any(int(c) & 15 == 2 for c in b["pool"])
    if kind in ("nowhere", "single_nowhere", "screened"):
        assert b["sam"] == b"" and b["per_read"] == b"" and st["max_insert_size"] == NO_OVERLAP
    if kind == "one_mate":
        assert len(pr) > 0 and (pr["r2"] == NO_OVERLAP).all() and (pr["r1"] != NO_OVERLAP).all() and (pr["insert_size"] == 0).all()
        assert (ov["read"] < b["n"]).all() and st["max_insert_size"] == NO_OVERLAP     # no R2 has an overlap record; no sample, no limit
    if kind == "screened":
        assert len(ov) > W.PAIRS_PER_BATCH and st["n_overlaps_screened"] == 0 and int(ov["score"].max()) < W.SCORE_THRESHOLD
    if kind == "short":
        assert lengths[:4] == [0, 1, W.K - 1, W.K] and lengths[-1] == W.READ_LEN
        assert sorted(int(g["r1_read"]) for g in rp) == [20, 41]
        proper = pr[pr["insert_size"] != 0]
        assert len(proper) == 1 and st["max_insert_size"] == int(proper["insert_size"][0])   # one sample: the limit is that sample
        other = pr[int(rp[1]["first"]):int(rp[1]["first"]) + int(rp[1]["count"])]
        assert ((other["r1"] == NO_OVERLAP) | (other["r2"] == NO_OVERLAP)).all()              # the mates on different species never pair
        assert any(len(b["bases"][int(o["read"])]) == W.K for o in ov)                       # a read of exactly k bases has a record
        assert all(len(b["bases"][int(o["read"])]) >= W.K for o in ov)
    if kind == "single":
        assert b["n"] == 1 and len(pr) >= 1 and (pr["insert_size"] != 0).sum() == 1


def test_single_end_twin(oracle, world):
    """R1 alone: the kinds with an aligned R1 keep their read pairs, the empty kinds stay empty"""
    for kind in W.KINDS:
        b = W.chain_batch(oracle, world, kind, paired=False)
        empty = kind in ("nowhere", "single_nowhere", "screened")
        assert (len(b["rp"]) == 0) == empty and (len(b["ov"]) == 0) == (kind in ("nowhere", "single_nowhere")), kind
        assert (b["pr"]["r2"] == NO_OVERLAP).all()


def test_the_host_twins_write_the_restatements_files(kslam, oracle, world, tmp_path):
    """tests/ragged_expect.py's files -- what tests/test_gpu_ragged_stream.py expects of the device -- against the host twins and
    the product's writers on the same arrays: the restated tables and bytes hold for ragged batches on the CPU already"""
    import numpy as np
    import alignqc_ref
    import ragged_expect as E
    import variants_ref
    M = {k: importlib.import_module("kslam_amd." + k) for k in ("db", "taxonomy", "coverage", "genes", "kreport", "variants", "consensus", "readqc",
                                                              "alignqc", "depth", "readsplit", "taxreads")}
    kinds, P = W.ORDERS["plain"], E.PARAMS
    batches = [W.chain_batch(oracle, world, k) for k in kinds]
    ids = [t for b in batches for t in b["tax"]]
    chosen = [max(set(ids), key=ids.count)]
    exp, facts = E.files(oracle, world, kinds, eol2=b"\r\n", chosen=chosen, source=kslam.lib().kslam_version().split()[0])
    case = facts["case"]
    db = M["db"].Database.load(os.path.join(RL.write_case(case, tmp_path, M["db"]), "database"))
    tax = M["taxonomy"].TaxDB(world["taxdb"])
    parts = [E._part(world, b) for b in batches]
    whole = None
    for p in parts:
        whole = p if whole is None else variants_ref.concat(whole, p)
    got = {}
    rows, skipped = M["coverage"].tail_coverage([len(e["bases"]) for e in world["entries"]], whole["ov"], whole["rp"], whole["pr"])
    got["coverage"] = M["coverage"].report_bytes(db, rows)
    rows, st = M["genes"].tail_genes(db, whole["rp"], whole["pr"])
    got["genes"] = M["genes"].table_bytes(db, rows)
    assert skipped == 0 and st["n_in_gene"] > 0 and st["n_no_gene"] > 0
    rows, _ = M["kreport"].tail_kreport(tax, np.asarray(ids, dtype=np.uint32))
    got["kreport"] = M["kreport"].report_bytes(tax, rows, facts["n_pairs"])
    a = (whole["gbases"], whole["goff"], whole["ov"], whole["pool"], whole["rbases"], whole["roff"], whole["rp"], whole["pr"])
    rows, st = M["variants"].tail_variants(*a, P["variants_min_alt"], P["variants_min_depth"])
    got["vcf"] = M["variants"].report_bytes(db, rows, st)
    assert len(rows) > 100 and st["n_skipped"] == 0
    rows, seq, st = M["consensus"].tail_consensus(*a, *P["consensus_params"])
    got["fasta"] = M["consensus"].report_bytes(db, rows, seq)
    assert st["n_insertions"] > 0 and st["n_del_intervals"] > 0
    rows, _ = M["depth"].tail_depth(whole["goff"], whole["ov"], whole["pool"], whole["roff"], whole["rp"], whole["pr"], P["depth_min"])
    got["bedgraph"] = M["depth"].report_bytes(db, rows)
    got["read_qc"] = M["readqc"].report_bytes(M["readqc"].tail_read_qc(case["bases"], case["quals"], True, P["read_qc_max_cycles"]))
    total = alignqc_ref.empty(P["align_qc_max_cycles"], True)
    for p in parts:      # (the twin takes one batch: [R1 block | R2 block]); the file is the sum's
        t = M["alignqc"].tail_align_qc(p["gbases"], p["goff"], p["ov"], p["pool"], p["rbases"], p["roff"], p["rp"], p["pr"], p["rqual"], True,
                                       P["align_qc_max_cycles"])
        ref = alignqc_ref.batch_tables(p, P["align_qc_max_cycles"])
        assert M["alignqc"].report_bytes(t) == alignqc_ref.text(ref), p["name"]
        total = alignqc_ref.add_tables(total, ref)
    got["align_qc"] = M["alignqc"].report_bytes(total)
    for f in ("c1", "c2", "u1", "u2", "x1", "x2"):
        got[f] = b""
    for k, b in zip(kinds, batches):      # the splits batch by batch, as the loop writes them
        c = W.case_of(world, [k], eol2=b"\r\n")
        rp = b["rp"].astype(kslam.READ_PAIR_DT)
        for f, block in zip(("c1", "c2", "u1", "u2"), M["readsplit"].tail_split_reads(c["r1"], c["r2"], rp)["blocks"]):
            got[f] += block or b""
        selected = M["taxreads"].tail_taxon_reads(tax, chosen, E.TAXON_MODE, c["r1"], c["r2"], rp, np.asarray(b["tax"], dtype=np.uint32))
        for f, block in zip(("x1", "x2"), selected["blocks"]):
            got[f] += block or b""
    tax.close()
    db.close()
    for f, text in got.items():
        assert text == exp[f] and len(text) > 0, f


def _chain_files(oracle, world, kinds, paired=True):
    batches = [W.chain_batch(oracle, world, k, paired) for k in kinds]
    tree = oracle.taxonomy_tree(world["taxdb"])
    tax = [t for b in batches for t in b["tax"]]
    cl = W.COMMAND_LINE if paired else b"SLAM --db db R1.fq"
    out = {"sam": W.sam_header(oracle, world, cl) + b"".join(b["sam"] for b in batches), "per_read": b"".join(b["per_read"] for b in batches),
           "abbreviated": oracle.taxonomy_summary(tree, tax, sum(b["n"] for b in batches))}
    tree.close()
    return out


@pytest.mark.parametrize("order", sorted(W.ORDERS) + ["single_end"])
def test_oracle_chain_equals_the_real_reference_loop(kslam, oracle, world, tmp_path, order):
    if not oracle.have_ref_slam():
        pytest.skip("oracle/_ref/libslam_ref.so not built (the reference's sources are not here)")
    D = importlib.import_module("kslam_amd.db")
    paired = order != "single_end"
    kinds = W.ORDERS[order if paired else "plain"]
    case = W.case_of(world, kinds, paired)
    dbdir = RL.write_case(case, tmp_path, D)
    cl = W.COMMAND_LINE if paired else b"SLAM --db db R1.fq"
    ref = RL.run_reference(oracle, case, tmp_path, dbdir, W.PAIRS_PER_BATCH, score_threshold=W.SCORE_THRESHOLD, command_line=cl)
    orc = _chain_files(oracle, world, kinds, paired)
    assert ref["sam"].count(b"\n") > 100 and ref["per_read"].count(b"\n") > 60
    for k in ("sam", "per_read", "abbreviated"):
        assert orc[k] == ref[k], k
    # the chain cut batch by batch (ref_loop_case.run_oracle_chain) is the chain of the kinds: a batch IS a kind
    whole = RL.run_oracle_chain(oracle, case, W.PAIRS_PER_BATCH, score_threshold=W.SCORE_THRESHOLD, command_line=cl)
    assert all(whole[k] == orc[k] for k in ("sam", "per_read", "abbreviated"))
    if ref["log"] is not None:      # (the first reference run of the process finds its log: every batch went through the aligner)
        assert ref["log"].decode().count("Aligning reads to database using k = 32") == 6
