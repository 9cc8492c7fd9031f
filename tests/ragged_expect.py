"""The expected bytes of every output of one kslam_stream_classify call over a sequence of tests/ragged_world.py's batch kinds.
Nothing here comes from the code under test:
  sam, per_read, tax_ids, abbreviated   the oracle chain, batch by batch (ragged_world.chain_batch); with SEQ / QUAL in the rows
                                        by tests/samseq_rules.py and every batch's rows for the reads without alignment behind
                                        its own rows by tests/unmapped_rules.py
  the ten opt-in outputs                each report's plain-Python restatement (tests/*_ref.py: the table AND the file's bytes) on
                                        the oracle's final arrays of every batch, concatenated as the reports' own stream tests
                                        concatenate them; tests/test_gpu_ragged_stream.py first holds the arrays the lanes hand
                                        back to these arrays
PARAMS are the non-default parameters of tests/test_gpu_stream_reports.py."""
import numpy as np

import alignqc_ref
import consensus_ref
import coverage_ref
import depth_ref
import genes_ref
import kreport_ref
import ragged_world as W
import readqc_ref
import readsplit_ref
import samseq_check
import samseq_rules
import taxreads_ref
import unmapped_rules
import variants_ref

PARAMS = dict(variants_min_alt=1, variants_min_depth=2, consensus_params=(2, 600, 1, 2), depth_min=2, read_qc_max_cycles=100, align_qc_max_cycles=120)
TAXON_MODE = taxreads_ref.CHILDREN
# an output and the files it writes (the names of tests/test_gpu_stream_reports.py)
OUTPUTS = {"coverage": ["coverage"], "genes": ["genes"], "kreport": ["kreport"], "variants": ["vcf"], "consensus": ["fasta"],
           "read_qc": ["read_qc"], "align_qc": ["align_qc"], "depth": ["bedgraph"], "reads_out": ["c1", "c2", "u1", "u2"],
           "taxon_reads": ["x1", "x2"]}
# a batch adds to these and an empty batch adds nothing: leaving an empty batch's reads out of the FASTQ text leaves the file as
# it is.  Not among them: read_qc (it counts every read that comes in, aligned or not), u1 / u2 (they hold the reads without a
# read pair), and the Kraken-style report (its "unclassified" row and every percentage count the pairs read).  No report file is
# fed by a batch's insert-size limit other than through the batch's own final arrays, so none depends on its neighbours.
ADDITIVE = ["coverage", "genes", "vcf", "fasta", "align_qc", "bedgraph", "c1", "c2", "x1", "x2"]


def sam_rows_with_seq(b):
    """a batch's oracle SAM rows with the SEQ and QUAL columns include/kslam_samseq.h puts there"""
    read_of = samseq_rules.name_reads(b["ids"], b["paired"])
    out = []
    for f in samseq_check.sam_rows(b["sam"]):
        flag = int(f[1])
        read = read_of[f[0]] + (b["n"] if flag & 0x80 else 0)
        f[9], f[10] = samseq_rules.expected_columns(flag, b["bases"][read], b["quals"][read])
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def sam_of_batch(b, seq=True, unmapped=True):
    rows = sam_rows_with_seq(b) if seq else b["sam"]
    if unmapped:
        rows += unmapped_rules.expected_text(b["ids"], b["bases"], b["quals"], unmapped_rules.rowless_of(b["rp"], b["n"]), b["n"], b["paired"], seq)
    return rows


def _part(world, b, arrays=None):
    """a batch as a case of tests/variants_ref.py, with the quality column and `paired` tests/alignqc_ref.py wants; arrays: (ov,
    pool, rp, pr) to take in place of the oracle's"""
    if arrays is not None:
        b = dict(b, ov=arrays[0], pool=arrays[1], rp=arrays[2], pr=arrays[3])
    ents = [bytes(e["bases"]) for e in world["entries"]]
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    roff = np.concatenate([[0], np.cumsum([len(r) for r in b["bases"]])]).astype(np.uint64)
    return {"name": b["kind"], "gbases": np.frombuffer(b"".join(ents), dtype=np.uint8), "goff": goff,
            "rbases": np.frombuffer(b"".join(b["bases"]), dtype=np.uint8), "roff": roff, "pool": b["pool"].astype(np.uint32),
            "ov": b["ov"].astype(variants_ref.OVERLAP_DT), "rp": b["rp"].astype(variants_ref.READ_PAIR_DT),
            "pr": b["pr"].astype(variants_ref.PAIRED_OVERLAP_DT), "rqual": np.frombuffer(b"".join(b["quals"]), dtype=np.uint8),
            "paired": b["paired"]}


def gene_columns(world):
    """-> (first, starts, stops, names, protein ids, products): the genes of every entry, flat, in the entries' order"""
    genes = [g for e in world["entries"] for g in e["genes"]]
    first = np.concatenate([[0], np.cumsum([len(e["genes"]) for e in world["entries"]])]).astype(np.uint64)
    return (first, np.array([g["start"] for g in genes], dtype=np.int32), np.array([g["stop"] for g in genes], dtype=np.int32),
            [g["geneName"] for g in genes], [g["proteinID"] for g in genes], [g["product"] for g in genes])


def files(oracle, world, kinds, paired=True, without=(), eol2=b"\n", chosen=None, source=b"kslam", params=PARAMS, arrays=None):
    """-> ({file: bytes}, facts): every file of the call -- sam (header included; rows with SEQ / QUAL and the rows of the reads
    without alignment), per_read, abbreviated and the files of OUTPUTS; facts: tax_ids, limits (max_insert_size per batch), plan,
    batches (for the XML restatement), n_pairs.  arrays: one (ov, pool, rp, pr) per batch for the restatements to read in place of the
    oracle's (the files that do not come from them stay the oracle chain's)"""
    kinds = [k for k in kinds if k not in without]
    batches = [W.chain_batch(oracle, world, k, paired) for k in kinds]
    case = W.case_of(world, kinds, paired, eol2=eol2)
    n_total = case["n_pairs"]
    cl = W.COMMAND_LINE if paired else b"SLAM --db db R1.fq"
    ents = world["entries"]
    loci, taxids, lengths = [e["locusTag"] for e in ents], [e["taxonomyID"] for e in ents], [len(e["bases"]) for e in ents]
    tax = [t for b in batches for t in b["tax"]]
    out = {"sam": W.sam_header(oracle, world, cl) + b"".join(sam_of_batch(b) for b in batches), "per_read": b"".join(b["per_read"] for b in batches)}
    tree = oracle.taxonomy_tree(world["taxdb"])
    out["abbreviated"] = oracle.taxonomy_summary(tree, tax, n_total)
    tree.close()
    # ---- the final arrays of all batches as one (tests/variants_ref.py's concat: reads, overlap records, CIGAR pool, pairs)
    parts = [_part(world, b, arrays[k] if arrays is not None else None) for k, b in enumerate(batches)]
    whole = None
    for p in parts:
        whole = p if whole is None else variants_ref.concat(whole, p)
    rows, _, _ = coverage_ref.table(np.asarray(lengths, dtype=np.uint64), whole["ov"], whole["rp"], whole["pr"])
    out["coverage"] = coverage_ref.report(rows, lengths, loci, taxids)
    first, starts, stops, names, proteins, products = gene_columns(world)
    rows, _ = genes_ref.table({"first": first, "starts": starts, "stops": stops, "rp": whole["rp"], "pr": whole["pr"]})
    out["genes"] = genes_ref.text(rows, first, starts, stops, loci, taxids, names, proteins, products)
    out["kreport"] = kreport_ref.text(world["taxdb"], tax, n_total)
    rows, _ = variants_ref.table(whole, params["variants_min_alt"], params["variants_min_depth"])
    out["vcf"] = variants_ref.vcf_bytes(rows, loci, lengths, source)
    rows, seqs, _ = consensus_ref.consensus(whole, *params["consensus_params"])
    out["fasta"] = consensus_ref.fasta_bytes(rows, seqs, loci)
    rows, _ = depth_ref.table(whole, params["depth_min"])
    out["bedgraph"] = depth_ref.bedgraph_bytes(rows, loci)
    out["read_qc"] = readqc_ref.text(readqc_ref.of_fastq(case["r1"], case["r2"] if paired else None, params["read_qc_max_cycles"]))
    cycles = params["align_qc_max_cycles"] or 512
    t = alignqc_ref.empty(cycles, paired)
    for p in parts:
        t = alignqc_ref.add_tables(t, alignqc_ref.batch_tables(p, cycles))
    t["paired"] = paired
    out["align_qc"] = alignqc_ref.text(t)
    # ---- the two read splits, by record number over the whole text
    at, records = 0, []
    for b in batches:
        records += [at + int(g["r1_read"]) for g in b["rp"]]
        at += b["n"]
    blocks, _ = readsplit_ref.split(case["r1"], case["r2"] if paired else None, records)
    for name, block in zip(OUTPUTS["reads_out"], blocks):
        out[name] = block
    if chosen is not None:
        blocks, _ = taxreads_ref.select(world["taxdb"], chosen, TAXON_MODE, case["r1"], case["r2"] if paired else None, records, tax)
        for name, block in zip(OUTPUTS["taxon_reads"], blocks):
            out[name] = block
    facts = {"tax_ids": tax, "limits": [b["st"]["max_insert_size"] for b in batches], "plan": [b["n"] for b in batches], "n_pairs": n_total,
             "batches": [(b["ids"], b["rp"], b["pr"]) for b in batches], "case": case, "kinds": kinds}
    return out, facts
