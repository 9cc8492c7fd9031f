"""A ragged world for the batch loop: a small index and one FASTQ pair (with its single-end twin) whose batches of
PAIRS_PER_BATCH pairs are NOT "a few hundred ordinary pairs" -- batches without overlaps, without surviving read pairs, without a
proper pair, with exactly one proper pair, of one pair.  Plain module, deterministic from seeds; tests/test_ragged_world.py
proves on the CPU, through the oracle, that every batch is the kind it claims, and tests/test_gpu_ragged_stream.py sends the
batches through the lanes and through kslam_stream_classify.

The kinds (KINDS), each a list of pairs (id, R1 bases, R2 bases, R1 quality, R2 quality):
  ordinary   pairs from the index on both strands, with substitutions and indels
  nowhere    every read from a genome that is not in the index: no overlap record, no read pair
  one_mate   R1 from the index, R2 from nowhere: every alignment pair has r2 == NO_OVERLAP, the insert-size statistics have no
             sample (src/PairedOverlap.h:314-324: the limit is UINT32_MAX)
  screened   chimeric reads, CHIMERA_HEAD index bases and random bases behind them: overlap records, every one below
             SCORE_THRESHOLD, so no read pair is left
  short      reads of SHORT_LENGTHS bases (k is 32; a bases line may be empty: tests/fastq_seams.py's filler records, and
             kslam_fastq_parse takes it) and two ordinary pairs, one proper and one with its mates on different species: exactly
             one insert size feeds the limit, which is that size (mean of one sample, standard deviation 0)
  single     one ordinary pair; single_nowhere: one pair from nowhere
ORDERS names three sequences of them; every batch but the last is full, so a batch is a kind."""
import numpy as np

import ref_loop_case as RL

PAIRS_PER_BATCH = 64
K = 32
READ_LEN = 110
SCORE_THRESHOLD = 100      # above 2 * CHIMERA_HEAD + what a random tail adds, below what an ordinary read scores
CHIMERA_HEAD = 40
SHORT_LENGTHS = (1, 31, 32, 0)
N_SPECIES, N_STRAINS, GENOME_LEN, N_GENES = 2, 2, 9000, 6
ORDERS = {
    "plain": ("ordinary", "nowhere", "one_mate", "screened", "short", "single"),
    "empty_first": ("nowhere", "ordinary", "one_mate", "screened", "short", "single"),
    "empty_last": ("ordinary", "nowhere", "one_mate", "screened", "short", "single_nowhere"),
}
KINDS = ("ordinary", "nowhere", "one_mate", "screened", "short", "single", "single_nowhere")
# what tests/test_ragged_world.py proves of each kind: (overlap records, read pairs, insert sizes that feed the limit); None: > 0
CLAIMS = {"ordinary": (None, None, None), "nowhere": (0, 0, 0), "one_mate": (None, None, 0), "screened": (None, 0, 0),
          "short": (None, 2, 1), "single": (None, 1, 1), "single_nowhere": (0, 0, 0)}
COMMAND_LINE = b"SLAM --db db R1.fq R2.fq"


def _entries(synth):
    genomes = synth.make_genomes(611, N_SPECIES, N_STRAINS, GENOME_LEN, strain_sub=0.02, strain_indel=0.001)
    entries = [{"bases": g, "taxonomyID": 1000 + i, "genbankID": 7000 + i, "locusTag": b"NC_%06d.1" % i, "isPlasmid": i == 3,
                "genes": [{"geneName": b"gene%d" % k, "proteinID": b"WP_%d.1" % (100 * i + k), "locusTag": b"LT%02d_%02d" % (i, k),
                           "referenceSequence": b"NC_%06d" % i, "product": b"hypothetical protein %d" % k,
                           "start": 400 + 1300 * k, "stop": 1500 + 1300 * k, "geneID": k, "complement": bool(k & 1)}
                          for k in range(N_GENES)]}
               for i, g in enumerate(synth.to_bytes(genomes))]
    return genomes, entries


def _pairs(synth, seed, genomes, n, sub_rate=0.02, indel_rate=0.004):
    reads, _ = synth.make_paired_reads(seed, genomes, n, read_len=READ_LEN, frag_mean=300, frag_sd=45, sub_rate=sub_rate,
                                       indel_rate=indel_rate, unmapped_frac=0.0)
    return reads[:n], reads[n:]


def _kind_reads(synth, genomes):
    """kind -> (R1 arrays, R2 arrays)"""
    rng = np.random.default_rng(613)
    elsewhere = synth.make_genomes(977, 1, 1, GENOME_LEN)
    n = PAIRS_PER_BATCH
    out = {"ordinary": _pairs(synth, 621, genomes, n), "nowhere": _pairs(synth, 622, elsewhere, n)}
    a, _ = _pairs(synth, 623, genomes, n)
    _, b = _pairs(synth, 624, elsewhere, n)
    out["one_mate"] = (a, b)
    # chimeric reads: the head is the index's (either strand), the tail nobody's
    a, b = _pairs(synth, 625, genomes, n, sub_rate=0.0, indel_rate=0.0)
    out["screened"] = tuple([np.concatenate([x[:CHIMERA_HEAD], synth.random_bases(rng, READ_LEN - CHIMERA_HEAD)]) for x in mate] for mate in (a, b))
    # short reads cut from ordinary ones, and two ordinary pairs in the middle of them
    a, b = _pairs(synth, 626, genomes, n, sub_rate=0.0, indel_rate=0.0)
    a = [x[:SHORT_LENGTHS[i % 4]] for i, x in enumerate(a)]
    b = [x[:SHORT_LENGTHS[(i + 1) % 4]] for i, x in enumerate(b)]
    p1, p2 = _pairs(synth, 627, genomes, 1)
    a[20], b[20] = p1[0], p2[0]                                    # the proper pair
    p1, _ = _pairs(synth, 628, genomes[:N_STRAINS], 1)             # R1 of the first species ...
    _, p2 = _pairs(synth, 629, genomes[N_STRAINS:], 1)             # ... R2 of the second: never on one entry
    a[41], b[41] = p1[0], p2[0]
    out["short"] = (a, b)
    out["single"] = _pairs(synth, 630, genomes, 1)
    out["single_nowhere"] = _pairs(synth, 631, elsewhere, 1)
    return out


def make(synth):
    """-> dict(entries, taxdb, kinds {kind: [(id, b1, b2, q1, q2)]}): the index in the layout kslam_amd.db.write takes"""
    genomes, entries = _entries(synth)
    rng = np.random.default_rng(617)
    kinds = {}
    for kind, (a, b) in _kind_reads(synth, genomes).items():
        a, b = synth.to_bytes(a), synth.to_bytes(b)
        kinds[kind] = [(b"%s%03d" % (kind.encode(), i), x, y, bytes(rng.integers(35, 74, len(x), dtype=np.uint8)),
                        bytes(rng.integers(35, 74, len(y), dtype=np.uint8))) for i, (x, y) in enumerate(zip(a, b))]
    assert sorted(kinds) == sorted(KINDS)
    return {"entries": entries, "taxdb": RL.taxdb_text(N_SPECIES, N_STRAINS), "kinds": kinds}


def case_of(world, kinds, paired=True, eol2=b"\n", without=()):
    """the `case` dict of ref_loop_case.make_case for a sequence of kinds (an order of ORDERS, or one kind alone), the pairs of the
    kinds in `without` left out; paired=False: the single-end twin, R1 alone"""
    pairs = [p for kind in kinds if kind not in without for p in world["kinds"][kind]]
    n = len(pairs)
    ids = [p[0] for p in pairs]
    bases, quals = [p[1] for p in pairs], [p[3] for p in pairs]
    r1 = RL.fastq_text(bases, quals, ids, 1)
    r2 = b""
    if paired:
        r2 = RL.fastq_text([p[2] for p in pairs], [p[4] for p in pairs], ids, 2, eol=eol2)
        bases, quals = bases + [p[2] for p in pairs], quals + [p[4] for p in pairs]
    return {"entries": world["entries"], "taxdb": world["taxdb"], "bases": bases, "quals": quals, "ids": ids, "n_pairs": n, "r1": r1, "r2": r2}


def chain_batch(oracle, world, kind, paired=True):
    """one batch -- a kind alone -- through the oracle chain (oracle.align_to_database -> tail_oracle -> taxonomy_oracle), computed
    once per world.  -> dict: ids / bases / quals by read ([R1 block | R2 block] when paired), n (records), ov / pool (the
    alignments and their CIGAR pool), rp / pr (the final read pairs and alignment pairs), st (the tail's statistics: the overlap
    records past the threshold, the insert sizes that fed the limit, the limit), sam, tax (one id per read pair), per_read"""
    import importlib
    key = (kind, paired)
    memo = world.setdefault("_chain", {})
    if key in memo:
        return memo[key]
    T = importlib.import_module("kslam_amd.tail")          # ctypes structures only (views / params)
    case = case_of(world, [kind], paired)
    ents = world["entries"]
    gb = [e["bases"] for e in ents]
    index = T.Index(gb, locus_tags=[e["locusTag"] for e in ents], taxonomy_ids=[e["taxonomyID"] for e in ents],
                    genes=[[(g["start"], g["stop"], g["geneName"], g["proteinID"], g["product"]) for g in e["genes"]] for e in ents])
    P = T.TailParams.default(score_threshold=SCORE_THRESHOLD, paired=paired)
    ids = case["ids"] * (2 if paired else 1)
    ov, pool, _ = oracle.align_to_database(case["bases"], gb, oracle.Params.default(score_threshold=SCORE_THRESHOLD))
    reads = T.Reads(case["bases"], case["quals"], ids)
    st, st2 = T.TailStats(), T.TailStats()
    sam = oracle.tail_sam(P, reads.view, index.view, ov, pool, stats=st)
    rp, pr = oracle.tail_pairs(P, reads.view, ov, stats=st2)
    assert st.max_insert_size == st2.max_insert_size and st.n_read_pairs == len(rp)
    tree = oracle.taxonomy_tree(world["taxdb"])
    tax = [tree.lca([ents[int(e)]["taxonomyID"] for e in pr["entry"][int(g["first"]):int(g["first"]) + int(g["count"])]]) for g in rp]
    tree.close()
    per_read = b"".join(b"%s\t%d\n" % (ids[int(g["r1_read"])], x) for g, x in zip(rp, tax))
    memo[key] = {"kind": kind, "paired": paired, "ids": ids, "bases": case["bases"], "quals": case["quals"], "n": case["n_pairs"], "ov": ov,
                 "pool": pool, "rp": rp, "pr": pr, "sam": sam, "tax": tax, "per_read": per_read,
                 "st": {"n_overlaps_screened": int(st.n_overlaps_screened), "n_insert_sizes": int(st.n_insert_sizes),
                        "max_insert_size": int(st.max_insert_size)}}
    return memo[key]


def sam_header(oracle, world, command_line=COMMAND_LINE):
    import importlib
    T = importlib.import_module("kslam_amd.tail")
    ents = world["entries"]
    index = T.Index([e["bases"] for e in ents], locus_tags=[e["locusTag"] for e in ents], taxonomy_ids=[e["taxonomyID"] for e in ents])
    return oracle.sam_header(index.view, command_line)


def plan(world, kinds, without=()):
    """the pairs per batch a loop with PAIRS_PER_BATCH cuts the sequence into"""
    n = sum(len(world["kinds"][kind]) for kind in kinds if kind not in without)
    return [min(PAIRS_PER_BATCH, n - lo) for lo in range(0, n, PAIRS_PER_BATCH)]
