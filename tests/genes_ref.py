"""The per-gene abundance table of include/kslam_genes.h, restated in plain Python from the header's text (a linear walk over the
entry's genes, dictionaries, the writer with the header's expression order), and the builder of the cases the host twin and the
device are held to.  Shares no code with host/genes.cpp.

A case is a dict: name, first (gene_first, one more than entries), starts / stops (the gene columns), rp / pr (the read pairs
and alignment-pair records as structured arrays laid out like kslam_read_pair and kslam_paired_overlap)."""
import numpy as np

COUNT_BLOCK = 256   # csrc/common.h: GENES_BLOCK, the count pass's workgroup
PAIRED_OVERLAP_DT = np.dtype([("combined_score", "<u4"), ("entry", "<u4"), ("ref_start", "<i4"), ("ref_end", "<i4"),
                              ("insert_size", "<u4"), ("r1", "<u4"), ("r2", "<u4"), ("pad", "<u4")])
READ_PAIR_DT = np.dtype([("r1_read", "<u4"), ("r2_read", "<u4"), ("first", "<u8"), ("count", "<u8")])
ROW_DT = np.dtype([("gene", "<u8"), ("alignments", "<u8"), ("unique_read_pairs", "<u8"), ("overlap_bases", "<u8")])
HEADER = (b"#entry\tlocus\ttaxid\tgene\tstart\tstop\tlength\tname\tprotein_id\tproduct\talignments\tunique_read_pairs\toverlap_bases"
          b"\trpk\ttpm\n")
NONE, SKIPPED = -1, -2


# ---------------------------------------------------------------- the definition

def gene_of(first, starts, stops, entry, ref_start, ref_end):
    """-> (gene, shared): the gene of the entry with the strictly largest shared > 0, the lowest index among equals; (NONE, 0)
    without one; (SKIPPED, 0) for an entry the index does not have"""
    if entry >= len(first) - 1:
        return SKIPPED, 0
    best, widest = NONE, 0
    for g in range(int(first[entry]), int(first[entry + 1])):
        shared = min(int(ref_end), int(stops[g])) - max(int(ref_start), int(starts[g]))
        if shared > widest:
            best, widest = g, shared
    return best, widest


def lookups(first, starts, stops, entries, ref_starts, ref_ends):
    """gene_of over arrays -> (genes int64, shared int64)"""
    got = [gene_of(first, starts, stops, int(e), int(b), int(t)) for e, b, t in zip(entries, ref_starts, ref_ends)]
    return np.array([g for g, _ in got], dtype=np.int64), np.array([s for _, s in got], dtype=np.int64)


def table(c):
    """-> (rows [ROW_DT: the genes with alignments > 0, ascending], statistics)"""
    counts = {}
    st = {"n_alignments": 0, "n_in_gene": 0, "n_no_gene": 0, "n_skipped": 0, "n_rows": 0}
    for g in c["rp"]:
        live = c["pr"][int(g["first"]):int(g["first"]) + int(g["count"])]   # the records behind first + count are dead
        genes = []
        for p in live:
            gene, shared = gene_of(c["first"], c["starts"], c["stops"], int(p["entry"]), int(p["ref_start"]), int(p["ref_end"]))
            genes.append(gene)
            st["n_alignments"] += 1
            st["n_in_gene" if gene >= 0 else "n_no_gene" if gene == NONE else "n_skipped"] += 1
            if gene >= 0:
                row = counts.setdefault(gene, [0, 0, 0])
                row[0] += 1
                row[2] += shared
        if genes and min(genes) >= 0 and len(set(genes)) == 1:
            counts[genes[0]][1] += 1
    rows = np.array([(g, *counts[g]) for g in sorted(counts)], dtype=ROW_DT) if counts else np.zeros(0, dtype=ROW_DT)
    st["n_rows"] = len(rows)
    return rows, st


def text(rows, first, starts, stops, loci, taxids, names, protein_ids, products):
    """the file's bytes, formatted here"""
    lengths = [int(stops[int(r["gene"])]) - int(starts[int(r["gene"])]) for r in rows]
    rpk = [int(r["alignments"]) * 1000.0 / length if length > 0 else 0.0 for r, length in zip(rows, lengths)]
    total = 0.0
    for v in rpk:   # in row order
        total += v
    out = [HEADER]
    for r, length, v in zip(rows, lengths, rpk):
        g = int(r["gene"])
        e = max(k for k in range(len(first) - 1) if int(first[k]) <= g)
        tpm = v * 1e6 / total if total != 0 else 0.0
        out.append(b"%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (
            e, loci[e], int(taxids[e]), g, int(starts[g]), int(stops[g]), length, names[g], protein_ids[g], products[g], int(r["alignments"]),
            int(r["unique_read_pairs"]), int(r["overlap_bases"]), b"%.4f" % v, b"%.4f" % tpm))
    return b"".join(out)


# ---------------------------------------------------------------- the cases

def arrays(name, first, starts, stops, rp, pr):
    p = np.zeros(len(pr), dtype=PAIRED_OVERLAP_DT)
    if len(pr):
        t = np.asarray(pr, dtype=np.int64).reshape(-1, 3)
        p["entry"], p["ref_start"], p["ref_end"] = t[:, 0], t[:, 1], t[:, 2]
        p["combined_score"] = 100
        p["r1"] = np.arange(len(pr))
        p["r2"] = 0xFFFFFFFF
    r = np.zeros(len(rp), dtype=READ_PAIR_DT)
    if len(rp):
        t = np.asarray(rp, dtype=np.int64).reshape(-1, 4)
        r["r1_read"], r["r2_read"], r["first"], r["count"] = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    return {"name": name, "first": np.asarray(first, dtype=np.uint64), "starts": np.asarray(starts, dtype=np.int32),
            "stops": np.asarray(stops, dtype=np.int32), "rp": r, "pr": p}


def genes_of(per_entry):
    """a list (per entry) of lists of (start, stop) -> (first, starts, stops)"""
    first, starts, stops = [0], [], []
    for genes in per_entry:
        for b, t in genes:
            starts.append(b)
            stops.append(t)
        first.append(len(starts))
    return first, starts, stops


def build(name, per_entry, groups):
    """groups: a list of (live, dead) record lists; a record is (entry, ref_start, ref_end).  The dead records follow the live
    ones in the pairs array, as device pseudo-assembly leaves them."""
    pr, rp = [], []
    n_groups = len(groups)
    for g, (live, dead) in enumerate(groups):
        rp.append((g, n_groups + g, len(pr), len(live)))
        pr.extend(list(live) + list(dead))
    return arrays(name, *genes_of(per_entry), rp, pr)


def random_genes(rng, n_entries, max_genes, span=5000):
    """gene columns with everything the lookup must bear: unsorted file order, nesting, duplicates, stop < start, negative
    starts, genes past the span, entries without genes"""
    per_entry = []
    for _ in range(n_entries):
        genes = []
        for _ in range(int(rng.integers(0, max_genes + 1))):
            kind = rng.random()
            b = int(rng.integers(-50, span))
            t = b + int(rng.integers(1, 400))
            if kind < 0.1 and genes:
                b, t = genes[int(rng.integers(0, len(genes)))]          # a duplicate
            elif kind < 0.2:
                t = b + int(rng.integers(400, span))                    # a long gene: others nest in it
            elif kind < 0.25:
                b, t = t, b                                             # stop < start
            elif kind < 0.3:
                b, t = span + b, span + t + 100                         # past the entry's end
            genes.append((b, t))
        per_entry.append(genes)
    return per_entry


def random_case(name, seed, n_pairs, n_entries, max_genes, invalid=True, max_group=6, per_entry=None, span=5000):
    """n_pairs alignment-pair records (live and dead) in groups of random size over random genes"""
    rng = np.random.default_rng(seed)
    per_entry = random_genes(rng, n_entries, max_genes, span) if per_entry is None else per_entry
    n_entries = len(per_entry)
    pr, rp = [], []
    while len(pr) < n_pairs:
        size = int(min(rng.integers(1, max_group + 1), n_pairs - len(pr)))
        live = int(rng.integers(0, size + 1)) if rng.random() < 0.3 else size
        home = int(rng.integers(0, n_entries))
        anchor = int(rng.integers(-100, span + 200))
        rp.append((len(rp), len(rp) + 1000000, len(pr), live))
        for _ in range(size):
            e = home if rng.random() < 0.85 else int(rng.integers(0, n_entries + (2 if invalid else 0)))
            b = anchor + int(rng.integers(-30, 30)) if rng.random() < 0.8 else int(rng.integers(-100, span + 200))
            t = b + int(rng.integers(-5, 300))
            pr.append((e, b, t))
    return arrays(name, *genes_of(per_entry), rp, pr)


def cases():
    out = []
    one = [[(100, 400)]]
    two = [[(100, 400), (1000, 1500)], [(0, 50)]]
    hit, other, none = (0, 150, 300), (0, 1100, 1200), (0, 500, 600)
    # ---- one wavefront on one gene; two genes alternating lane by lane
    out.append(build("wave-one-gene", one, [([hit], []) for _ in range(64)]))
    out.append(build("wave-alternating", two, [([hit if k % 2 else other], []) for k in range(64)]))
    # ---- record counts that straddle the workgroup
    for n in (COUNT_BLOCK - 1, COUNT_BLOCK, COUNT_BLOCK + 1):
        out.append(build("block-%d" % n, two, [([(0, 100 + k, 250 + k) if k % 3 else (0, 1000 + k, 1100 + k)], []) for k in range(n)]))
    # ---- dead records between groups: they point at a gene nothing else touches
    dead = (1, 0, 50)
    out.append(build("dead", two, [([hit], [dead, dead]), ([], [dead]), ([other, other], []), ([hit], [dead, dead, dead])]))
    out.append(build("group-of-one", one, [([hit], [])]))
    # ---- one group of 3 000 records on one gene; the same with one gene-less record in the middle
    big = [(0, 100 + k % 200, 260 + k % 200) for k in range(3000)]
    out.append(build("big-group", one, [(big, [])]))
    out.append(build("big-group-gap", one, [(big[:1500] + [none] + big[1501:], [])]))
    out.append(build("first-gene-less", one, [([none, hit, hit], [])]))
    out.append(build("only-gene-less", one, [([none, none], []), ([none], [])]))
    out.append(build("skipped", two, [([hit, (2, 150, 300)], []), ([(7, 0, 10)], []), ([hit], [])]))
    out.append(build("two-genes", two, [([hit, other], []), ([other, other], []), ([(1, 0, 10), hit], [])]))
    out.append(build("no-pairs", two, [([], []), ([], [])]))          # read pairs without a record: n_pairs == 0
    out.append(arrays("no-read-pairs", *genes_of(two), [], [hit, other]))
    out.append(build("no-genes", [[], []], [([(0, 0, 100)], []), ([(1, 5, 6), (3, 0, 1)], [])]))
    # ---- grid seams, random
    out.append(random_case("grid-20001", 4242, 20001, 40, 30))
    for n in (1, COUNT_BLOCK + 1):
        out.append(random_case("grid-%d" % n, 100 + n, n, 5, 12, invalid=False))
    return out


def concat(a, b):
    """two cases over the same genes as one batch"""
    rp2 = b["rp"].copy()
    rp2["first"] += len(a["pr"])
    return dict(a, name=a["name"] + "+" + b["name"], rp=np.concatenate([a["rp"], rp2]), pr=np.concatenate([a["pr"], b["pr"]]))


# ---------------------------------------------------------------- the hand-checkable fixture (tests/golden/genes_small.tsv)

SMALL_LOCI = [b"NC_A.1", b"NC_B.2", b"pX"]
SMALL_TAX = [562, 1280, 0]
SMALL_GENES = [   # (start, stop, name, protein_id, product) per entry
    [(100, 400, b"thrA", b"NP_1.1", b"aspartokinase"), (350, 700, b"", b"NP_2.1", b"hypothetical protein"), (50, 250, b"dup", b"", b""),
     (900, 800, b"rev", b"NP_4.1", b"stop before start")],
    [(0, 1000, b"long", b"NP_5.1", b"polyprotein"), (200, 300, b"in", b"NP_6.1", b"nested"), (200, 300, b"in2", b"NP_7.1", b"nested again")],
    [(-20, 80, b"edge", b"NP_8.1", b"starts before the entry"), (10, 10, b"nil", b"", b"empty"), (500, 650, b"far", b"NP_10.1", b"x")]]
SMALL_GROUPS = [
    ([(0, 100, 250), (0, 120, 240)], []),            # genes 0 and 2 share 150 and 120: the tie goes to gene 0, twice
    ([(0, 360, 500), (0, 380, 420)], [(0, 0, 1000)]),   # gene 1 (140, 40) over gene 0 (40, 20); a dead record
    ([(1, 210, 290), (1, 100, 250)], []),            # genes 4, 5, 6 share 80: gene 4; then gene 4 alone (150)
    ([(1, 1200, 1300)], []),                         # no gene
    ([(2, 0, 60), (2, 520, 600)], []),               # gene 7 (60) and gene 9 (80): unique for neither
    ([(5, 0, 10)], []),                              # no such entry
    ([(2, -10, 30)], [])]                            # gene 7 (40)
SMALL_ROWS = [(0, 2, 1, 270), (1, 2, 1, 180), (4, 2, 1, 230), (7, 2, 1, 100), (9, 1, 0, 80)]   # worked out by hand
SMALL_STATS = {"n_alignments": 11, "n_in_gene": 9, "n_no_gene": 1, "n_skipped": 1, "n_rows": 5}
SMALL_EXTRA_ROW = (3, 3, 1, 0)   # handed to the writer among the others: a gene of length <= 0 has rpk 0


def small():
    """-> (case, names, protein_ids, products)"""
    c = build("small", [[(g[0], g[1]) for g in e] for e in SMALL_GENES], SMALL_GROUPS)
    flat = [g for e in SMALL_GENES for g in e]
    return c, [g[2] for g in flat], [g[3] for g in flat], [g[4] for g in flat]
