#!/usr/bin/env python3
"""Rate of the per-gene table's passes (include/kslam_genes.h, csrc/genes.hip) on one synthetic batch of BASELINE configs[1]'s
shape: 1 M read pairs with 1.75 M alignment-pair records over a database of entries with 4 000 genes each (gene k of an entry
covers [1000 k + 50, 1000 k + 950); every tenth entry also has a gene that spans the whole entry, so that the running maximum
keeps the indexed lookup's window open there).

Two shapes: "spread" (the records spread evenly over entries and genes) and "skewed" (90 % of the records on one gene).  Per
shape the count pass runs with the indexed lookup and with the linear walk ALTERNATING in one process (2 warm-up and 5 timed
passes each, after a reset each; kslam_genes_kernel_ms: HIP events around the count, flag and unique-read-pair kernels), then one
take.  The index build is timed at switch-on.  The coverage table's mark pass over the same records (one 150-base mate per
record) in the same run serves as a yardstick.  The rows of the two lookups are compared with each other and their sums with
numpy sums over the arrays.  Prints, and writes to profiles/genes.json, the medians.  The GPU step runs in a child process
under a time limit of its own; a run that finds no GPU fails.

    python tools/genes_bench.py [--pairs 1000000] [--entries 32] [--genes 4000] [--warmup 2] [--repeats 5]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(a, skewed):
    """-> (read pairs, alignment-pair records, overlap records, the expected number of records inside a gene)"""
    import importlib
    K = sys.modules["kslam_amd"]
    T = importlib.import_module("kslam_amd.tail")
    rng = np.random.default_rng(11 if skewed else 10)
    sizes = np.tile(np.array([1, 2, 2, 2], dtype=np.int64), (a.pairs + 3) // 4)[:a.pairs]
    n = int(sizes.sum())
    rp = np.zeros(a.pairs, dtype=T.READ_PAIR_DT)
    rp["r1_read"], rp["r2_read"] = np.arange(a.pairs), np.arange(a.pairs) + a.pairs
    rp["first"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rp["count"] = sizes
    entry = rng.integers(0, a.entries, n)
    gene = rng.integers(0, a.genes, n)
    offset = rng.integers(0, 1000, n)
    if skewed:
        hot = rng.random(n) < 0.9
        entry[hot], gene[hot], offset[hot] = 1, a.genes // 2, rng.integers(100, 400, int(hot.sum()))
    pr = np.zeros(n, dtype=T.PAIRED_OVERLAP_DT)
    pr["entry"] = entry
    pr["ref_start"] = 1000 * gene + offset
    pr["ref_end"] = pr["ref_start"] + 450
    pr["r1"], pr["r2"] = np.arange(n), 0xFFFFFFFF
    ov = np.zeros(n, dtype=K.OVERLAP_DT)
    ov["entry"], ov["ref_begin"] = entry, pr["ref_start"]
    ov["ref_end"] = np.minimum(pr["ref_start"] + 149, 1000 * a.genes - 1)
    # inside a gene: [start, start + 450) meets [1000 k + 50, 1000 k + 950) of its own or the next k -- always, but for the last
    # gene's tail; the entries with a spanning gene take everything
    own = (np.minimum(pr["ref_end"], 1000 * gene + 950) - np.maximum(pr["ref_start"], 1000 * gene + 50)) > 0
    nxt = (gene + 1 < a.genes) & ((pr["ref_end"] - (1000 * (gene + 1) + 50)) > 0)
    return rp, pr, ov, int((own | nxt | (entry % 10 == 0)).sum())


def child(a):
    import importlib
    from __graft_entry__ import load_package
    K = load_package()
    GN = importlib.import_module("kslam_amd.genes")
    CV = importlib.import_module("kslam_amd.coverage")
    ST = importlib.import_module("kslam_amd.samtext")
    length = 1000 * a.genes
    first, starts, stops = [0], [], []
    for e in range(a.entries):
        if e % 10 == 0:
            starts.append(0)
            stops.append(length)
        starts += [1000 * k + 50 for k in range(a.genes)]
        stops += [1000 * k + 950 for k in range(a.genes)]
        first.append(len(starts))
    index = GN.GeneIndex(first, starts, stops, entry_lengths=[length] * a.entries)
    ctx = K.Context()
    rng = np.random.default_rng(1)
    ctx.set_index_arrays(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), length * a.entries), np.arange(a.entries + 1, dtype=np.uint64) * length)
    ctx.set_pairing(stages=3)
    ST.set_annotations(ctx, index)
    builds = []
    for _ in range(a.warmup + a.repeats):
        GN.set_genes(ctx, False)
        GN.set_genes(ctx, True)
        builds.append(GN.kernel_ms(ctx)[0])
    CV.set_coverage(ctx, True)
    out = {"pairs": a.pairs, "entries": a.entries, "genes_per_entry": a.genes, "genes": len(starts), "index_bytes": 16 * len(starts),
           "build_ms_all": builds[a.warmup:], "build_ms_median": float(np.median(builds[a.warmup:]))}
    for shape in ("spread", "skewed"):
        rp, pr, ov, inside = batch(a, shape == "skewed")
        times, rows = {"indexed": [], "linear": []}, {}
        for it in range(a.warmup + a.repeats):
            for mode in ("indexed", "linear"):   # alternating
                os.environ["KSLAM_GENES_LOOKUP"] = mode
                GN.reset(ctx)
                GN.add(ctx, rp, pr)
                if it >= a.warmup:
                    times[mode].append(GN.kernel_ms(ctx)[1])
                if it == a.warmup + a.repeats - 1:
                    rows[mode] = GN.take(ctx)
        del os.environ["KSLAM_GENES_LOOKUP"]
        take_ms = GN.kernel_ms(ctx)[2]
        got, st = rows["indexed"]
        if got.tolist() != rows["linear"][0].tolist() or st != rows["linear"][1]:
            sys.exit("the indexed and the linear count pass differ (%s)" % shape)
        if st["n_alignments"] != len(pr) or st["n_in_gene"] != inside or int(got["alignments"].sum()) != inside or st["n_skipped"]:
            sys.exit("the rows' sums differ from the arrays' (%s): %r for %d records, %d of them inside a gene" % (shape, st, len(pr), inside))
        marks = []
        for it in range(a.warmup + a.repeats):
            CV.reset(ctx)
            CV.add(ctx, ov, rp, pr)
            if it >= a.warmup:
                marks.append(CV.kernel_ms(ctx)[0])
        out[shape] = {"alignment_pairs": len(pr), "in_gene": inside, "rows": len(got), "unique_read_pairs": int(got["unique_read_pairs"].sum()),
                      "count_indexed_ms_all": times["indexed"], "count_indexed_ms_median": float(np.median(times["indexed"])),
                      "count_linear_ms_all": times["linear"], "count_linear_ms_median": float(np.median(times["linear"])),
                      "take_ms": take_ms, "coverage_mark_ms_all": marks, "coverage_mark_ms_median": float(np.median(marks))}
    CV.set_coverage(ctx, False)
    GN.set_genes(ctx, False)
    ctx.set_pairing(stages=0)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--entries", type=int, default=32)
    ap.add_argument("--genes", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genes.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(a.pairs), "--entries", str(a.entries), "--genes",
                        str(a.genes), "--warmup", str(a.warmup), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    out = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    out["warmup"], out["repeats"] = a.warmup, a.repeats
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
