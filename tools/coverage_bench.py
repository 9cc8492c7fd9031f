#!/usr/bin/env python3
"""Rate of the coverage table's passes (include/kslam_coverage.h, csrc/coverage.hip) on one batch shaped like BASELINE
configs[1]: 1 M pairs x 2 x 150 bases against the synthetic species x strains database of bench.py, aligned and paired by the
library itself; the batch's overlap records, read pairs and alignment pairs then go through kslam_coverage_add.

Two shapes: "workload" (the alignment pairs as the pipeline left them) and "contended" (the same records with every interval
moved onto one 10 kb region of entry 0: thousands of reads per bitmap word).  Per shape 2 warm-up and 5 timed mark passes
(kslam_coverage_kernel_ms: HIP events around the mark and unique-read-pair kernels) after a reset each, and one count pass.
Prints, and writes to profiles/coverage.json, the medians.  The sums of the rows are checked against numpy sums over the
arrays.  The GPU step runs in a child process under a time limit of its own; a run that finds no GPU fails.

    python tools/coverage_bench.py [--pairs 1000000] [--species 250] [--strains 5] [--genome-len 4000000] [--warmup 2] [--repeats 5]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import importlib
    import torch
    from __graft_entry__ import load_package
    K = load_package()
    W = importlib.import_module("kslam_amd.workload")
    CV = importlib.import_module("kslam_amd.coverage")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, a.strains, a.genome_len)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150)
    torch.cuda.synchronize()
    n_entries = len(offs) - 1
    ctx = K.Context()
    ctx.set_index_device(n_entries, db.data_ptr(), offs)
    n_reads = reads.shape[0]
    ctx.load_reads_device(n_reads, reads.data_ptr(), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(150))
    ctx.align_resident()
    ctx.pair_screen(paired=True, stages=3)
    rp, pr = ctx.take_pairs()
    ov, _, release = ctx.take_results()
    ov = ov.copy()
    release()
    ctx.set_pairing(stages=3)
    CV.set_coverage(ctx, True)
    out = {"pairs": a.pairs, "entries": n_entries, "database_bases": int(offs[-1]), "overlap_records": len(ov), "read_pairs": len(rp),
           "alignment_pairs": len(pr), "bitmap_bytes": int(sum((int(offs[e + 1] - offs[e]) + 63) // 64 for e in range(n_entries)) * 8)}
    rng = np.random.default_rng(3)
    hot_ov, hot_pr = ov.copy(), pr.copy()
    hot_ov["entry"] = 0
    hot_ov["ref_begin"] = rng.integers(0, 10000 - 150, len(ov))
    hot_ov["ref_end"] = hot_ov["ref_begin"] + 149
    hot_pr["entry"] = 0
    for shape, o, p in (("workload", ov, pr), ("contended", hot_ov, hot_pr)):
        marks = []
        for it in range(a.warmup + a.repeats):
            CV.reset(ctx)
            CV.add(ctx, o, rp, p)
            if it >= a.warmup:
                marks.append(CV.kernel_ms(ctx)[0])
        rows, skipped = CV.take(ctx)
        live = np.repeat(rp["first"].astype(np.int64) - np.concatenate([[0], np.cumsum(rp["count"].astype(np.int64))[:-1]]), rp["count"].astype(np.int64)) + np.arange(int(rp["count"].sum()))
        mates = np.concatenate([p["r1"][live], p["r2"][live]])
        mates = mates[mates != 0xFFFFFFFF]
        spans = (o["ref_end"][mates].astype(np.int64) - o["ref_begin"][mates] + 1).sum()
        if int(rows["alignments"].sum()) != len(live) or int(rows["aligned_bases"].sum()) != int(spans) or skipped:
            sys.exit("the rows' sums differ from the arrays' (%s): %d alignments for %d live records, %d aligned bases for %d, %d skipped"
                     % (shape, rows["alignments"].sum(), len(live), rows["aligned_bases"].sum(), spans, skipped))
        out[shape] = {"mark_ms_all": marks, "mark_ms_median": float(np.median(marks)), "count_ms": CV.kernel_ms(ctx)[1],
                      "live_alignment_pairs": int(len(live)), "mates": int(len(mates)), "covered_bases": int(rows["covered_bases"].sum()),
                      "entries_with_alignments": int((rows["alignments"] > 0).sum())}
    CV.set_coverage(ctx, False)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--strains", type=int, default=5)
    ap.add_argument("--genome-len", type=int, default=4000000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(a.pairs), "--species", str(a.species), "--strains",
                        str(a.strains), "--genome-len", str(a.genome_len), "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                       capture_output=True, text=True, timeout=a.timeout)
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
