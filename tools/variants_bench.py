#!/usr/bin/env python3
"""Rate of the SNV table's passes (include/kslam_variants.h, csrc/variants.hip) on one batch shaped like BASELINE configs[1]:
1 M pairs x 2 x 150 bases against the synthetic species x strains database of bench.py, aligned and paired by the library itself;
the batch's overlap records, CIGAR pool, reads, read pairs and alignment pairs then go through kslam_variants_add.

2 warm-up and 5 timed emit passes (kslam_variants_kernel_ms: HIP events from the first to the last pass of the batch, the host's
looks at the counts between them included) after a reset each, then one take.  The yardsticks, in the same process: the
per-row walk of the same batch (kslam_row_details_of_pairs: k_row_details, its scan and the MD gather; wall clock around the call,
which waits for its stream) and the coverage table's mark pass (kslam_coverage_kernel_ms).  Prints, and writes to
profiles/variants.json, the medians, the events and intervals of the batch and the bytes of state per million pairs.  The
statistics are checked against numpy sums over the arrays.  The GPU step runs in a child process under a time limit of its own;
a run that finds no GPU fails.

    python tools/variants_bench.py [--pairs 1000000] [--species 250] [--strains 5] [--genome-len 4000000] [--warmup 2] [--repeats 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

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
    VR = importlib.import_module("kslam_amd.variants")
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
    roff = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(150)
    ctx.load_reads_device(n_reads, reads.data_ptr(), roff)
    qual = torch.full((n_reads * 150 + 64,), ord("I"), dtype=torch.uint8, device=dev)
    ctx.load_qualities_device(qual.data_ptr())
    ctx.align_resident()
    ctx.pair_screen(paired=True, stages=3)
    walks = []
    for it in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.row_details(of_pairs=True)
        if it >= a.warmup:
            walks.append((time.perf_counter() - t0) * 1e3)
    rp, pr = ctx.take_pairs()
    ov, cg, release = ctx.take_results()
    ov, cg = ov.copy(), cg.copy()
    release()
    rbases = reads.reshape(-1).cpu().numpy()
    ctx.set_pairing(stages=3)
    CV.set_coverage(ctx, True)
    marks = []
    for it in range(a.warmup + a.repeats):
        CV.reset(ctx)
        CV.add(ctx, ov, rp, pr)
        if it >= a.warmup:
            marks.append(CV.kernel_ms(ctx)[0])
    CV.set_coverage(ctx, False)
    VR.set_variants(ctx, True)
    emits = []
    for it in range(a.warmup + a.repeats):
        VR.reset(ctx)
        VR.add(ctx, ov, cg, rbases, roff, rp, pr)
        if it >= a.warmup:
            emits.append(VR.kernel_ms(ctx)[0])
    rows, stats = VR.take(ctx, 2, 1)
    take_ms = VR.kernel_ms(ctx)[1]
    rows_again, _ = VR.take(ctx, 2, 1)      # sorted already: heads, depth and compaction alone
    take_sorted_ms = VR.kernel_ms(ctx)[1]
    live = np.repeat(rp["first"].astype(np.int64) - np.concatenate([[0], np.cumsum(rp["count"].astype(np.int64))[:-1]]), rp["count"].astype(np.int64)) + np.arange(int(rp["count"].sum()))
    named = np.unique(np.concatenate([pr["r1"][live], pr["r2"][live]]))
    named = named[named != 0xFFFFFFFF]
    # every M operation of a named record is one interval (none of this batch's records is skipped)
    lens, starts = ov["cigar_len"][named].astype(np.int64), ov["cigar_off"][named].astype(np.int64)
    ops = cg[np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))]
    n_m = int(((ops & 15) == 0).sum() - (ops == 0).sum())
    if stats["n_records"] != len(named) or stats["n_skipped"] or stats["n_intervals"] != n_m or rows.tobytes() != rows_again.tobytes():
        sys.exit("the statistics differ from the arrays': %r for %d named records with %d M operations" % (stats, len(named), n_m))
    out = {"pairs": a.pairs, "entries": n_entries, "database_bases": int(offs[-1]), "overlap_records": len(ov), "read_pairs": len(rp),
           "alignment_pairs": len(pr), "cigar_ops": len(cg), "stats": stats, "rows_min_alt_2": len(rows),
           "emit_ms_all": emits, "emit_ms_median": float(np.median(emits)), "take_ms": take_ms, "take_sorted_ms": take_sorted_ms,
           "row_details_ms_all": walks, "row_details_ms_median": float(np.median(walks)),
           "coverage_mark_ms_all": marks, "coverage_mark_ms_median": float(np.median(marks)),
           "state_bytes_events_per_million_pairs": 8.0 * stats["n_events"] * 1e6 / a.pairs,
           "state_bytes_intervals_per_million_pairs": 16.0 * stats["n_intervals"] * 1e6 / a.pairs,
           "end_to_end_step_on_against_off": "not measured"}
    VR.set_variants(ctx, False)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants.json"))
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
