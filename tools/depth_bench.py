#!/usr/bin/env python3
"""Rate of the depth track's passes (include/kslam_depth.h, csrc/depth.hip) on batches shaped like BASELINE configs[1]: 1 M pairs
x 2 x 150 bases against the synthetic species x strains database of bench.py, aligned and paired by the library itself; each
batch's overlap records, CIGAR pool, read offsets, read pairs and alignment pairs then go through kslam_depth_add.

34 DIFFERENT batches (the reads' seed differs) are made.  On the first: 2 warm-up and 5 timed emit passes after a reset each
(kslam_depth_kernel_ms), and the SNV table's emit on the same batch in the same process as the yardstick
(kslam_variants_kernel_ms).  Then, with the threshold out of the way: batch 1 and a take (the state after 1 batch), batches 2-17
and a take (after 17), batches 18-34 and a take -- ONE compaction of 17 batches' pending keys into an existing state -- and the
state after 34; the take at min_depth 1 and the same take again.  The 17 last batches are then added and compacted
warm-up + repeats times more (their boundaries are in the state by then: the sort is the same, the merge finds every key), for a
median.  Prints, and writes to profiles/depth.json, the medians and the state's bytes.  The statistics are checked against numpy
sums over the arrays.  The GPU step runs in a child process under a time limit of its own; a run that finds no GPU fails.

    python tools/depth_bench.py [--pairs 1000000] [--species 250] [--strains 5] [--genome-len 4000000] [--batches 34] [--warmup 2] [--repeats 5]
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
    VR = importlib.import_module("kslam_amd.variants")
    DP = importlib.import_module("kslam_amd.depth")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, a.strains, a.genome_len)
    n_entries = len(offs) - 1
    ctx = K.Context()
    ctx.set_index_device(n_entries, db.data_ptr(), offs)

    def batch(k):
        gen.manual_seed(2 + k)
        reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150)
        torch.cuda.synchronize()
        n_reads = reads.shape[0]
        roff = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(150)
        ctx.set_pairing(stages=0)
        ctx.load_reads_device(n_reads, reads.data_ptr(), roff)
        qual = torch.full((n_reads * 150 + 64,), ord("I"), dtype=torch.uint8, device=dev)
        ctx.load_qualities_device(qual.data_ptr())
        ctx.align_resident()
        ctx.pair_screen(paired=True, stages=3)
        rp, pr = ctx.take_pairs()
        ov, cg, release = ctx.take_results()
        ov, cg = ov.copy(), cg.copy()
        release()
        ctx.set_pairing(stages=3)
        return ov, cg, roff, rp.copy(), pr.copy(), (reads.reshape(-1).cpu().numpy() if k == 0 else None)

    def add(b):
        DP.add(ctx, b[0], b[1], b[2], b[3], b[4])

    first = batch(0)
    ov, cg, roff, rp, pr, rbases = first
    VR.set_variants(ctx, True)
    snv = []
    for it in range(a.warmup + a.repeats):
        VR.reset(ctx)
        VR.add(ctx, ov, cg, rbases, roff, rp, pr)
        if it >= a.warmup:
            snv.append(VR.kernel_ms(ctx)[0])
    _, vstats = VR.take(ctx, 2, 1)
    VR.set_variants(ctx, False)
    DP.set_depth(ctx, True)
    DP.set_compact_at(ctx, 1 << 31)
    emits = []
    for it in range(a.warmup + a.repeats):
        DP.reset(ctx)
        add(first)
        if it >= a.warmup:
            emits.append(DP.kernel_ms(ctx)[0])
    # the statistics against the arrays: every M operation of a named record is one interval (none of this batch's records is skipped)
    live = np.repeat(rp["first"].astype(np.int64) - np.concatenate([[0], np.cumsum(rp["count"].astype(np.int64))[:-1]]), rp["count"].astype(np.int64)) + np.arange(int(rp["count"].sum()))
    named = np.unique(np.concatenate([pr["r1"][live], pr["r2"][live]]))
    named = named[named != 0xFFFFFFFF]
    lens, starts = ov["cigar_len"][named].astype(np.int64), ov["cigar_off"][named].astype(np.int64)
    ops = cg[np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))]
    n_m = int(((ops & 15) == 0).sum() - (ops == 0).sum())
    rows, stats = DP.take(ctx, 1)
    state = {1: {"keys": stats["n_keys"], "bytes": 16 * stats["n_keys"], "rows": stats["n_rows"], "covered_bases": stats["covered_bases"]}}
    first_compact_ms = DP.kernel_ms(ctx)[1]
    if stats["n_records"] != len(named) or stats["n_skipped"] or stats["n_intervals"] != n_m or \
            [stats[k] for k in ("n_records", "n_skipped", "n_intervals")] != [vstats[k] for k in ("n_records", "n_skipped", "n_intervals")]:
        sys.exit("the statistics differ from the arrays': %r for %d named records with %d M operations" % (stats, len(named), n_m))
    if int((rows["end"].astype(np.int64) - rows["start"]).sum()) != stats["covered_bases"] or int(rows["depth"].max()) != stats["max_depth"]:
        sys.exit("the rows differ from their statistics: %r" % stats)
    half = (a.batches + 1) // 2
    kept = []
    for k in range(1, a.batches):
        b = batch(k)
        add(b)
        if k >= half:
            kept.append(b)
        if k == half - 1:
            _, stats = DP.take(ctx, 1)
            state[half] = {"keys": stats["n_keys"], "bytes": 16 * stats["n_keys"], "rows": stats["n_rows"], "covered_bases": stats["covered_bases"]}
    before = stats["n_intervals"]
    rows, stats = DP.take(ctx, 1)
    _, compact_fresh_ms, take_ms = DP.kernel_ms(ctx)
    pending_keys = 2 * (stats["n_intervals"] - before)
    state[a.batches] = {"keys": stats["n_keys"], "bytes": 16 * stats["n_keys"], "rows": stats["n_rows"], "covered_bases": stats["covered_bases"]}
    rows_again, _ = DP.take(ctx, 1)
    _, compact_after, take_again_ms = DP.kernel_ms(ctx)
    if rows.tobytes() != rows_again.tobytes() or compact_after != compact_fresh_ms:
        sys.exit("a take without an add in between differs from the one before, or compacted again")
    compacts, takes = [], []
    for it in range(a.warmup + a.repeats):
        for b in kept:
            add(b)
        DP.take(ctx, 1)
        if it >= a.warmup:
            compacts.append(DP.kernel_ms(ctx)[1])
            takes.append(DP.kernel_ms(ctx)[2])
    out = {"pairs": a.pairs, "entries": n_entries, "database_bases": int(offs[-1]), "batches": a.batches, "overlap_records": len(ov),
           "alignment_pairs": len(pr), "cigar_ops": len(cg), "intervals_first_batch": n_m, "pending_bytes_per_batch": 16 * n_m,
           "emit_ms_all": emits, "emit_ms_median": float(np.median(emits)),
           "snv_emit_ms_all": snv, "snv_emit_ms_median": float(np.median(snv)),
           "compact_1_batch_into_empty_ms": first_compact_ms,
           "compact_batches": len(kept), "compact_pending_keys": pending_keys, "compact_fresh_ms": compact_fresh_ms,
           "compact_again_ms_all": compacts, "compact_again_ms_median": float(np.median(compacts)),
           "take_ms": take_ms, "take_again_ms": take_again_ms, "take_ms_all": takes, "take_ms_median": float(np.median(takes)),
           "rows_min_depth_1": len(rows), "max_depth": stats["max_depth"], "state_after_batches": state,
           "end_to_end_step_on_against_off": "not measured"}
    DP.set_depth(ctx, False)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--strains", type=int, default=5)
    ap.add_argument("--genome-len", type=int, default=4000000)
    ap.add_argument("--batches", type=int, default=34)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(a.pairs), "--species", str(a.species), "--strains",
                        str(a.strains), "--genome-len", str(a.genome_len), "--batches", str(a.batches), "--warmup", str(a.warmup), "--repeats",
                        str(a.repeats)], capture_output=True, text=True, timeout=a.timeout)
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
