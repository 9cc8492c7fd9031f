#!/usr/bin/env python3
"""Rate of the indel table's passes (include/kslam_indels.h, csrc/indels.hip) on one batch shaped like BASELINE configs[1]: 1 M
pairs x 2 x 150 bases against the synthetic species x strains database of bench.py, aligned and paired by the library itself; the
batch's overlap records, CIGAR pool, reads, read pairs and alignment pairs then go through kslam_indels_add.

Emit: 2 warm-up and 5 timed emit passes (kslam_indels_kernel_ms: HIP events from the first to the last pass of the batch, the
host's looks at the counts between them included) after a reset each.  The yardstick, in the same process over the same batch:
the SNV table's emit passes (kslam_variants_kernel_ms), which walk the same records and compare every column.
Take: the batch is added --accumulate times (the keys of several batches over the same entries), then taken --take-repeats + 1
times: the first take sorts the four arrays, the others find them sorted and run the run heads, the strand splits, the depth
lookups, the compactions and the host's merge of the filtered rows alone.
Prints, and writes to profiles/indels.json, every value, the medians, the smallest and largest of the repeats, and the bytes of
state per batch.  The statistics are checked against the SNV table's over the same batch.  The GPU step runs in a child process
under a time limit of its own; a run that finds no GPU fails.

--e2e: the end-to-end step of bench.py's loop with the report off and on, alternating on one context, `rounds` legs each; the
spread of the equal legs is recorded beside the difference.

    python tools/indels_bench.py [--pairs 1000000] [--species 250] [--strains 5] [--genome-len 4000000] [--warmup 2] [--repeats 5]
                                 [--e2e] [--steps 4] [--rounds 3]
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
    ID = importlib.import_module("kslam_amd.indels")
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
    ctx.align_resident()
    ctx.pair_screen(paired=True, stages=3)
    rp, pr = ctx.take_pairs()
    ov, cg, release = ctx.take_results()
    ov, cg = ov.copy(), cg.copy()
    release()
    rbases = reads.reshape(-1).cpu().numpy()
    ctx.set_pairing(stages=3)
    VR.set_variants(ctx, True)
    var_emits = []
    for it in range(a.warmup + a.repeats):
        VR.reset(ctx)
        VR.add(ctx, ov, cg, rbases, roff, rp, pr)
        if it >= a.warmup:
            var_emits.append(VR.kernel_ms(ctx)[0])
    _, var_stats = VR.take(ctx, 2, 1)
    VR.set_variants(ctx, False)
    ID.set_indels(ctx, True)
    emits = []
    for it in range(a.warmup + a.repeats):
        ID.reset(ctx)
        ID.add(ctx, ov, cg, rbases, roff, rp, pr)
        if it >= a.warmup:
            emits.append(ID.kernel_ms(ctx)[0])
    for _ in range(a.accumulate - 1):
        ID.add(ctx, ov, cg, rbases, roff, rp, pr)
    takes, rows, stats = [], None, None
    for it in range(a.take_repeats + 1):
        rows, stats = ID.take(ctx, 2, 1)
        takes.append(ID.kernel_ms(ctx)[1])
    all_rows, _ = ID.take(ctx, 1, 0)
    # the M runs and the contributing records are the SNV table's
    if stats["n_records"] != a.accumulate * var_stats["n_records"] or stats["n_intervals"] != a.accumulate * var_stats["n_intervals"] or stats["n_skipped"]:
        sys.exit("the statistics differ from the SNV table's: %r against %r" % (stats, var_stats))
    if len(all_rows) != stats["n_sites"] or int(all_rows["alt_fwd"].sum() + all_rows["alt_rev"].sum()) != stats["n_deletions"] + stats["n_insertions"]:
        sys.exit("the rows do not add up to the events: %r" % (stats,))
    keys = 2 * stats["n_intervals"] + stats["n_deletions"] + stats["n_insertions"]
    state_bytes = 16 * stats["n_intervals"] + 8 * stats["n_deletions"] + 16 * stats["n_insertions"]
    sorted_takes = takes[1:]
    out = {"pairs": a.pairs, "entries": n_entries, "database_bases": int(offs[-1]), "overlap_records": len(ov), "read_pairs": len(rp),
           "alignment_pairs": len(pr), "cigar_ops": len(cg), "batches_accumulated": a.accumulate, "stats": stats,
           "rows_min_alt_2": len(rows), "rows_all": len(all_rows), "rows_with_more_alt_than_depth": int((all_rows["alt_fwd"].astype(np.int64) + all_rows["alt_rev"] > all_rows["depth"]).sum()),
           "emit_ms_all": emits, "emit_ms_median": float(np.median(emits)), "emit_ms_min_max": [min(emits), max(emits)],
           "variants_emit_ms_all": var_emits, "variants_emit_ms_median": float(np.median(var_emits)),
           "variants_emit_ms_min_max": [min(var_emits), max(var_emits)],
           "emit_over_variants_emit": float(np.median(emits) / np.median(var_emits)),
           "take_first_ms_with_sorts": takes[0], "take_sorted_ms_all": sorted_takes, "take_sorted_ms_median": float(np.median(sorted_takes)),
           "take_sorted_ms_min_max": [min(sorted_takes), max(sorted_takes)], "stored_keys": keys,
           "sort_ms": takes[0] - float(np.median(sorted_takes)),
           "state_bytes_per_batch": state_bytes / a.accumulate,
           "end_to_end_step_on_against_off": "not measured"}
    ID.set_indels(ctx, False)
    ctx.close()
    print("RESULT " + json.dumps(out))


def e2e_child(a):
    import importlib
    import torch
    torch.cuda.init()   # torch carries its own copy of the HIP runtime and has to open the GPU before the library does
    from __graft_entry__ import load_package
    from bench_legs import FastqFiles, e2e_leg
    K = load_package()
    ID = importlib.import_module("kslam_amd.indels")
    W, T, X = [importlib.import_module("kslam_amd." + m) for m in ("workload", "tail", "taxonomy")]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, a.strains, a.genome_len)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150)
    ctx = K.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    tax_text, entry_tax = W.taxonomy(a.species, a.strains)
    index_view = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(K, dev, [reads], 150)
    del reads
    torch.cuda.empty_cache()
    taxdb = X.TaxDB(tax_text)
    o = {"ms_per_step_off": [], "ms_per_step_on": []}
    for _ in range(a.rounds):
        for on in (False, True):
            if on:
                ctx.set_pairing(stages=3)   # (the switch asks for it; the loop sets its own stages and takes them back)
            ID.set_indels(ctx, on)          # the lanes pile up every batch of the leg; the take is not part of a step
            leg = e2e_leg(K, ctx, files, a.pairs, index_view, taxdb, a.steps, 2, False, reps=1, tag="ind" if on else "plain", out_dir=a.out_dir)
            o["ms_per_step_on" if on else "ms_per_step_off"].append(leg["ms_per_step"])
    ID.set_indels(ctx, False)
    files.close()
    ctx.close()
    off, on = float(np.median(o["ms_per_step_off"])), float(np.median(o["ms_per_step_on"]))
    o.update(pairs=a.pairs, steps=a.steps, rounds=a.rounds, ms_per_step_off_median=off, ms_per_step_on_median=on, difference_ms=on - off,
             spread_of_off_legs_ms=max(o["ms_per_step_off"]) - min(o["ms_per_step_off"]),
             spread_of_on_legs_ms=max(o["ms_per_step_on"]) - min(o["ms_per_step_on"]))
    o["on_median_inside_the_off_legs_range"] = min(o["ms_per_step_off"]) <= on <= max(o["ms_per_step_off"])
    print("RESULT " + json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--strains", type=int, default=5)
    ap.add_argument("--genome-len", type=int, default=4000000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--accumulate", type=int, default=3)
    ap.add_argument("--take-repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indels.json"))
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of off and on on one context")
    ap.add_argument("--out-dir", default="/dev/shm")
    ap.add_argument("--child", choices=["passes", "e2e"])
    a = ap.parse_args()
    if a.child:
        return child(a) if a.child == "passes" else e2e_child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "passes", "--pairs", str(a.pairs), "--species", str(a.species), "--strains",
                        str(a.strains), "--genome-len", str(a.genome_len), "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--accumulate",
                        str(a.accumulate), "--take-repeats", str(a.take_repeats)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    out = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    out["warmup"], out["repeats"], out["take_repeats"] = a.warmup, a.repeats, a.take_repeats
    if a.e2e:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "e2e", "--pairs", str(a.pairs), "--species", str(a.species), "--strains",
                            str(a.strains), "--genome-len", str(a.genome_len), "--steps", str(a.steps), "--rounds", str(a.rounds), "--out-dir", a.out_dir],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0 or "RESULT " not in r.stdout:
            sys.exit("the end-to-end step failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        out["end_to_end_step_on_against_off"] = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
