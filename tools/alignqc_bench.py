#!/usr/bin/env python3
"""Rate of the alignment QC report's count pass (include/kslam_alignqc.h, csrc/alignqc.hip) on one batch shaped like BASELINE
configs[1]: 1 M pairs x 2 x 150 bases against the synthetic species x strains database of bench.py, aligned and paired by the
library itself; the batch's overlap records, CIGAR pool, reads, quality column, read pairs and alignment pairs then go through
kslam_align_qc_add.

Per shape 2 warm-up and 5 timed count passes (kslam_align_qc_kernel_ms: HIP events around the count pass alone) after a reset
each, with the product kernel (a wavefront per record) and with the kept one-thread-per-record instantiation
(KSLAM_ALIGNQC_WALK=thread); the two must give the same tables.  Shapes: reads made with 0 %, 1 % and 10 % substitutions (the
rate the tables report is recorded with each: the strains differ from their species' root besides), each with one quality value
for every base and with qualities spread over eight values.  The yardsticks, in the same process on the 1 % batch: the variants'
emit passes (kslam_variants_kernel_ms) and the read QC's count pass on the same reads (kslam_read_qc_kernel_ms).
--e2e: the end-to-end step of bench.py's loop with the report off and on, alternating on one context, `rounds` legs each; the
spread of the equal legs is recorded beside the difference.
Every GPU step runs in a child process under a time limit of its own; a run that finds no GPU fails.  Writes
profiles/alignqc.json.

    python tools/alignqc_bench.py [--pairs 1000000] [--rates 0,0.01,0.1] [--e2e] [--steps 4] [--rounds 3]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import torch
    from __graft_entry__ import load_package
    K = load_package()
    W = importlib.import_module("kslam_amd.workload")
    VR = importlib.import_module("kslam_amd.variants")
    RQ = importlib.import_module("kslam_amd.readqc")
    AQ = importlib.import_module("kslam_amd.alignqc")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, a.strains, a.genome_len)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150, sub_rate=a.rate)
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
    rng = np.random.default_rng(3)
    quals = {"one_quality": np.full(len(rbases), ord("F"), dtype=np.uint8),
             "spread_qualities": rng.choice(np.array([35, 44, 50, 55, 58, 65, 70, 73], dtype=np.uint8), len(rbases))}
    ctx.set_pairing(stages=3)
    AQ.set_align_qc(ctx, True)
    out = {"rate_asked": a.rate, "pairs": a.pairs, "overlap_records": len(ov), "read_pairs": len(rp), "alignment_pairs": len(pr), "cigar_ops": len(cg)}
    for name, q in quals.items():
        tables = {}
        for walk in ("wave", "thread"):
            if walk == "thread":
                os.environ["KSLAM_ALIGNQC_WALK"] = "thread"
            ms = []
            try:
                for it in range(a.warmup + a.repeats):
                    AQ.reset(ctx)
                    AQ.add(ctx, ov, cg, rbases, roff, rp, pr, q, True)
                    if it >= a.warmup:
                        ms.append(AQ.kernel_ms(ctx))
            finally:
                os.environ.pop("KSLAM_ALIGNQC_WALK", None)
            tables[walk] = AQ.take(ctx)
            out["%s_%s_ms_all" % (name, walk)] = ms
            out["%s_%s_ms_median" % (name, walk)] = float(np.median(ms))
        if tables["wave"] != tables["thread"]:
            sys.exit("the two instantiations of the walk give different tables (%s)" % name)
        t = tables["wave"]
        s = [t["streams"][z] for z in range(2)]
        compared, miss = s[0]["compared"] + s[1]["compared"], s[0]["mismatches"] + s[1]["mismatches"]
        # the tables against numpy sums over the arrays
        live = np.repeat(rp["first"].astype(np.int64) - np.concatenate([[0], np.cumsum(rp["count"].astype(np.int64))[:-1]]), rp["count"].astype(np.int64)) + \
            np.arange(int(rp["count"].sum()))
        named = np.unique(np.concatenate([pr["r1"][live], pr["r2"][live]]))
        named = named[named != 0xFFFFFFFF]
        both = (pr["r1"][live] != 0xFFFFFFFF) & (pr["r2"][live] != 0xFFFFFFFF)
        if s[0]["n_records"] + s[1]["n_records"] != len(named) or t["pairs_both"] != int(both.sum()) or \
                t["insert_sum"] != int(pr["insert_size"][live][both].astype(np.int64).sum()) or sum(s[0]["cq_compared"]) != s[0]["compared"] or \
                sum(s[0]["subst"]) != s[0]["compared"] or t["n_read_pairs"] != int((rp["count"] > 0).sum()):
            sys.exit("the tables differ from the arrays' sums")
        out.update(records=len(named), compared=compared, mismatches=miss, mismatch_rate=miss / compared if compared else 0.0,
                   ins_events=s[0]["ins_events"] + s[1]["ins_events"], del_events=s[0]["del_events"] + s[1]["del_events"],
                   skipped=s[0]["n_skipped"] + s[1]["n_skipped"])
    AQ.set_align_qc(ctx, False)
    if a.yardsticks:
        VR.set_variants(ctx, True)
        emits = []
        for it in range(a.warmup + a.repeats):
            VR.reset(ctx)
            VR.add(ctx, ov, cg, rbases, roff, rp, pr)
            if it >= a.warmup:
                emits.append(VR.kernel_ms(ctx)[0])
        VR.set_variants(ctx, False)
        RQ.set_read_qc(ctx, True)
        counts = []
        for it in range(a.warmup + a.repeats):
            RQ.reset(ctx)
            RQ.add_columns(ctx, rbases, roff, quals["spread_qualities"], paired=True)
            if it >= a.warmup:
                counts.append(RQ.kernel_ms(ctx)[0])
        RQ.set_read_qc(ctx, False)
        out.update(variants_emit_ms_all=emits, variants_emit_ms_median=float(np.median(emits)), read_qc_count_ms_all=counts,
                   read_qc_count_ms_median=float(np.median(counts)))
    ctx.close()
    print("RESULT " + json.dumps(out))


def e2e_child(a):
    import torch
    torch.cuda.init()   # torch carries its own copy of the HIP runtime and has to open the GPU before the library does
    from __graft_entry__ import load_package
    from bench_legs import FastqFiles, e2e_leg
    K = load_package()
    AQ = importlib.import_module("kslam_amd.alignqc")
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
    records = 0
    for _ in range(a.rounds):
        for on in (False, True):
            if on:
                ctx.set_pairing(stages=3)   # (the switch asks for it; the loop sets its own stages and takes them back)
            AQ.set_align_qc(ctx, on)
            leg = e2e_leg(K, ctx, files, a.pairs, index_view, taxdb, a.steps, 2, False, reps=1, tag="aq" if on else "plain", out_dir=a.out_dir)
            o["ms_per_step_on" if on else "ms_per_step_off"].append(leg["ms_per_step"])
            if on:
                records = AQ.take(ctx)["streams"][0]["n_records"]
    AQ.set_align_qc(ctx, False)
    files.close()
    ctx.close()
    off, on = float(np.median(o["ms_per_step_off"])), float(np.median(o["ms_per_step_on"]))
    o.update(pairs=a.pairs, steps=a.steps, rounds=a.rounds, ms_per_step_off_median=off, ms_per_step_on_median=on, difference_ms=on - off,
             spread_of_off_legs_ms=max(o["ms_per_step_off"]) - min(o["ms_per_step_off"]),
             spread_of_on_legs_ms=max(o["ms_per_step_on"]) - min(o["ms_per_step_on"]), r1_records_counted_last_leg=records)
    o["difference_within_spread_of_equal_legs"] = abs(on - off) <= max(o["spread_of_off_legs_ms"], o["spread_of_on_legs_ms"])
    print("RESULT " + json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--strains", type=int, default=5)
    ap.add_argument("--genome-len", type=int, default=4000000)
    ap.add_argument("--rates", default="0,0.01,0.1")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of off and on on one context")
    ap.add_argument("--out-dir", default="/dev/shm")
    ap.add_argument("--timeout", type=int, default=300, help="seconds, for each GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignqc.json"))
    ap.add_argument("--child", choices=["count", "e2e"])
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--yardsticks", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a) if a.child == "count" else e2e_child(a)
    common = ["--pairs", str(a.pairs), "--species", str(a.species), "--strains", str(a.strains), "--genome-len", str(a.genome_len), "--warmup",
              str(a.warmup), "--repeats", str(a.repeats), "--steps", str(a.steps), "--rounds", str(a.rounds), "--out-dir", a.out_dir]

    def step(extra):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + common + extra, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0 or "RESULT " not in r.stdout:
            sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
        return json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])

    out = {"warmup": a.warmup, "repeats": a.repeats, "shapes": []}
    slower = []
    for rate in [float(x) for x in a.rates.split(",")]:
        res = step(["--child", "count", "--rate", str(rate)] + (["--yardsticks"] if rate == 0.01 else []))
        out["shapes"].append(res)
        for name in ("one_quality", "spread_qualities"):
            if res[name + "_wave_ms_median"] > res[name + "_thread_ms_median"]:
                slower.append("%s at %g" % (name, rate))
    out["wave_slower_than_thread_on"] = slower
    out["end_to_end_step_on_against_off"] = step(["--child", "e2e"]) if a.e2e else "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
