#!/usr/bin/env python3
"""Rate of the read QC report's count pass (include/kslam_readqc.h, csrc/readqc.hip) on one batch shaped like BASELINE
configs[1]: 1 M pairs x 2 x 150 bases, the columns of the FASTQ text tools/readsplit_bench.py makes (15 quality values, most of
them one), through kslam_read_qc_add.

Prints, and writes to profiles/readqc.json:
  count_ms     the device time of the count pass (HIP events around its launches, kslam_read_qc_kernel_ms), warm-up + repeats
               passes after a reset each, and the bases + quality bytes it read per millisecond;
  one_quality  the same pass on the same bases with every quality byte 'F': every lane of every wave adds to one column, the
               contention case;
  reads_split  the yardstick for a streaming pass over the same text, in the same run: the reads split's flag, length, scan and
               copy kernels on the batch's FASTQ text (kslam_reads_out_kernel_ms) and the bytes it read plus wrote per millisecond;
  e2e          with --e2e: the step time of the batch loop (kslam_stream_classify on a synthetic database, bench.py's e2e leg)
               with kslam_set_read_qc off and on, alternating on one context, and the share the hook adds.
The tables of the first pass are checked against numpy sums over the columns.  The GPU step runs in a child process under a time
limit of its own; a run that finds no GPU fails.

    python tools/readqc_bench.py [--pairs 1000000] [--warmup 2] [--repeats 5] [--e2e] [--species 250] [--steps 4] [--rounds 3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(a):
    if a.e2e:   # torch carries its own copy of the HIP runtime and has to open the GPU before the library does
        import torch
        torch.cuda.init()
    from __graft_entry__ import load_package
    from readsplit_bench import fastq_text
    K = load_package()
    RQ = importlib.import_module("kslam_amd.readqc")
    RS = importlib.import_module("kslam_amd.readsplit")
    L, pairs = 150, a.pairs
    recs = [fastq_text(pairs, 1, 11), fastq_text(pairs, 2, 12)]
    bases = np.concatenate([r[:, 12:12 + L] for r in recs]).reshape(-1)
    quality = np.concatenate([r[:, 15 + L:15 + 2 * L] for r in recs]).reshape(-1)
    off = np.arange(2 * pairs + 1, dtype=np.uint64) * np.uint64(L)
    ctx = K.Context()
    RQ.set_read_qc(ctx, True)

    def passes(qual):
        ms = []
        for it in range(a.warmup + a.repeats):
            RQ.reset(ctx)
            RQ.add_columns(ctx, bases, off, qual, paired=True)
            if it >= a.warmup:
                ms.append(RQ.kernel_ms(ctx)[0])
        return ms, RQ.kernel_ms(ctx)[1]

    count_ms, n_bytes = passes(quality)
    t = RQ.take(ctx)
    # the tables against the columns: per stream the reads, the bases, row 0's base counts and the quality column sums
    for z in range(2):
        s = t["streams"][z]
        b = bases.reshape(2 * pairs, L)[z * pairs:(z + 1) * pairs]
        q = quality.reshape(2 * pairs, L)[z * pairs:(z + 1) * pairs]
        row0 = [int((b[:, 0] == ord(c)).sum()) for c in "ACGT"] + [0, 0]
        qual = np.array(s["qual"], dtype=np.int64).reshape(-1, 95)
        want = np.bincount(q.reshape(-1).astype(np.int64) - 33, minlength=95)
        if (s["n_reads"], s["n_bases"], s["min_len"], s["max_len"]) != (pairs, pairs * L, L, L) or s["base"][:6] != row0 or \
                qual.sum(axis=0).tolist() != want.tolist() or qual[L:].any() or s["len_hist"][L] != pairs:
            sys.exit("the tables differ from numpy's sums over the columns (stream %d)" % z)
    one_ms, _ = passes(np.full_like(quality, ord("F")))
    RQ.set_read_qc(ctx, False)
    # the yardstick: the reads split of the same batch's text, every second pair classified
    r1, r2 = recs[0].tobytes(), recs[1].tobytes()
    sel = np.arange(0, pairs, 2)
    rp = np.zeros(len(sel), dtype=K.READ_PAIR_DT)
    rp["r1_read"], rp["r2_read"], rp["count"] = sel, sel + pairs, 1
    split_ms, moved = [], 0
    for it in range(a.warmup + a.repeats):
        RS.split_reads_text(ctx, r1, r2, rp, 3)
        ms, moved = RS.kernel_ms(ctx)
        if it >= a.warmup:
            split_ms.append(ms)
    ctx.close()
    out = {"pairs": pairs, "read_len": L, "bytes_read": n_bytes, "count_ms_all": count_ms, "one_quality_ms_all": one_ms,
           "reads_split_ms_all": split_ms, "reads_split_bytes_read_plus_written": moved, "text_bytes": len(r1) + len(r2)}
    del recs, r1, r2, bases, quality
    if a.e2e:
        out["e2e"] = e2e(a, K, RQ)
    print("RESULT " + json.dumps(out))


def e2e(a, K, RQ):
    import torch
    from bench_legs import FastqFiles, e2e_leg
    W, T, X = [importlib.import_module("kslam_amd." + m) for m in ("workload", "tail", "taxonomy")]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, 5, a.genome_len)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150)
    ctx = K.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    tax_text, entry_tax = W.taxonomy(a.species, 5)
    index_view = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(K, dev, [reads], 150)
    del reads
    torch.cuda.empty_cache()
    taxdb = X.TaxDB(tax_text)
    o = {"ms_per_step_off": [], "ms_per_step_on": []}
    for _ in range(a.rounds):
        for on in (False, True):
            RQ.set_read_qc(ctx, on)
            leg = e2e_leg(K, ctx, files, a.pairs, index_view, taxdb, a.steps, 2, False, reps=1, tag="qc" if on else "plain", out_dir=a.out_dir)
            o["ms_per_step_on" if on else "ms_per_step_off"].append(leg["ms_per_step"])
    reads_counted = RQ.take(ctx)["streams"][0]["n_reads"]
    RQ.set_read_qc(ctx, False)
    files.close()
    ctx.close()
    off, on = float(np.median(o["ms_per_step_off"])), float(np.median(o["ms_per_step_on"]))
    o.update(steps=a.steps, rounds=a.rounds, species=a.species, genome_len=a.genome_len, ms_per_step_off_median=off, ms_per_step_on_median=on,
             share_added=(on - off) / off if off else None, r1_reads_counted_last_leg=reads_counted)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--genome-len", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of off and on on one context")
    ap.add_argument("--out-dir", default="/dev/shm")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readqc.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(a.pairs), "--warmup", str(a.warmup), "--repeats", str(a.repeats),
            "--species", str(a.species), "--genome-len", str(a.genome_len), "--steps", str(a.steps), "--rounds", str(a.rounds), "--out-dir", a.out_dir]
    r = subprocess.run(argv + (["--e2e"] if a.e2e else []), capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    med = lambda v: float(np.median(v))   # noqa: E731
    out = dict(res, warmup=a.warmup, repeats=a.repeats, count_ms_median=med(res["count_ms_all"]), one_quality_ms_median=med(res["one_quality_ms_all"]),
               reads_split_ms_median=med(res["reads_split_ms_all"]))
    out["count_bytes_per_ms"] = res["bytes_read"] / out["count_ms_median"]
    out["one_quality_bytes_per_ms"] = res["bytes_read"] / out["one_quality_ms_median"]
    out["reads_split_bytes_per_ms_read_plus_written"] = res["reads_split_bytes_read_plus_written"] / out["reads_split_ms_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
