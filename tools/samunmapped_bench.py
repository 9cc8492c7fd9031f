#!/usr/bin/env python3
"""Rate of the rows for the reads without alignment (include/kslam_samunmapped.h, csrc/samunmapped.hip) on batches shaped like
BASELINE configs[1]: 1 M pairs x 2 x 150 bases against 250 x 5 genomes of 4 Mb, through the batch loop (kslam_stream_classify)
with kslam_set_sam_seq on, as text and as BAM.

Prints, and writes to profiles/samunmapped.json, per mode: the device time of the new kernels on the last batch of each run (HIP
events around the flag, length, scan and write launches, kslam_sam_unmapped_kernel_ms), the bytes of the new rows and their
number, bytes per millisecond, and the step time with the switch off and on.  --unaligned sets the share of the pairs that
are from no genome of the database (configs[1] itself: 0.02; a metagenomic sample: 0.5).  The yardstick is the existing
writer in the same run, k_sam_write<.., SEQ>'s bytes per millisecond: its time comes from a kernel trace of this tool,

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o samunmapped -- python tools/samunmapped_bench.py --child ...

and its bytes are this tool's sam_mb_per_batch with the switch off.  The GPU step runs in a child process under a time limit
of its own; a run that finds no GPU fails.

    python tools/samunmapped_bench.py [--pairs 1000000] [--species 250] [--steps 4] [--rounds 3] [--unaligned 0.5] [--only text|bam]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import torch
    import __graft_entry__ as entry
    from bench_legs import FastqFiles, e2e_leg
    K = entry.load_package()
    W, T, X, M, Q, U = [importlib.import_module("kslam_amd." + m) for m in ("workload", "tail", "taxonomy", "bam", "samseq", "samunmapped")]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, 5, a.genome_len)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150, unmapped=a.unaligned)
    ctx = K.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    tax_text, entry_tax = W.taxonomy(a.species, 5)
    index_view = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(K, dev, [reads], 150)
    del reads
    torch.cuda.empty_cache()
    taxdb = X.TaxDB(tax_text)
    out = {}
    Q.set_sam_seq(ctx, True)
    for _ in range(a.rounds):
        for kind in (["text", "bam"] if a.only == "both" else [a.only]):
            M.set_sam_bam(ctx, kind == "bam")
            legs = {}
            for on in (False, True):
                U.set_sam_unmapped(ctx, on)
                legs[on] = e2e_leg(K, ctx, files, a.pairs, index_view, taxdb, a.steps, 2, False, reps=1,
                                   tag=kind + ("+unmapped" if on else ""), out_dir=a.out_dir)
            ms, n_bytes, n_rows = U.kernel_ms(ctx)
            o = out.setdefault(kind, {"kernel_ms_last_batch": [], "ms_per_step_off": [], "ms_per_step_on": []})
            o["kernel_ms_last_batch"].append(round(ms, 4))
            o["ms_per_step_off"].append(legs[False]["ms_per_step"])
            o["ms_per_step_on"].append(legs[True]["ms_per_step"])
            o.update(bytes_written=n_bytes, rows=n_rows, sam_mb_per_batch_off=legs[False]["sam_mb_per_batch"],
                     sam_mb_per_batch_on=legs[True]["sam_mb_per_batch"])
    for o in out.values():
        ms = sorted(o["kernel_ms_last_batch"])[len(o["kernel_ms_last_batch"]) // 2]
        o["bytes_per_ms_median"] = round(o["bytes_written"] / ms) if ms else None
    U.set_sam_unmapped(ctx, False)
    M.set_sam_bam(ctx, False)
    Q.set_sam_seq(ctx, False)
    files.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--genome-len", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--unaligned", type=float, default=0.5)
    ap.add_argument("--only", choices=["both", "text", "bam"], default="both")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the modes on one context")
    ap.add_argument("--out-dir", default="/dev/shm")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samunmapped.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(a.pairs), "--species", str(a.species), "--genome-len",
            str(a.genome_len), "--steps", str(a.steps), "--unaligned", str(a.unaligned), "--only", a.only, "--out-dir", a.out_dir, "--rounds", str(a.rounds)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    out = {"pairs": a.pairs, "species": a.species, "genome_len": a.genome_len, "steps": a.steps, "unaligned_share": a.unaligned, "rounds": a.rounds, "modes": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
