"""The SAM file as BGZF on a configs[1] batch (1 M pairs x 150 bp against 250 x 5 genomes of 4 Mb): the batch loop
(kslam_stream_classify, through bench_legs.e2e_leg) plain, with kslam_set_sam_bgzf, and with kslam_set_sam_bgzf under
kslam_set_bgzf_deflate(KSLAM_BGZF_DEFLATE_DYNAMIC), alternating on one box.

    python tools/bgzf_probe.py [--steps 10] [--rounds 2] [--out-dir /dev/shm]

One JSON line: SAM bytes per batch plain and compressed, the ratios (fixed, and "ratio_dynamic"), the writer thread's write()
ms per batch and the classified ms per step of every mode; the dynamic mode's figures belong in profiles/bgzf_dynamic.json.
The compressor's kernel time comes from a run of its own (--only bgzf, or --only dynamic):

    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o bgzf -- python tools/bgzf_probe.py --steps 3 --rounds 1 --only bgzf
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from bench_legs import FastqFiles, e2e_leg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="plain / BGZF / dynamic alternations")
    ap.add_argument("--only", choices=["all", "both", "plain", "bgzf", "dynamic"], default="all")
    ap.add_argument("--out-dir", default="/dev/shm")
    args = ap.parse_args()
    K = entry.load_package()
    W = importlib.import_module("kslam_amd.workload")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    Z = importlib.import_module("kslam_amd.bgzf")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, 250, 5, 4_000_000)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, 1_000_000, read_len=150)
    ctx = K.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    tax_text, entry_tax = W.taxonomy(250, 5)
    import numpy as np
    index_view = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(K, dev, [reads], 150)
    del reads
    torch.cuda.empty_cache()
    taxdb = X.TaxDB(tax_text)
    modes = {"all": ["plain", "bgzf", "dynamic"], "both": ["plain", "bgzf"], "plain": ["plain"], "bgzf": ["bgzf"], "dynamic": ["dynamic"]}[args.only]
    runs = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            Z.set_sam_bgzf(ctx, m != "plain")
            Z.set_deflate(ctx, Z.DEFLATE_DYNAMIC if m == "dynamic" else Z.DEFLATE_FIXED)
            runs[m].append(e2e_leg(K, ctx, files, 1_000_000, index_view, taxdb, args.steps, args.warmup, False, reps=1, tag=m,
                                   out_dir=args.out_dir))
    Z.set_sam_bgzf(ctx, False)
    Z.set_deflate(ctx, Z.DEFLATE_FIXED)
    out = {m: {"ms_per_step": [r["ms_per_step"] for r in rs], "sam_mb_per_batch": rs[-1]["sam_mb_per_batch"],
               "sam_file_bytes": rs[-1]["verified"]["sam_file_bytes"],
               "writer_ms_in_write_per_batch": [r["host_ms_per_batch"]["writer_thread_in_write"] for r in rs]} for m, rs in runs.items()}
    if "plain" in out and "bgzf" in out:
        out["ratio"] = round(out["plain"]["sam_file_bytes"] / out["bgzf"]["sam_file_bytes"], 3)
    if "plain" in out and "dynamic" in out:
        out["ratio_dynamic"] = round(out["plain"]["sam_file_bytes"] / out["dynamic"]["sam_file_bytes"], 3)
    print(json.dumps(out))
    files.close()
    ctx.close()


if __name__ == "__main__":
    main()
