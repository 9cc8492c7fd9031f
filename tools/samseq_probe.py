"""SEQ and QUAL in the SAM file (include/kslam_samseq.h) on a configs[1] batch (1 M pairs x 150 bp against 250 x 5 genomes
of 4 Mb): the batch loop (kslam_stream_classify, through bench_legs.e2e_leg) plain, with kslam_set_sam_bgzf and with
kslam_set_sam_bam, each with kslam_set_sam_seq off and on, alternating on one box.

    python tools/samseq_probe.py [--steps 10] [--rounds 2] [--seq both] [--out-dir /dev/shm]

One JSON line, per mode ("plain", "plain+seq", ...): the bytes before compression and the bytes written per batch, the writer
thread's write() ms and the classified ms per step.  The kernels' times come from a run of their own:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o samseq -- python tools/samseq_probe.py --steps 3 --rounds 1
"""
import argparse
import importlib
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from bench_legs import FastqFiles, e2e_leg  # noqa: E402


def bgzf_isize(path):
    """the uncompressed bytes of a BGZF file, from its members' trailers (nothing inflated)"""
    total = 0
    with open(path, "rb") as f:
        data = f.read()
    pos = 0
    while pos < len(data):
        bsize = struct.unpack_from("<H", data, pos + 16)[0] + 1
        total += struct.unpack_from("<I", data, pos + bsize - 4)[0]
        pos += bsize
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="plain / BGZF / BAM alternations")
    ap.add_argument("--only", choices=["all", "plain", "bgzf", "bam"], default="all")
    ap.add_argument("--seq", choices=["both", "off", "on"], default="both")
    ap.add_argument("--out-dir", default="/dev/shm")
    args = ap.parse_args()
    K = entry.load_package()
    W = importlib.import_module("kslam_amd.workload")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    Z = importlib.import_module("kslam_amd.bgzf")
    M = importlib.import_module("kslam_amd.bam")
    Q = importlib.import_module("kslam_amd.samseq")
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
    header_len = len(M.header(index_view, T.sam_header(index_view, b"SLAM --db synthetic R1.fq R2.fq")))
    kinds = ["plain", "bgzf", "bam"] if args.only == "all" else [args.only]
    modes = [k + s for k in kinds for s in {"both": ["", "+seq"], "off": [""], "on": ["+seq"]}[args.seq]]
    runs = {m: [] for m in modes}
    raw = {}
    for _ in range(args.rounds):
        for m in modes:
            kind = m.split("+")[0]
            Z.set_sam_bgzf(ctx, kind == "bgzf")
            M.set_sam_bam(ctx, kind == "bam")
            Q.set_sam_seq(ctx, m.endswith("+seq"))

            def dump(res, sam_path, _pr, m=m, kind=kind):
                if kind != "plain":   # the bytes before compression, from the members' trailers
                    raw[m] = (bgzf_isize(sam_path), res["n_batches"])
            runs[m].append(e2e_leg(K, ctx, files, 1_000_000, index_view, taxdb, args.steps, args.warmup, False, reps=1, tag=m,
                                   out_dir=args.out_dir, dump=dump))
    Z.set_sam_bgzf(ctx, False)
    M.set_sam_bam(ctx, False)
    Q.set_sam_seq(ctx, False)
    # file_mb_per_batch: plain = the SAM text, bgzf = its members, bam = the members of the BAM records (raw_mb_per_batch)
    out = {m: {"ms_per_step": [r["ms_per_step"] for r in rs], "file_mb_per_batch": rs[-1]["sam_mb_per_batch"],
               "sam_file_bytes": rs[-1]["verified"]["sam_file_bytes"],
               "writer_ms_in_write_per_batch": [r["host_ms_per_batch"]["writer_thread_in_write"] for r in rs]} for m, rs in runs.items()}
    for m, (isize, n_batches) in raw.items():   # (the header: BAM's is header_len, the text's a few hundred kB less)
        out[m]["raw_mb_per_batch"] = round((isize - (header_len if m.startswith("bam") else 0)) / n_batches / 1e6, 1)
    print(json.dumps(out))
    files.close()
    ctx.close()


if __name__ == "__main__":
    main()
