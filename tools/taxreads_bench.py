#!/usr/bin/env python3
"""Rate of the passes behind the reads of chosen taxa (include/kslam_taxreads.h, csrc/taxreads.hip) on one MI355X: the synthetic
tree and the id shapes of tools/kreport_bench.py (--nodes nodes; --ids ids, "uniform" over --taxa taxa and "skewed" with 90 % on
one taxon) and the FASTQ batch of tools/readsplit_bench.py (--ids pairs x 2 x 150 bases, every pair a read pair).

Reported, each the median of --repeats after --warmup, timed by HIP events:
  mask      the mask pass of kslam_set_taxon_reads, once per mode (0 .. 7), for the chosen ids of each shape;
  flag      the flag pass (kslam_taxon_reads_kernel_ms) next to the Kraken-style report's count pass over the SAME ids in the
            same run (kslam_kreport_kernel_ms): both do one binary search per read pair;
  copy      the lengths, scans and copy next to kslam_reads_out_kernel_ms of kslam_split_reads_text for the same batch and
            the same selected records (that figure includes the split's own flag pass).
Chosen ids: "uniform" takes every second taxon (half of the pairs match), "skewed" the heavy taxon (90 %).  The selected R1
block of the first pass is checked against the records cut out on the host.  With --ablate-lib (the measurement-only
`make ABLATE=1` library) the flag pass runs twice more, without its matched-pair count (KSLAM_TAXREADS_ABLATE=1) and without its
marks on the records (=2): where its time goes.  Prints, and writes to profiles/taxreads.json.  The
GPU step runs in a child process under a time limit of its own; a run that finds no GPU fails.

    python tools/taxreads_bench.py [--ids 1000000] [--nodes 2000000] [--taxa 10000] [--warmup 2] [--repeats 5] [--ablate-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(a):
    import importlib
    from __graft_entry__ import load_package
    from kreport_bench import make_tree
    from readsplit_bench import fastq_text
    K = load_package()
    TR = importlib.import_module("kslam_amd.taxreads")
    KR = importlib.import_module("kslam_amd.kreport")
    RS = importlib.import_module("kslam_amd.readsplit")
    ST = importlib.import_module("kslam_amd.samtext")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    tax = X.TaxDB(make_tree(a.nodes))
    ctx = K.Context()
    bases, off = np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64)
    ctx.set_index_arrays(bases, off)
    index = T.IndexArrays(bases, off, taxonomy_ids=[2])
    ST.set_annotations(ctx, index, tax)
    ctx.set_pairing(stages=3)
    KR.set_kreport(ctx, True)
    rng = np.random.default_rng(3)
    taxa = (2 + rng.choice(a.nodes, a.taxa, replace=False)).astype(np.uint32)
    uniform = rng.choice(taxa, a.ids)
    skewed = uniform.copy()
    skewed[rng.random(a.ids) < 0.9] = taxa[0]
    pairs = a.ids
    recs = [fastq_text(pairs, 1, 11), fastq_text(pairs, 2, 12)]
    r1, r2 = recs[0].tobytes(), recs[1].tobytes()
    rp = np.zeros(pairs, dtype=K.READ_PAIR_DT)
    rp["r1_read"], rp["r2_read"], rp["count"] = np.arange(pairs), np.arange(pairs) + pairs, 1
    med = lambda v: float(np.median(v))   # noqa: E731
    out = {"ids": a.ids, "nodes": len(tax), "taxa": a.taxa, "text_bytes": len(r1) + len(r2), "warmup": a.warmup, "repeats": a.repeats}
    for shape, ids, chosen in (("uniform", uniform, taxa[::2].copy()), ("skewed", skewed, taxa[:1].copy())):
        res = {"chosen_ids": int(len(chosen))}
        masks = {}
        for mode in range(8):
            v = []
            for it in range(a.warmup + a.repeats):
                TR.set_taxon_reads(ctx, chosen, mode)
                if it >= a.warmup:
                    v.append(TR.kernel_ms(ctx)[0])
            masks[str(mode)] = {"mask_ms_median": med(v), "mask_ms_all": v}
        res["mask"] = masks
        TR.set_taxon_reads(ctx, chosen, 0)
        hit = np.isin(ids, chosen)
        flag, copy, count, split, moved = [], [], [], [], 0
        for it in range(a.warmup + a.repeats):
            KR.reset(ctx)
            KR.add(ctx, ids)
            got = TR.taxon_reads_text(ctx, r1, r2, rp, ids)
            if it == 0 and not os.environ.get("KSLAM_TAXREADS_ABLATE") and (zlib.crc32(got["blocks"][0]) != zlib.crc32(recs[0][hit].tobytes()) or got["n_records"][0] != int(hit.sum())):
                sys.exit("the selected block differs from the records cut out on the host (%s)" % shape)
            RS.split_reads_text(ctx, r1, r2, rp[hit], 1)
            if it >= a.warmup:
                _, f, c, moved = TR.kernel_ms(ctx)
                flag.append(f)
                copy.append(c)
                count.append(KR.kernel_ms(ctx)[0])
                split.append(RS.kernel_ms(ctx)[0])
        res.update({"selected_share": float(hit.mean()), "flag_ms_median": med(flag), "flag_ms_all": flag, "kreport_count_ms_median": med(count),
                    "kreport_count_ms_all": count, "copy_ms_median": med(copy), "copy_ms_all": copy, "bytes_read_plus_written": moved,
                    "copy_GBps_read_plus_written": moved / med(copy) / 1e6, "reads_out_kernel_ms_median": med(split), "reads_out_kernel_ms_all": split})
        out[shape] = res
    TR.set_taxon_reads(ctx, [], 0)
    KR.set_kreport(ctx, False)
    ctx.close()
    print("RESULT " + json.dumps(out))


def run_child(a, env_extra):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ids", str(a.ids), "--nodes", str(a.nodes), "--taxa", str(a.taxa),
                        "--warmup", str(a.warmup), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.timeout,
                       env=dict(os.environ, **env_extra))
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=1000000)
    ap.add_argument("--nodes", type=int, default=2000000)
    ap.add_argument("--taxa", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--ablate-lib", default=None, help="libkslam_hip_ablate.so (make -C k-slam_amd/csrc ABLATE=1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taxreads.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = run_child(a, {})
    if a.ablate_lib:
        if not os.path.exists(a.ablate_lib):
            sys.exit(a.ablate_lib + " is missing: make -C k-slam_amd/csrc ABLATE=1")
        for variant, name in (("1", "flag_ms_without_count"), ("2", "flag_ms_without_marks")):
            ab = run_child(a, {"KSLAM_LIB": os.path.abspath(a.ablate_lib), "KSLAM_TAXREADS_ABLATE": variant})
            for shape in ("uniform", "skewed"):
                out[shape][name + "_median"] = ab[shape]["flag_ms_median"]
                out[shape][name + "_all"] = ab[shape]["flag_ms_all"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
