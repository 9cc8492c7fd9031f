#!/usr/bin/env python3
"""Rates of the coordinate-sorted BAM (include/kslam_bamsort.h, csrc/bamsort.hip) on the records of one batch shaped like BASELINE
configs[1]: 1 M pairs x 2 x 150 bases against the synthetic species x strains database of bench.py, classified by the batch loop
itself with the plain BAM route; the unsorted file's records, inflated on the host, are the batch.

Append: the batch goes in --batches times through kslam_bam_sort_add (the upload from pageable memory, the record index's count,
scan and write passes; HIP events and wall time per batch), beside the wall time of kslam_bgzf_compress over the same bytes -- the
upload, the compression and the copy back of the plain route that the held route leaves out.  A lane's own append copies device
to device instead of uploading; it is not timed apart here.
Take: --repeats takes per gather form (16 lanes per record, 64, and the one-thread-per-record baseline), each split by
kslam_bam_sort_kernel_ms into sort, gather, compress and index, in ms and in ms per GB of records; the gather's bytes (read +
written) per ms beside the streaming copy of tools/copy_peak.hip when --copy-peak names its binary, run on the same box.
--e2e: the batch loop's step with the sorted file against the plain BAM file, legs alternating on one context; the spread of the
equal legs is recorded beside the difference.  Bytes of device memory held per batch.  Writes profiles/bamsort.json.

    python tools/bamsort_bench.py [--pairs 1000000] [--species 250] [--strains 5] [--genome-len 4000000] [--batches 8] [--repeats 3]
                                  [--e2e] [--steps 4] [--rounds 3] [--copy-peak build_tools/copy_peak]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inflate_members(blob):
    out, rest = [], blob
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        rest = d.unused_data
    return b"".join(out)


def child(a):
    import importlib
    import torch
    torch.cuda.init()   # torch carries its own copy of the HIP runtime and has to open the GPU before the library does
    from __graft_entry__ import load_package
    from bench_legs import FastqFiles
    K = load_package()
    W, T, S, BS, Z, M = [importlib.import_module("kslam_amd." + m) for m in ("workload", "tail", "stream", "bamsort", "bgzf", "bam")]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    db, offs = W.make_database(dev, gen, a.species, a.strains, a.genome_len)
    gen.manual_seed(2)
    reads = W.make_reads(dev, gen, db, offs, a.pairs, read_len=150)
    ctx = K.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    _, entry_tax = W.taxonomy(a.species, a.strains)
    index = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(K, dev, [reads], 150)
    del reads
    torch.cuda.empty_cache()
    header = T.sam_header(index, b"SLAM --db synthetic R1.fq R2.fq")
    P = T.TailParams.default()
    tmp = os.path.join(a.out_dir, "bamsort_bench.bam")

    def loop(sorted_file, passes=1):
        fd = os.open(tmp, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
        idx = os.open(tmp + ".bai", os.O_RDWR | os.O_CREAT | os.O_TRUNC)
        try:
            t0 = time.perf_counter()
            st = S.classify_stream_native(ctx, index, files.h[0].ptr, files.len, files.h[1].ptr, files.len, a.pairs, P, sam_fd=fd, sam_header=header,
                                          passes=passes, sam_sorted=sorted_file, sam_index_fd=idx if sorted_file else None)
            return (time.perf_counter() - t0) * 1e3, st
        finally:
            os.close(fd)
            os.close(idx)

    out = {"pairs": a.pairs, "entries": len(offs) - 1, "database_bases": int(offs[-1])}
    M.set_sam_bam(ctx, True)
    loop(False)
    blob = open(tmp, "rb").read()
    head_len = len(M.header(index, header))
    records = inflate_members(blob)[head_len:]
    del blob
    out["record_bytes_per_batch"] = len(records)
    # ---- append
    BS.set_bam_sort(ctx, True)
    add_ms, add_wall, plain_wall = [], [], []
    for k in range(a.batches):
        t0 = time.perf_counter()
        BS.add(ctx, k, records)
        add_wall.append((time.perf_counter() - t0) * 1e3)
        add_ms.append(BS.kernel_ms(ctx)["append"])
    for _ in range(3):
        t0 = time.perf_counter()
        z = Z.compress(ctx, records)
        plain_wall.append((time.perf_counter() - t0) * 1e3)
    out.update({"batches_held": a.batches, "add_event_ms_all": add_ms, "add_event_ms_median": float(np.median(add_ms[1:])),
                "add_wall_ms_all": add_wall, "add_wall_ms_median": float(np.median(add_wall[1:])),
                "plain_route_upload_compress_fetch_wall_ms_all": plain_wall, "plain_route_upload_compress_fetch_wall_ms_median": float(np.median(plain_wall)),
                "compressed_bytes_per_batch": len(z)})
    del z
    # ---- take
    sink = BS.take_fd
    takes = {}
    stats = None
    for lanes in (16, 64, 1):
        BS.set_gather(ctx, lanes)
        rows = []
        for _ in range(a.repeats + 1):
            fd = os.open(tmp, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
            idx = os.open(tmp + ".bai", os.O_RDWR | os.O_CREAT | os.O_TRUNC)
            try:
                t0 = time.perf_counter()
                stats = sink(ctx, header, fd, idx)
                wall = (time.perf_counter() - t0) * 1e3
            finally:
                os.close(fd)
                os.close(idx)
            ms = BS.kernel_ms(ctx)
            ms["wall"] = wall
            rows.append(ms)
        rows = rows[1:]   # (the first take sizes its buffers)
        gb = stats["record_bytes"] / 1e9
        med = {k: float(np.median([r[k] for r in rows])) for k in ("sort", "gather", "compress", "index", "wall")}
        takes[str(lanes)] = {"all": rows, "median_ms": med, "median_ms_per_GB": {k: v / gb for k, v in med.items()},
                             "gather_min_max_ms": [min(r["gather"] for r in rows), max(r["gather"] for r in rows)],
                             "gather_bytes_read_and_written_per_ms": 2 * stats["record_bytes"] / med["gather"],
                             "gather_TB_per_s": 2 * stats["record_bytes"] / med["gather"] / 1e9}
    BS.set_gather(ctx, 0)
    out["take"] = takes
    out["take_stats"] = stats
    out["bytes_held_per_batch"] = stats["bytes_held"] / a.batches
    out["gather_16_over_one_thread_per_record"] = takes["1"]["median_ms"]["gather"] / takes["16"]["median_ms"]["gather"]
    BS.set_bam_sort(ctx, False)
    del records
    # ---- the batch loop's step, sorted against plain BAM, alternating
    if a.e2e:
        legs = {"plain_bam": [], "sorted": []}
        for _ in range(a.rounds):
            for name in ("plain_bam", "sorted"):
                wall, st = loop(name == "sorted", passes=a.steps)
                legs[name].append(wall / max(st["n_batches"], 1))
        p, s = float(np.median(legs["plain_bam"])), float(np.median(legs["sorted"]))
        out["e2e"] = {"steps_per_leg": a.steps, "ms_per_step": legs, "median_plain_bam": p, "median_sorted": s, "sorted_minus_plain_ms": s - p,
                      "spread_of_equal_legs_ms": {k: max(v) - min(v) for k, v in legs.items()},
                      "note": "a sorted leg includes the take (sort, gather, compress, index and the write of the whole file) behind its last batch"}
    M.set_sam_bam(ctx, False)
    files.close()
    ctx.close()
    for f in (tmp, tmp + ".bai"):
        if os.path.exists(f):
            os.remove(f)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=250)
    ap.add_argument("--strains", type=int, default=5)
    ap.add_argument("--genome-len", type=int, default=4000000)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copy-peak", default="")
    ap.add_argument("--out-dir", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bamsort.json"))
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"], stdout=subprocess.PIPE,
                       timeout=a.timeout)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.exit("the GPU step failed (exit %d)" % r.returncode)
    out = json.loads(lines[-1][7:])
    if a.copy_peak and os.path.exists(a.copy_peak):
        cp = subprocess.run([a.copy_peak], stdout=subprocess.PIPE, timeout=120)
        rates = [float(ln.split(" ms")[1].split("TB/s")[0]) for ln in cp.stdout.decode().splitlines() if "TB/s" in ln]
        out["copy_peak_TB_per_s_best"] = max(rates) if rates else None
        if rates:
            out["gather_16_over_copy_peak"] = out["take"]["16"]["gather_TB_per_s"] / max(rates)
    else:
        out["copy_peak_TB_per_s_best"] = "not measured in this run"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in out if k not in ("take",)}, indent=1))
    for lanes, t in out["take"].items():
        print("gather with %s lanes per record: %s  %.2f TB/s" % (lanes, json.dumps(t["median_ms"]), t["gather_TB_per_s"]))


if __name__ == "__main__":
    main()
