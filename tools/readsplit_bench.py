#!/usr/bin/env python3
"""Rate of the reads split (include/kslam_readsplit.h, csrc/readsplit.hip) on one batch shaped like BASELINE configs[1]:
1 M pairs x 2 x 150 bases of LF-terminated FASTQ, every second pair classified.

Prints, and writes to profiles/readsplit.json: the device time of the flag, length, scan and copy kernels (HIP events around
their launches, kslam_reads_out_kernel_ms), the text bytes the copy read plus wrote per second of that time, and the time of
the whole call (upload, index, split, the four blocks' way back to page-locked host memory).  Hold the GB/s figure against
what tools/copy_peak.hip sustains on the same box in the same visit (--copy-peak-gbps adds the ratio).  The GPU step runs in
a child process under a time limit of its own; a run that finds no GPU fails.

    python tools/readsplit_bench.py [--pairs 1000000] [--warmup 2] [--repeats 5] [--copy-peak-gbps X]
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


def fastq_text(rows, mate, seed, L=150):
    rnd = np.random.default_rng(seed)
    rec = np.empty((rows, 16 + 2 * L), dtype=np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(rows)
    for d in range(8):
        rec[:, 8 - d] = ord("0") + (idx // 10 ** d) % 10
    rec[:, 9] = ord("/")
    rec[:, 10] = ord("0") + mate
    rec[:, 11] = ord("\n")
    rec[:, 12:12 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rnd.integers(0, 4, (rows, L))]
    rec[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 15 + L:15 + 2 * L] = np.frombuffer(b"FFFFFFFFFFFF:,#", dtype=np.uint8)[rnd.integers(0, 15, (rows, L))]
    rec[:, 15 + 2 * L] = ord("\n")
    return rec


def child(pairs, warmup, repeats):
    import importlib
    from __graft_entry__ import load_package
    K = load_package()
    RS = importlib.import_module("kslam_amd.readsplit")
    recs = [fastq_text(pairs, 1, 11), fastq_text(pairs, 2, 12)]
    r1, r2 = recs[0].tobytes(), recs[1].tobytes()
    sel = np.arange(0, pairs, 2)
    rp = np.zeros(len(sel), dtype=K.READ_PAIR_DT)
    rp["r1_read"], rp["r2_read"], rp["count"] = sel, sel + pairs, 1
    expect = [zlib.crc32(recs[k % 2][(0 if k < 2 else 1)::2].tobytes()) for k in range(4)]
    ctx = K.Context()
    calls, kernels, moved = [], [], 0
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        out = RS.split_reads_text(ctx, r1, r2, rp, 3)
        dt = time.perf_counter() - t0
        if it == 0 and [zlib.crc32(b) for b in out["blocks"]] != expect:
            sys.exit("the blocks differ from the records cut out on the host")
        ms, moved = RS.kernel_ms(ctx)
        if it >= warmup:
            calls.append(dt * 1e3)
            kernels.append(ms)
    ctx.close()
    print("RESULT " + json.dumps({"pairs": pairs, "text_bytes": len(r1) + len(r2), "bytes_moved": moved, "call_ms": calls, "kernel_ms": kernels}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--copy-peak-gbps", type=float, default=None)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readsplit.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.pairs, a.warmup, a.repeats)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(a.pairs), "--warmup", str(a.warmup),
                        "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    kern, call = float(np.median(res["kernel_ms"])), float(np.median(res["call_ms"]))
    out = {"pairs": res["pairs"], "text_bytes": res["text_bytes"], "bytes_read_plus_written": res["bytes_moved"],
           "kernel_ms_median": kern, "kernel_ms_all": res["kernel_ms"], "kernel_GBps_read_plus_written": res["bytes_moved"] / kern / 1e6,
           "call_ms_median": call, "call_ms_all": res["call_ms"], "warmup": a.warmup, "repeats": a.repeats}
    if a.copy_peak_gbps:
        out["copy_peak_GBps"] = a.copy_peak_gbps
        out["fraction_of_copy_peak"] = out["kernel_GBps_read_plus_written"] / a.copy_peak_gbps
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
