#!/usr/bin/env python3
"""Rate of kslam_bgzf_inflate (include/kslam_inflate.h) on about one batch of FASTQ-like text, BGZF at level 6.

Prints, and writes to profiles/inflate.json: GB/s of text for the whole call (upload of the compressed bytes, kernel, the
text's way back to page-locked host memory), for the kernel alone (HIP events around each round's launch), and for ONE
CPU thread of zlib.decompress over the same members on the same box.  The GPU step runs in a child process under a time
limit of its own; a run that finds no GPU fails.

    python tools/inflate_bench.py [--mb 700] [--warmup 2] [--repeats 5] [--step-ms E2E_STEP_MS]

--step-ms: the end-to-end step time bench.py reports for a batch on the same box; the ingest stays hidden behind a batch's
compute when the whole call takes no longer than that.
"""
import argparse
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 65280


def fastq_like(n_bytes, seed):
    rnd = np.random.default_rng(seed)
    L = 150
    rows = n_bytes // (14 + 2 * L) + 1
    rec = np.empty((rows, 14 + 2 * L), dtype=np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(rows)
    for d in range(8):
        rec[:, 8 - d] = ord("0") + (idx // 10 ** d) % 10
    rec[:, 9] = ord("\n")
    rec[:, 10:10 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rnd.integers(0, 4, (rows, L))]
    rec[:, 10 + L:13 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    # qualities as a sequencer writes them: mostly the top bin, runs of lower ones
    rec[:, 13 + L:13 + 2 * L] = np.frombuffer(b"FFFFFFFFFFFF:,#", dtype=np.uint8)[rnd.integers(0, 15, (rows, L))]
    rec[:, 13 + 2 * L] = ord("\n")
    return rec.reshape(-1)[:n_bytes]


def _members(args):
    seed, n = args
    text = fastq_like(n, seed).tobytes()
    out = []
    for at in range(0, len(text), CHUNK):
        part = text[at:at + CHUNK]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(part) + c.flush()
        size = 18 + len(body) + 8
        out.append(bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", size - 1) + body +
                   struct.pack("<II", zlib.crc32(part), len(part)))
    return b"".join(out), len(text)


def build_blob(mb, workers):
    pieces = max(1, mb // 16)
    with ProcessPoolExecutor(workers) as pool:
        parts = list(pool.map(_members, [(100 + k, (mb << 20) // pieces) for k in range(pieces)]))
    return b"".join(p[0] for p in parts), sum(p[1] for p in parts)


def child(path, warmup, repeats):
    from __graft_entry__ import load_package
    K = load_package()
    Z = importlib.import_module("kslam_amd.inflate")
    blob = open(path, "rb").read()
    L = Z.lib()
    import ctypes as C
    ctx = K.Context()
    n_members, text_len = Z.scan(blob)
    calls, kernels = [], []
    crc = None
    for it in range(warmup + repeats):
        out, n = C.c_void_p(), C.c_uint64()
        t0 = time.perf_counter()
        ctx._chk(L.kslam_bgzf_inflate(ctx._h, blob, len(blob), C.byref(out), C.byref(n)))
        dt = time.perf_counter() - t0                  # the call returns after its last copy has landed
        if it == 0:
            crc = zlib.crc32(C.string_at(out.value, n.value))
        L.kslam_free_pinned(ctx._h, out)
        assert n.value == text_len
        if it >= warmup:
            calls.append(dt * 1e3)
            kernels.append(Z.kernel_ms(ctx))
    ctx.close()
    print("RESULT " + json.dumps({"members": n_members, "text_bytes": text_len, "compressed_bytes": len(blob), "call_ms": calls,
                                  "kernel_ms": kernels, "crc": crc}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=700)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.warmup, a.repeats)
    blob, text_len = build_blob(a.mb, min(16, os.cpu_count() or 1))
    # one CPU thread of zlib over the same members
    t0 = time.perf_counter()
    at, total = 0, 0
    while at < len(blob):
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        total += len(zlib.decompress(blob[at + 18:at + size - 8], -15))
        at += size
    cpu_s = time.perf_counter() - t0
    assert total == text_len
    at, crc = 0, 0                        # untimed: the CRC-32 of the whole text, to hold the GPU's text against
    while at < len(blob):
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        crc = zlib.crc32(zlib.decompress(blob[at + 18:at + size - 8], -15), crc)
        at += size
    with tempfile.NamedTemporaryFile(suffix=".bgzf") as f:
        f.write(blob)
        f.flush()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f.name, "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    if res["crc"] != crc:
        sys.exit("the GPU's text differs from zlib's")
    call, kern = float(np.median(res["call_ms"])), float(np.median(res["kernel_ms"]))
    out = {"text_bytes": text_len, "compressed_bytes": len(blob), "members": res["members"], "level": 6,
           "call_ms_median": call, "call_ms_all": res["call_ms"], "kernel_ms_median": kern, "kernel_ms_all": res["kernel_ms"],
           "call_GBps_text": text_len / call / 1e6, "kernel_GBps_text": text_len / kern / 1e6,
           "zlib_one_thread_GBps_text": text_len / cpu_s / 1e9, "warmup": a.warmup, "repeats": a.repeats}
    if a.step_ms:
        out["e2e_step_ms"] = a.step_ms
        out["ingest_hidden_behind_a_step"] = call <= a.step_ms
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
