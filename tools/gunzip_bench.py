#!/usr/bin/env python3
"""Rate of kslam_gunzip_inflate (include/kslam_gunzip.h) on FASTQ-like text compressed at level 6 into ONE plain gzip member.

Prints, and writes to profiles/gunzip.json, for chunk sizes of 32, 64, 128, 256 and 512 KiB: the device time of every stage
(kslam_gunzip_last_stats), the window chain's share of their sum, GB/s of text over the kernels and over the whole call, and
the starts found / live / dropped.  Two comparators from the same run on the same box:
  (a) zlib.decompress of the same file on one CPU thread -- what `gunzip` in front of the run costs;
  (b) kslam_bgzf_inflate of the same text as BGZF -- what not knowing the block starts costs.
The GPU steps run in a child process under a time limit of its own; a run that finds no GPU fails.

    python tools/gunzip_bench.py [--mb 256] [--warmup 1] [--repeats 3]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inflate_bench import build_blob, fastq_like   # noqa: E402  (the same text generator, and the BGZF comparator's file)

CHUNKS_KIB = (32, 64, 128, 256, 512)
STAGES = ("find_ms", "count_ms", "decode_ms", "window_ms", "resolve_ms", "check_ms")


def gzip_member(text):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(text) + c.flush()
    return bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF]) + body + (zlib.crc32(text)).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")


def child(gz_path, bgzf_path, warmup, repeats):
    import ctypes as C
    from __graft_entry__ import load_package
    K = load_package()
    G = importlib.import_module("kslam_amd.gunzip")
    Z = importlib.import_module("kslam_amd.inflate")
    blob, bgzf = open(gz_path, "rb").read(), open(bgzf_path, "rb").read()
    ctx = K.Context()
    L = G.lib()
    res = {"chunks": {}}
    for kib in CHUNKS_KIB:
        G.set_chunk(ctx, kib * 1024)
        calls, stats, crc = [], [], None
        for it in range(warmup + repeats):
            out, n = C.c_void_p(), C.c_uint64()
            t0 = time.perf_counter()
            ctx._chk(L.kslam_gunzip_inflate(ctx._h, blob, len(blob), C.byref(out), C.byref(n)))
            dt = time.perf_counter() - t0
            if it == 0:
                crc = zlib.crc32(C.string_at(out.value, n.value))
            L.kslam_free_pinned(ctx._h, out)
            if it >= warmup:
                calls.append(dt * 1e3)
                stats.append(G.stats(ctx))
        res["chunks"][str(kib)] = {"call_ms": calls, "stats": stats, "crc": crc}
    G.set_chunk(ctx, 0)
    ZL = Z.lib()
    calls, kernels, crc = [], [], None
    for it in range(warmup + repeats):
        out, n = C.c_void_p(), C.c_uint64()
        t0 = time.perf_counter()
        ctx._chk(ZL.kslam_bgzf_inflate(ctx._h, bgzf, len(bgzf), C.byref(out), C.byref(n)))
        dt = time.perf_counter() - t0
        if it == 0:
            crc = zlib.crc32(C.string_at(out.value, n.value))
        ZL.kslam_free_pinned(ctx._h, out)
        if it >= warmup:
            calls.append(dt * 1e3)
            kernels.append(Z.kernel_ms(ctx))
    res["bgzf"] = {"call_ms": calls, "kernel_ms": kernels, "crc": crc, "compressed_bytes": len(bgzf)}
    ctx.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip.json"))
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.warmup, a.repeats)
    bgzf, text_len = build_blob(a.mb, min(16, os.cpu_count() or 1))          # the text as BGZF, in pieces of 16 MiB ...
    pieces = max(1, a.mb // 16)
    text = b"".join(fastq_like((a.mb << 20) // pieces, 100 + k).tobytes() for k in range(pieces))   # ... and the same text whole
    assert len(text) == text_len
    blob = gzip_member(text)
    crc = zlib.crc32(text)
    t0 = time.perf_counter()
    plain = zlib.decompress(blob[10:-8], -15)
    cpu_s = time.perf_counter() - t0
    assert plain == text
    del plain
    with tempfile.NamedTemporaryFile(suffix=".gz") as f, tempfile.NamedTemporaryFile(suffix=".bgzf") as g:
        f.write(blob)
        f.flush()
        g.write(bgzf)
        g.flush()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f.name, g.name, "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0 or "RESULT " not in r.stdout:
        sys.exit("the GPU step failed (no GPU, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    if res["bgzf"]["crc"] != crc or any(c["crc"] != crc for c in res["chunks"].values()):
        sys.exit("the GPU's text differs from zlib's")
    out = {"text_bytes": text_len, "compressed_bytes": len(blob), "level": 6, "members": 1, "warmup": a.warmup, "repeats": a.repeats,
           "zlib_one_thread_GBps_text": text_len / cpu_s / 1e9, "chunks_KiB": {}}
    for kib, c in res["chunks"].items():
        med = {s: float(np.median([x[s] for x in c["stats"]])) for s in STAGES}
        kern = sum(med.values())
        call = float(np.median(c["call_ms"]))
        st = c["stats"][-1]
        out["chunks_KiB"][kib] = dict(med, kernels_ms=kern, window_share=med["window_ms"] / kern, kernels_GBps_text=text_len / kern / 1e6,
                                      call_ms_median=call, call_GBps_text=text_len / call / 1e6,
                                      **{k: st[k] for k in ("chunks", "starts_found", "starts_live", "starts_dropped", "rounds")})
    best = min(out["chunks_KiB"], key=lambda k: out["chunks_KiB"][k]["kernels_ms"])
    out["best_chunk_KiB_by_kernels"] = int(best)
    out["best_chunk_KiB_by_call"] = int(min(out["chunks_KiB"], key=lambda k: out["chunks_KiB"][k]["call_ms_median"]))
    b = res["bgzf"]
    call, kern = float(np.median(b["call_ms"])), float(np.median(b["kernel_ms"]))
    out["bgzf_inflate"] = {"compressed_bytes": b["compressed_bytes"], "call_ms_median": call, "kernel_ms_median": kern,
                           "call_GBps_text": text_len / call / 1e6, "kernel_GBps_text": text_len / kern / 1e6}
    out["gunzip_over_zlib_one_thread_by_call"] = out["chunks_KiB"][best]["call_GBps_text"] / out["zlib_one_thread_GBps_text"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
