#!/usr/bin/env python3
"""Rate of the Kraken-style report's passes (include/kslam_kreport.h, csrc/kreport.hip) on one batch of taxonomy ids over a
synthetic tree of NCBI's size: --nodes nodes (a random recursive tree: every node's parent is an earlier node), --ids ids through
kslam_kreport_add.

Two shapes: "uniform" (the ids spread evenly over --taxa taxa) and "skewed" (90 % of the ids on one taxon, the rest spread over
the same taxa: what a real sample looks like).  Per shape 2 warm-up and 5 timed count passes after a reset each
(kslam_kreport_kernel_ms: HIP events around the count kernel), then one take.  With --ablate-lib (the measurement-only
`make ABLATE=1` library) the same count passes run once more with the wave combining compiled out (KSLAM_KREPORT_ABLATE=1): one
atomic per read pair.  Prints, and writes to profiles/kreport.json, the medians.  The rows' sums are checked against the ids.
Every GPU step runs in a child process under a time limit of its own; a run that finds no GPU fails.

    python tools/kreport_bench.py [--ids 1000000] [--nodes 2000000] [--taxa 10000] [--warmup 2] [--repeats 5] [--ablate-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_tree(n_nodes, seed=1):
    """taxDB text of ids 2 .. n_nodes + 1 under root 1: the parent of node k is a random earlier node (depth ~ 2 ln n)"""
    rng = np.random.default_rng(seed)
    parents = np.ones(n_nodes, dtype=np.int64)
    k = np.arange(8, n_nodes)
    parents[8:] = 2 + (rng.random(n_nodes - 8) * k).astype(np.int64)
    ranks = [b"no rank", b"species", b"genus", b"family", b"order", b"class", b"phylum", b"superkingdom"]
    return b"".join(b"%d\n%d\nt%d\n%s\n" % (2 + i, p, 2 + i, ranks[i & 7]) for i, p in enumerate(parents.tolist()))


def child(a):
    import importlib
    from __graft_entry__ import load_package
    K = load_package()
    KR = importlib.import_module("kslam_amd.kreport")
    ST = importlib.import_module("kslam_amd.samtext")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    tax = X.TaxDB(make_tree(a.nodes))
    ctx = K.Context()
    bases, off = np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64)
    ctx.set_index_arrays(bases, off)
    index = T.IndexArrays(bases, off, taxonomy_ids=[2])
    ST.set_annotations(ctx, index, tax)
    KR.set_kreport(ctx, True)
    rng = np.random.default_rng(3)
    taxa = (2 + rng.choice(a.nodes, a.taxa, replace=False)).astype(np.uint32)
    uniform = rng.choice(taxa, a.ids)
    skewed = uniform.copy()
    skewed[rng.random(a.ids) < 0.9] = taxa[0]
    out = {"ids": a.ids, "nodes": len(tax), "taxa": a.taxa, "combining": os.environ.get("KSLAM_KREPORT_ABLATE") != "1"}
    for shape, ids in (("uniform", uniform), ("skewed", skewed)):
        counts = []
        for it in range(a.warmup + a.repeats):
            KR.reset(ctx)
            KR.add(ctx, ids)
            if it >= a.warmup:
                counts.append(KR.kernel_ms(ctx)[0])
        rows, stats = KR.take(ctx)
        values, n = np.unique(ids, return_counts=True)
        got = {int(r["tax_id"]): int(r["direct"]) for r in rows if r["direct"]}
        if stats["n_ids"] != a.ids or got != dict(zip(values.tolist(), n.tolist())):
            sys.exit("the rows' direct counts differ from the ids' (%s)" % shape)
        out[shape] = {"count_ms_all": counts, "count_ms_median": float(np.median(counts)), "take_ms": KR.kernel_ms(ctx)[1], "rows": int(stats["n_rows"]),
                      "distinct_ids": int(len(values))}
    KR.set_kreport(ctx, False)
    ctx.close()
    print("RESULT " + json.dumps(out))


def run_child(a, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ids", str(a.ids), "--nodes", str(a.nodes), "--taxa", str(a.taxa),
                        "--warmup", str(a.warmup), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.timeout, env=env)
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
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--ablate-lib", default=None, help="libkslam_hip_ablate.so (make -C k-slam_amd/csrc ABLATE=1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kreport.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = run_child(a, {})
    if a.ablate_lib:
        if not os.path.exists(a.ablate_lib):
            sys.exit(a.ablate_lib + " is missing: make -C k-slam_amd/csrc ABLATE=1")
        ab = run_child(a, {"KSLAM_LIB": os.path.abspath(a.ablate_lib), "KSLAM_KREPORT_ABLATE": "1"})
        for shape in ("uniform", "skewed"):
            out[shape]["count_ms_no_combining_all"] = ab[shape]["count_ms_all"]
            out[shape]["count_ms_no_combining_median"] = ab[shape]["count_ms_median"]
    out["warmup"], out["repeats"] = a.warmup, a.repeats
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
