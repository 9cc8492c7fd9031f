"""The shard split, export and merge (csrc/merge.hip behind kslam_shard_counts_device, kslam_export_shard_device and
kslam_merge_shards_device) alone, at every seam: the cases of tests/merge_seams.py -- a first R2 CIGAR 0 .. 1000 rows behind the
split or nowhere, splits at 0 / 1 / n - 1 / n of 0 .. 257 rows, a wave of the export that straddles the split, CIGAR offsets that
carry into the high word, read ids up to 2^32 - 3, 1 .. 256 shards with runs of empty ones, shard boundaries at rows 255 / 256 /
257 / 512, CIGARs of 0 / 1 / 300 ops, pool words no row refers to -- against the batch-global table each case was cut from, byte
for byte.  tests/test_merge_seams.py proves on the CPU that every case sits on the seam it names and that the case list tells
each plausible mistake in the kernels from the right answer.

A synthetic table becomes a context's "last result" through kslam_adopt_results_device.  That needs a loaded batch and nothing
else: csrc/api_core.hip checks have_reads and copies the two arrays, it compares no read id with the batch, and none of the
three entry points under test reads the reads (csrc/api_multi.hip: they take res_ov, res_cig, n_res and n_cig only).  So the
dummy batch has 2 * max(n_local_pairs, 1) four-base reads, or two where n_local_pairs is near 2^31.

NOT checked here: the 64-bit arithmetic of the MERGE (pool_base, new_off) beyond the few kilobytes these pools have -- that
would take gigabytes of pool.  The export's 64-bit re-base is checked, because its pool bases are only addends."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_seams as S  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = S.all_cases()
BY_NAME = {c["name"]: c for c in CASES["X"] + CASES["M"]}
GUARD, FILL = 64, 0xA5


def _name(case):
    return case["name"]


@pytest.fixture(scope="module")
def torch(kslam):
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


class Guarded:
    """n bytes of device memory between two guards of 64 bytes, all of it 0xA5"""

    def __init__(self, torch, nbytes):
        self.torch, self.n = torch, nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD

    def at(self, offset):
        return self.ptr + offset

    def read(self, what):
        """the bytes between the guards, the guards checked"""
        self.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + self.n:] == FILL).all(), "%s: a store outside the destination" % what
        return h[GUARD:GUARD + self.n].tobytes()

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.t == FILL).all().item())


def _upload(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _adopt(torch, c, rows, pool, n_local_pairs):
    c.load_reads([b"ACGT"] * (2 * max(n_local_pairs, 1) if n_local_pairs <= 1 << 16 else 2))
    d_rows, d_pool = _upload(torch, rows), _upload(torch, pool)
    c.adopt_results_device(d_rows.data_ptr() if len(rows) else None, len(rows), d_pool.data_ptr() if len(pool) else None, len(pool))


def _adopt_shard(torch, c, case, s=0):
    (rows, pool), (lo, hi) = S.shards_of(case)[s], case["bounds"][s]
    _adopt(torch, c, rows, pool, hi - lo)
    return hi - lo, lo


@pytest.mark.parametrize("case", CASES["S"], ids=_name)
def test_split_and_first_cigar_walk(kslam, torch, ctx, case):
    """k_shard_split at 0 / 1 / n - 1 / n of 0, 1, 2, 255, 256, 257 rows; k_shard_first_cigar finding the first R2 CIGAR in its
    first, second, third and fourth step, in a last step that ends beyond the rows, and not at all"""
    n_loc, _ = _adopt_shard(torch, ctx, case)
    got = ctx.shard_counts_device(n_loc)
    print(case["name"], got, S.counts_of(case))
    assert got == S.counts_of(case), case["name"]


@pytest.mark.parametrize("null_empty_side", [False, True], ids=["pointers", "null_for_empty"])
@pytest.mark.parametrize("case", CASES["X"], ids=_name)
def test_export_in_batch_terms(kslam, torch, ctx, case, null_empty_side):
    """k_export_rows with the split inside a wave, on a block edge, at 0 and at n; the four destinations between guards; an empty
    side given a valid pointer (untouched) or null (accepted); rows without a CIGAR keep offset 0 on both sides"""
    n_loc, lo = _adopt_shard(torch, ctx, case)
    want = S.exported(case)
    pb1, pb2 = want[4:]
    bufs = [Guarded(torch, len(w.tobytes())) for w in want[:4]]
    ptrs = [None if null_empty_side and b.n == 0 else b.ptr for b in bufs]
    ctx.export_shard_device(n_loc, lo, case["n_pairs"], pb1, pb2, *ptrs)
    for what, b, w in zip(("rows of R1", "rows of R2", "pool of R1", "pool of R2"), bufs, want[:4]):
        got = b.read(case["name"] + ": " + what)
        if got != w.tobytes() and what.startswith("rows"):
            g = np.frombuffer(got, dtype=S.OVERLAP_DT)
            bad = [k for k in range(len(g)) if g[k].tobytes() != w[k].tobytes()][:3]
            print(case["name"], what, "first rows that differ:", [(k, g[k], w[k]) for k in bad])
        assert got == w.tobytes(), "%s: %s" % (case["name"], what)


def _merge(torch, c, case, null_when_empty=False):
    rows, pool, shards = S.gathered(case)
    d_rows, d_pool = _upload(torch, rows), _upload(torch, pool)
    out_rows, out_pool = Guarded(torch, case["rows"].nbytes), Guarded(torch, case["pool"].nbytes)
    none = null_when_empty and len(rows) == 0
    c.merge_shards_device(shards, case["n_pairs"], d_rows.data_ptr() if len(rows) else None, d_pool.data_ptr() if len(pool) else None,
                          None if none else out_rows.ptr, None if none else out_pool.ptr)
    got_rows, got_pool = out_rows.read(case["name"] + ": rows"), out_pool.read(case["name"] + ": pool")
    if got_rows != case["rows"].tobytes():
        g = np.frombuffer(got_rows, dtype=S.OVERLAP_DT)
        bad = [k for k in range(len(g)) if g[k].tobytes() != case["rows"][k].tobytes()][:3]
        print(case["name"], "first rows that differ:", [(k, g[k], case["rows"][k]) for k in bad])
    assert got_rows == case["rows"].tobytes(), case["name"]
    assert got_pool == case["pool"].tobytes(), case["name"]


@pytest.mark.parametrize("case", CASES["M"], ids=_name)
def test_merge_of_gathered_shards(kslam, torch, ctx, case):
    """k_merge_plan / k_merge_rows / k_merge_cigars: 1, 2, 3, 255, 256 shards, empty shards (no rows and / or no pairs) at the
    front, in the middle, at the end, alone and a hundred in a row, gaps between the pair ranges, shard boundaries at rows 255,
    256, 257, 512, shards of one block only or one row, CIGARs of 0 / 1 / 300 ops, pool words no row refers to"""
    _merge(torch, ctx, case)
    if len(case["rows"]) == 0:
        _merge(torch, ctx, case, null_when_empty=True)


def test_merge_again_on_one_context_with_smaller_cases(kslam, torch):
    """the mg_* buffers of a context are reused: after 256 shards the next, smaller merge must not see a stale MergeShard"""
    c = kslam.Context()
    try:
        for name in ("m256", "m3_100_empty_middle", "m2", "m_all_empty_1", "m_cigar_0_1_300", "m1", "m_all_empty_3", "m3"):
            _merge(torch, c, BY_NAME[name])
    finally:
        c.close()


@pytest.mark.parametrize("refusal", S.refusals(), ids=lambda r: r[0])
def test_merge_refusals_write_nothing(kslam, torch, ctx, refusal):
    name, shards, n_pairs, null, says = refusal
    rows, ops = max(sum(s[2] for s in shards), 1), max(sum(s[3] for s in shards), 1)
    d_rows = torch.zeros(48 * rows, dtype=torch.uint8, device="cuda")
    d_pool = torch.zeros(4 * ops, dtype=torch.uint8, device="cuda")
    out_rows, out_pool = Guarded(torch, 48 * rows), Guarded(torch, 4 * ops)
    torch.cuda.synchronize()
    with pytest.raises(kslam.KslamError, match=says) as e:
        ctx.merge_shards_device(shards, n_pairs, None if "rows_in" in null else d_rows.data_ptr(), None if "pool_in" in null else d_pool.data_ptr(),
                                None if "rows_out" in null else out_rows.ptr, None if "pool_out" in null else out_pool.ptr)
    assert e.value.status == kslam.KSLAM_ERR_ARG, name
    assert out_rows.untouched() and out_pool.untouched(), name
    _merge(torch, ctx, BY_NAME["m2"])                    # and the context still merges


@pytest.mark.parametrize("name", S.EQUIVALENCE)
def test_export_protocol_and_device_merge_both_give_the_table(kslam, torch, ctx, name):
    """the protocol of the library's own multi-GPU paths -- counts per shard, the placement of kslam_comm_gather_plan, every shard
    exported into its places -- and kslam_merge_shards_device on the same shards: both are the batch-global table"""
    kc = importlib.import_module("kslam_amd.comm")
    case = BY_NAME[name]
    counts = []
    for s in range(len(case["bounds"])):
        n_loc, _ = _adopt_shard(torch, ctx, case, s)
        counts.append(ctx.shard_counts_device(n_loc))
        assert counts[-1] == S.counts_of(case, s), (name, s)
    row1, row2, op1, op2, (n_rows, n_ops) = kc.gather_plan(counts)
    assert (n_rows, n_ops) == (len(case["rows"]), len(case["pool"]))
    rows, pool = Guarded(torch, 48 * n_rows), Guarded(torch, 4 * n_ops)
    for s in range(len(case["bounds"])):
        n_loc, lo = _adopt_shard(torch, ctx, case, s)
        ctx.export_shard_device(n_loc, lo, case["n_pairs"], op1[s], op2[s], rows.at(48 * row1[s]), rows.at(48 * row2[s]),
                                pool.at(4 * op1[s]), pool.at(4 * op2[s]))
    assert rows.read(name + ": rows") == case["rows"].tobytes()
    assert pool.read(name + ": pool") == case["pool"].tobytes()
    _merge(torch, ctx, case)


# ---- the sending side of kslam_multi_align_batch when a shard returns no rows, only R1 rows or only R2 rows ----------------------
N_PAIRS, N_DEV = 300, 3


@pytest.fixture(scope="module")
def lopsided(kslam, synth):
    genomes = synth.make_genomes(940, 3, 1, 8000, strain_sub=0.02, strain_indel=0.001, shared_segment=1000)
    reads, truth = synth.make_paired_reads(941, genomes, N_PAIRS, sub_rate=0.015, indel_rate=0.004, edge_frac=0.05)
    planted = [i for i in range(N_PAIRS) if truth[i][0] >= 0 and 0 <= truth[i][1] < 7000]      # reads cut from inside a genome
    gb = synth.to_bytes(genomes)
    one = kslam.Context()
    one.set_index(gb)
    multi = kslam.MultiContext([0] * N_DEV)
    multi.set_index(gb)
    yield synth.to_bytes(reads), one, multi, planted
    multi.close()
    one.close()


def _replaced(synth, reads, ids, seed):
    """reads `ids` of the batch replaced by seeded random bases of the same length"""
    rng = np.random.default_rng(seed)
    out = list(reads)
    for i in ids:
        out[i] = synth.random_bases(rng, len(out[i])).tobytes()
    return out


def _rows_in(exp, lo, hi):
    return int(((exp["read"] >= lo) & (exp["read"] < hi)).sum())


# shard k holds pairs [100 k, 100 (k + 1)): its R1 reads have these ids, its R2 reads 300 more
LOPSIDED = {
    "middle_shard_without_rows": (list(range(100, 200)) + list(range(400, 500)), 950, [(100, 200), (400, 500)]),
    "last_shard_r1_rows_only": (list(range(500, 600)), 951, [(500, 600)]),
    "collecting_shard_r2_rows_only": (list(range(0, 100)), 952, [(0, 100)]),
}


@pytest.mark.parametrize("which", sorted(LOPSIDED))
def test_multi_device_entry_with_lopsided_shards(kslam, synth, lopsided, which):
    """so + n1, sp + c1 and the four conditional peer copies with a piece of a shard empty: both mates of the middle shard, R2 of
    the last shard, R1 of shard 0 (the collecting device, which exports straight into the final arrays) are random bases"""
    reads, one, multi, _ = lopsided
    ids, seed, empty = LOPSIDED[which]
    rb = _replaced(synth, reads, ids, seed)
    exp, ecig = one.align_batch(rb)
    for lo, hi in empty:                                   # a random read that happens to hit: change the seed above
        assert _rows_in(exp, lo, hi) == 0, (which, lo, hi)
    for k in range(N_DEV):
        for lo, hi in ((100 * k, 100 * k + 100), (N_PAIRS + 100 * k, N_PAIRS + 100 * k + 100)):
            if (lo, hi) not in empty:
                assert _rows_in(exp, lo, hi) > 50, (which, lo, hi)
    assert len(ecig) > 0
    for _ in range(2):
        got, gcig = multi.align_batch(rb, paired=True)
        assert got.tobytes() == exp.tobytes() and gcig.tobytes() == ecig.tobytes(), which


def test_multi_device_entry_unpaired_with_fewer_reads_than_devices(kslam, lopsided):
    reads, one, multi, planted = lopsided
    for n in (2, 1):
        few = [reads[i] for i in planted[:n]]
        exp, ecig = one.align_batch(few)
        assert len(exp) >= n and len(ecig) > 0
        got, gcig = multi.align_batch(few, paired=False)
        assert got.tobytes() == exp.tobytes() and gcig.tobytes() == ecig.tobytes(), n
