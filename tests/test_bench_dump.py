"""bench.py --dump-outputs without a GPU: the helpers on host tensors at the sizes of the largest configurations (10 M read
pairs), against a plain numpy restatement -- what is kept, its values, the 64 MB bound, and that the rows kept depend on the
batch's read indices, not on how many records a build returned."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def bench():
    import bench as B
    return B


def _result(B, n_reads, rows_per_read, seed, drop=()):
    """a synthetic alignToDatabase result in (read, entry, rel) order with a CIGAR pool; reads in `drop` have no records"""
    per = np.full(n_reads, rows_per_read)
    per[list(drop)] = 0
    read = np.repeat(np.arange(n_reads), per)
    ov = np.zeros(len(read), dtype=B.OVERLAP_DT)
    ov["read"] = read
    ov["entry"] = (np.arange(len(read)) - np.repeat(np.cumsum(per) - per, per)) * 17 + seed
    ov["rel"] = read * 7 % 1000
    ov["score"] = (read * 13 + ov["entry"]) % 600
    ov["query_end"] = 149
    lens = ((read + ov["entry"]) % 4).astype(np.uint32)
    ov["cigar_len"] = lens
    off = np.cumsum(lens.astype(np.int64)) - lens
    ov["cigar_off"] = np.where(lens > 0, off, 0)
    n_ops = int(lens.sum())
    cg = ((np.arange(n_ops, dtype=np.int64) * 2654435761) % (1 << 32)).astype(np.uint32)
    return ov, cg


def _dump_hot(B, d, ov, cg, n_reads):
    B.clear_dump(str(d))
    B.dump_hot_path(str(d), torch.from_numpy(ov.view(np.uint8).reshape(-1).copy()), torch.from_numpy(cg.view(np.uint8).copy()), n_reads)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_hot_path_dump_values_and_bound(bench, tmp_path):
    B = bench
    n_reads = 100_000
    ov, cg = _result(B, n_reads, 6, 1)                # 6 records per read: more than DUMP_ROWS of the sampled reads' records
    a = _dump_hot(B, tmp_path, ov, cg, n_reads)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["hot_path_counts"].tolist() == [len(ov), len(cg)]
    reads = a["hot_path_sampled_reads"].astype(np.int64)
    full = B.seeded_sample(n_reads, B.DUMP_READS)
    assert len(full) == B.DUMP_READS and np.array_equal(reads, full[:len(reads)]) and len(reads) < len(full)
    want = ov[np.isin(ov["read"], reads)]
    assert len(want) <= B.DUMP_ROWS
    for c in B.OVERLAP_COLUMNS:
        assert np.array_equal(a["hot_path_" + c], want[c].astype(np.float64)), c
    ops = np.concatenate([cg[int(o):int(o) + int(n)] for o, n in zip(want["cigar_off"], want["cigar_len"])])
    assert np.array_equal(a["hot_path_cigar_of_sampled_rows"], ops[:B.DUMP_OPS].astype(np.float64))
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6


def test_hot_path_sample_is_keyed_by_read(bench, tmp_path):
    """two results of the same batch that differ in some reads' records keep the same records for every other sampled read"""
    B = bench
    n_reads = 50_000
    ov, cg = _result(B, n_reads, 2, 2)
    sampled = B.seeded_sample(n_reads, B.DUMP_READS)
    gone = [int(sampled[5]), 7, 11, 40_000]
    ov2, cg2 = _result(B, n_reads, 2, 2, drop=gone)
    a = _dump_hot(B, tmp_path / "a", ov, cg, n_reads)
    b = _dump_hot(B, tmp_path / "b", ov2, cg2, n_reads)
    assert np.array_equal(a["hot_path_sampled_reads"], b["hot_path_sampled_reads"])
    assert a["hot_path_counts"][0] != b["hot_path_counts"][0]
    ka = ~np.isin(a["hot_path_read"], gone)
    for c in ("read", "rel", "score", "cigar_len"):
        assert np.array_equal(a["hot_path_" + c][ka], b["hot_path_" + c]), c


def test_e2e_dump_at_10m_pairs(bench, tmp_path):
    """--config 2 / --config 4 batches: 10 M read pairs, their taxa sampled, the whole directory within 64 MB"""
    B = bench
    pairs, steps = 10_000_000, 2
    ids = (np.arange(pairs * steps, dtype=np.int64) * 7919 % 100_003).astype(np.uint32)
    sam, pr = tmp_path / "x.sam", tmp_path / "x_PerRead"
    sam.write_bytes(bytes(range(256)) * (3 << 14))
    pr.write_bytes(b"q1\t17\n" * 1000)
    d = tmp_path / "dump"
    ov, cg = _result(B, 100_000, 6, 3)
    _dump_hot(B, d, ov, cg, 100_000)
    B.dump_e2e(str(d), pairs, {"tax_ids": ids}, str(sam), str(pr))
    a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    pick = a["e2e_sampled_pairs"].astype(np.int64)
    assert len(pick) == B.DUMP_PAIRS and np.array_equal(pick, B.seeded_sample(pairs, B.DUMP_PAIRS))
    assert np.array_equal(a["e2e_tax_ids"], ids[pairs:][pick].astype(np.float64))
    assert a["e2e_file_bytes"].tolist() == [sam.stat().st_size, pr.stat().st_size]
    assert np.array_equal(a["e2e_sam_text_end"], np.frombuffer(sam.read_bytes()[-B.DUMP_TAIL_BYTES:], dtype=np.uint8).astype(np.float32))
    assert np.array_equal(a["e2e_per_read_text_end"], np.frombuffer(pr.read_bytes(), dtype=np.uint8).astype(np.float32))
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6


def test_dump_directory_holds_one_run(bench, tmp_path):
    """a second run into the same directory leaves no file of the first (an e2e_* beside a --no-e2e run's hot_path_*)"""
    B = bench
    (tmp_path / "e2e_tax_ids.npy").write_bytes(b"old")
    (tmp_path / "hot_path_score.npy").write_bytes(b"old")
    (tmp_path / "notes.txt").write_text("kept")
    B.clear_dump(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["notes.txt"]
