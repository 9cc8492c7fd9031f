"""The coordinate-sorted BAM and its BAI index made on the device (kslam_bam_sort_take, include/kslam_bamsort.h) from hand-built
record batches (tests/bamsort_cases.py) through kslam_bam_sort_add: byte for byte against the host twins and the restatement
(tests/bamsort_ref.py), the file as bgzf(header) + bgzf(stream) + EOF by kslam_bgzf_compress and, for a small stream, by
tests/deflate_ref.py, the index through tests/bai_check.py; the knobs that change no byte; the refusals."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_check  # noqa: E402
import bamsort_cases as BC  # noqa: E402
import bamsort_ref as R  # noqa: E402
import deflate_ref  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = BC.cases()


def _index_arrays(lengths, seed=3):
    rng = np.random.default_rng(seed)
    goff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(goff[-1]))]
    return np.concatenate([bases, np.zeros(64, dtype=np.uint8)]), goff


class _Bench:
    def __init__(self, kslam):
        self.K = kslam
        self.BS = importlib.import_module("kslam_amd.bamsort")
        self.Z = importlib.import_module("kslam_amd.bgzf")
        self.c = kslam.Context()
        self.keep, goff = _index_arrays([n for _, n in BC.REFS])
        self.c.set_index_arrays(self.keep, goff)
        self.BS.set_bam_sort(self.c, True)

    def run(self, batches, order=None, slice_bytes=0, segment=0, gather=0, deflate=0, index=True):
        BS, c = self.BS, self.c
        BS.reset(c)
        BS.set_slice(c, slice_bytes)
        BS.set_segment(c, segment)
        BS.set_gather(c, gather)
        self.Z.set_deflate(c, deflate)
        for seq in (order if order is not None else range(len(batches))):
            BS.add(c, seq, batches[seq])
        out = BS.take(c, BC.SAM_HEADER, index=index)
        self.Z.set_deflate(c, 0)
        return out

    def expect(self, batches, bam, bai, stats, deflate=0):
        """the whole definition: twins, restatement, file layout, checker, stats"""
        BS = self.BS
        stream = R.sort_batches(batches)
        assert BS.tail_bam_sort(batches) == stream
        header = R.bam_header(R.coordinate_header(BC.SAM_HEADER), BC.REFS)
        self.Z.set_deflate(self.c, deflate)
        head, body = self.Z.compress(self.c, header), self.Z.compress(self.c, stream)
        self.Z.set_deflate(self.c, 0)
        assert bam == head + body + BC.EOF
        sizes = BC.member_sizes(bam, len(head))
        want = R.bai(stream, len(BC.REFS), sizes, len(head))
        assert bai == want and BS.tail_bai(stream, len(BC.REFS), sizes, len(head)) == want
        got = bai_check.check(bam, bai)
        recs = R.split(stream)
        assert stats["n_records"] == got["n_records"] == len(recs) and stats["n_no_coor"] == got["n_no_coor"]
        assert stats["record_bytes"] == len(stream) and stats["compressed_bytes"] == len(body) and stats["n_members"] == len(sizes)
        assert stats["n_chunks"] == got["n_chunks"] and (stats["bytes_held"] >= len(stream))
        return stream


@pytest.fixture(scope="module")
def bench(kslam):
    b = _Bench(kslam)
    yield b
    b.BS.set_bam_sort(b.c, False)
    b.c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_take_against_twins_restatement_and_checker(bench, name):
    bam, bai, stats = bench.run(CASES[name])
    bench.expect(CASES[name], bam, bai, stats)


def test_batches_added_out_of_order_and_ties(bench):
    batches = CASES["all_keys_equal"]
    bam, bai, stats = bench.run(batches, order=[2, 0, 1])
    stream = bench.expect(batches, bam, bai, stats)
    names = [r[36:r.index(b"\0", 36)] for r in R.split(stream)]
    assert names == [b"b%d_%d" % (b, i) for b in range(3) for i in range(5)]
    assert bench.run(CASES["mixed"], order=[3, 1, 0, 2])[:2] == bench.run(CASES["mixed"])[:2]


def test_stream_sizes_at_the_member_edge(bench):
    for name, size in (("ends_at_member_edge", BC.M), ("ends_at_member_edge_plus_one", BC.M + 1)):
        bam, bai, stats = bench.run(CASES[name])
        assert stats["record_bytes"] == size and stats["n_members"] == (size + BC.M - 1) // BC.M


@pytest.mark.parametrize("name", ["mixed", "straddles_member_edge", "record_longer_than_a_member"])
def test_knobs_change_no_byte(bench, name):
    batches = CASES[name]
    base = bench.run(batches)
    assert base[2]["n_members"] >= 2
    for kw in ({"slice_bytes": BC.M}, {"slice_bytes": 2 * BC.M}, {"slice_bytes": 1}, {"segment": 1}, {"segment": 1 << 30}, {"gather": 1}, {"gather": 16},
               {"gather": 64}, {"slice_bytes": BC.M, "gather": 1, "segment": 3}):
        assert bench.run(batches, **kw)[:2] == base[:2], kw


def test_both_deflate_modes(bench):
    batches = CASES["mixed"]
    fixed = bench.run(batches, deflate=0)
    dynamic = bench.run(batches, deflate=1)
    bench.expect(batches, *dynamic, deflate=1)
    assert len(dynamic[0]) < len(fixed[0]) and dynamic[1] != fixed[1]      # smaller members, other virtual offsets
    # a small stream against the restatement of the compressor
    small = CASES["pos_minus_one_on_a_reference"]
    for mode in (deflate_ref.FIXED, deflate_ref.DYNAMIC):
        bam, _, _ = bench.run(small, deflate=mode)
        header = R.bam_header(R.coordinate_header(BC.SAM_HEADER), BC.REFS)
        assert bam == deflate_ref.compress(header, mode) + deflate_ref.compress(R.sort_batches(small), mode) + BC.EOF


def test_take_is_repeatable_and_more_batches_may_follow(bench):
    batches = CASES["mixed"]
    BS, c = bench.BS, bench.c
    first = bench.run(batches[:2])
    assert BS.take(c, BC.SAM_HEADER)[:2] == first[:2]
    BS.add(c, 2, batches[2])
    BS.add(c, 3, batches[3])
    bam, bai, stats = BS.take(c, BC.SAM_HEADER)
    bench.expect(batches, bam, bai, stats)
    assert BS.take(c, BC.SAM_HEADER, index=False)[0] == bam
    ms = BS.kernel_ms(c)
    assert set(ms) == set(BS.KERNEL_MS_NAMES) and all(v >= 0 for v in ms.values()) and ms["gather"] > 0 and ms["sort"] > 0


def test_refusals_leave_the_state_as_it_was(bench, kslam):
    BS, c = bench.BS, bench.c
    batches = CASES["empty_batch_between"]
    good = bench.run(batches)
    rec = BC.rec(0, 5)
    for bad, what in ((rec[:-1], "chain"), (rec + b"\x01\x00", "chain"), (b"\x10\x00\x00\x00" + bytes(16), "fixed part"), (BC.rec(3, 5), "refID"),
                      (BC.rec(1, 2990), "past the end")):
        with pytest.raises(kslam.KslamError, match=what) as e:
            BS.add(c, 3, rec + bad)
        assert e.value.status == 1
    with pytest.raises(kslam.KslamError, match="already held") as e:
        BS.add(c, 1, rec)
    assert e.value.status == 1
    assert BS.take(c, BC.SAM_HEADER)[:2] == good[:2]
    # a missing ordinal
    BS.add(c, 4, rec)
    with pytest.raises(kslam.KslamError, match="ordinal 3 is missing") as e:
        BS.take(c, BC.SAM_HEADER)
    assert e.value.status == 5
    BS.add(c, 3, b"")
    assert BS.take(c, BC.SAM_HEADER)[2]["n_records"] == good[2]["n_records"] + 1
    # a header that is not the index's
    with pytest.raises(kslam.KslamError, match="@SQ") as e:
        BS.take(c, b"@SQ\tSN:chrA\tLN:200000\n")
    assert e.value.status == 1
    with pytest.raises(kslam.KslamError, match="1, 16 or 64"):
        BS.set_gather(c, 5)
    # switched off: every entry refuses, and the switch comes back empty
    BS.set_bam_sort(c, False)
    assert not BS.get_bam_sort(c)
    for call in (lambda: BS.add(c, 0, rec), lambda: BS.take(c, BC.SAM_HEADER), lambda: BS.reset(c), lambda: BS.set_slice(c, 0)):
        with pytest.raises(kslam.KslamError, match="kslam_set_bam_sort") as e:
            call()
        assert e.value.status == 5
    BS.set_bam_sort(c, True)
    assert BS.get_bam_sort(c) and BS.take(c, BC.SAM_HEADER)[2]["n_records"] == 0


def test_switch_on_preconditions(kslam):
    BS = importlib.import_module("kslam_amd.bamsort")
    c = kslam.Context()
    try:
        with pytest.raises(kslam.KslamError, match="kslam_set_index") as e:
            BS.set_bam_sort(c, True)
        assert e.value.status == 5
        # an entry of 2^29 + 1 bases: BAI cannot address it
        n = (1 << 29) + 1
        keep = np.full(n + 64 + 1000, ord("N"), dtype=np.uint8)
        keep[n:n + 1000] = np.frombuffer(b"ACGT" * 250, dtype=np.uint8)
        c.set_index_arrays(keep, np.array([0, n, n + 1000], dtype=np.uint64))
        with pytest.raises(kslam.KslamError, match="2\\^29") as e:
            BS.set_bam_sort(c, True)
        assert e.value.status == 4 and not BS.get_bam_sort(c)
    finally:
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert BS.lib().kslam_set_bam_sort(h, 1) == 4
    finally:
        m.close()
