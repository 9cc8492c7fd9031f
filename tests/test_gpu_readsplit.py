"""The reads split on the GPU (csrc/readsplit.hip, include/kslam_readsplit.h): the device's four blocks against the host twin
(kslam_tail_split_reads) and the plain-Python restatement (tests/readsplit_ref.py), byte for byte -- the format cases, the
scan-tile seams, BGZF across a member boundary, real batches through the lanes and through kslam_stream_classify, and the
refusals."""
import gzip
import importlib
import os

import numpy as np
import pytest

import bgzf_check
import readsplit_ref as R

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_UNSUPPORTED, ERR_STATE = 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def RS(kslam):
    return importlib.import_module("kslam_amd.readsplit")


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


def _three_ways(RS, ctx, r1, r2, sel, n, which=3, max_pairs=0, at_eof=True):
    rp = R.read_pairs(sel, n, paired=r2 is not None)
    exp, n_exp = R.split(r1, r2, sel, which, max_pairs, at_eof)
    host = RS.tail_split_reads(r1, r2, rp, which, max_pairs, at_eof)
    dev = RS.split_reads_text(ctx, r1, r2, rp, which, max_pairs, at_eof)
    assert dev["blocks"] == exp and host["blocks"] == exp
    assert dev["n_records"] == n_exp == host["n_records"] and dev["flags"] == 0
    return dev["blocks"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_blocks_equal_twin_and_restatement(RS, ctx, case):
    name, r1, r2, max_pairs, at_eof = case
    n = len(R.records(r1, max_pairs, at_eof))
    for pname, sel in R.patterns(n).items():
        both = _three_ways(RS, ctx, r1, r2, sel, n, 3, max_pairs, at_eof)
        for k, text in enumerate([r1] + ([r2] if r2 is not None else [])):
            assert R.merge(both[k], both[2 + k], sel, n) == b"".join(R.records(text, max_pairs, at_eof)), (name, pname)
    alt = R.patterns(n)["alternating"]
    _three_ways(RS, ctx, r1, r2, alt, n, 1, max_pairs, at_eof)
    _three_ways(RS, ctx, r1, r2, alt, n, 2, max_pairs, at_eof)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_scan_tile_seams(RS, ctx, n):
    """one scan tile (SCAN_TILE = 4096 lengths) less one, exactly, plus one; the selected set changes at the seam"""
    r1 = R.text_of(n, [b"\n", b"\n", b"\r\n"], n_bases=6)
    r2 = R.text_of(n, b"\n", n_bases=9, mate=2)
    for sel in ([r for r in range(n) if (r < 4095) == (r % 2 == 0)], list(range(4095, n)), list(range(0, min(n, 4096))), [4094], [n - 1]):
        _three_ways(RS, ctx, r1, r2, sel, n)


@pytest.mark.parametrize("mode", [0, 1])
def test_bgzf_across_a_member_boundary(kslam, RS, ctx, mode):
    """250 records of 150 bases: the selected stream is longer than one member's 65 280 input bytes"""
    Z = importlib.import_module("kslam_amd.bgzf")
    n = 250
    r1, r2 = R.text_of(n, n_bases=150), R.text_of(n, b"\r\n", n_bases=150, mate=2)
    sel = [r for r in range(n) if r % 10]
    plain, _ = R.split(r1, r2, sel)
    assert len(plain[0]) > bgzf_check.MAX_INPUT > len(plain[2])
    Z.set_deflate(ctx, mode)
    RS.set_reads_out_bgzf(ctx, True)
    try:
        assert RS.get_reads_out_bgzf(ctx)
        dev = RS.split_reads_text(ctx, r1, r2, R.read_pairs(sel, n))
        assert dev["flags"] == RS.FLAG_BGZF
        host = RS.tail_split_reads(r1, r2, R.read_pairs(sel, n))["blocks"]
        for k in range(4):
            z = dev["blocks"][k]
            assert gzip.decompress(z + Z.EOF) == plain[k] == host[k]
            if mode == 0:   # the strict validator knows stored and fixed members
                assert bgzf_check.check(z + Z.EOF) == plain[k]
                assert [m[3] for m in bgzf_check.members(z + Z.EOF)[:-1]] == ([bgzf_check.MAX_INPUT, len(plain[k]) - bgzf_check.MAX_INPUT] if k < 2 else [len(plain[k])])
            assert z == Z.compress(ctx, host[k])   # the host twin's route (kslam_bgzf_compress) writes the same file
        empty = RS.split_reads_text(ctx, r1, r2, R.read_pairs(list(range(n)), n))
        assert empty["blocks"][2] == b"" and empty["blocks"][3] == b""   # an empty stream gives no member
    finally:
        RS.set_reads_out_bgzf(ctx, False)
        Z.set_deflate(ctx, 0)


# ---- real batches: a small index, about half of the pairs from no genome of it ----

@pytest.fixture(scope="module")
def world(kslam, synth, tmp_path_factory):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    tmp = tmp_path_factory.mktemp("readsplit")
    n = 900
    case = RL.make_case(synth, n_pairs=n, seed=7311)
    rng = np.random.default_rng(5)
    bases = list(case["bases"])
    for i in range(n):
        if i % 2:   # a pair from nowhere
            for j in (i, n + i):
                bases[j] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), len(bases[j])))
    case["r1"] = RL.fastq_text(bases[:n], case["quals"][:n], case["ids"], 1)
    case["r2"] = RL.fastq_text(bases[n:], case["quals"][n:], case["ids"], 2, eol=b"\r\n")
    RL.write_case(case, tmp, D)
    db = D.Database.load(os.path.join(str(tmp), "db", "database"))
    return {"case": case, "db": db, "tmp": tmp, "n": n}


def _indexed_context(kslam, world, **params):
    import ctypes as C
    c = kslam.Context(**params)
    bases_pp, lens_p = world["db"].entry_pointers()
    c._chk(c._L.kslam_set_index(c._h, world["db"].n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
    return c


def _host_text(kslam, text):
    h = kslam.HostBuffer(len(text) + 64)
    h.a[:len(text)] = np.frombuffer(text, dtype=np.uint8)
    return h


def test_a_batch_through_the_lanes(kslam, RS, world):
    """kslam_submit_batch_fastq_text -> kslam_collect_batch -> kslam_collect_reads_out: the blocks are the split by the batch's own
    read_pairs (host twin, restatement), classified and unclassified merged are the LF-normalised input, and the alignment is what
    it is with the switch off"""
    r1, r2, n = world["case"]["r1"], world["case"]["r2"], world["n"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    try:
        c.set_pairing(stages=7)
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        ov0, _, _, _, release0 = c.collect_batch(tk)
        rp0 = c.last_pairs[0].copy()
        ov0 = ov0.copy()
        release0()
        with pytest.raises(kslam.KslamError):   # the switch was off for that batch
            RS.collect_reads_out(c, tk)
        RS.set_reads_out(c, 3)
        assert RS.get_reads_out(c) == 3
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        ov, _, _, _, release = c.collect_batch(tk)
        rp = c.last_pairs[0].copy()
        assert c.last_reads.consumed == (len(r1), len(r2))
        assert ov.tobytes() == ov0.tobytes() and rp.tobytes() == rp0.tobytes()
        ro = RS.collect_reads_out(c, tk)
        release()
        sel = sorted(int(x) for x in rp["r1_read"])
        assert n // 4 < len(sel) < 3 * n // 4 and ro["flags"] == 0
        exp, n_exp = R.split(r1, r2, sel)
        assert ro["blocks"] == exp and ro["n_records"] == n_exp
        assert RS.tail_split_reads(r1, r2, rp)["blocks"] == exp
        assert R.merge(ro["blocks"][0], ro["blocks"][2], sel, n) == r1
        assert R.merge(ro["blocks"][1], ro["blocks"][3], sel, n) == r2.replace(b"\r\n", b"\n")
        with pytest.raises(kslam.KslamError):   # taken already
            RS.collect_reads_out(c, tk)
        # one stream kind only, then off again
        RS.set_reads_out(c, RS.UNCLASSIFIED)
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        c.collect_batch(tk)[4]()
        assert RS.collect_reads_out(c, tk)["blocks"] == [None, None, exp[2], exp[3]]
        RS.set_reads_out(c, 0)
    finally:
        c.set_pairing(stages=0)
        c.close()
        h1.close()
        h2.close()


def _stream_run(kslam, RS, world, tmp, tag, lanes, host_text=False, bgzf=False, single=False):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = {"KSLAM_LANES": str(lanes)}
    if host_text:
        env["KSLAM_HOST_SAM_TEXT"] = "1"
    os.environ.update(env)
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        names = [str(tmp / ("%s.%d" % (tag, k))) for k in range(4)]
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC) for p in names]
        if single:
            os.close(fds[1]), os.close(fds[3])
            fds[1] = fds[3] = -1
        pr_fd = os.open(str(tmp / (tag + ".per_read")), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        if bgzf:
            RS.set_reads_out_bgzf(c, True)
        P = T.TailParams.default(paired=not single)
        S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300, P, taxdb=tax,
                                 per_read_fd=pr_fd, depth=3, reads_out_fds=fds)
        assert RS.get_reads_out(c) == 0   # the call switched it off again
        for fd in fds + [pr_fd]:
            if fd >= 0:
                os.close(fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    files = [open(p, "rb").read() if fds[k] != -1 else None for k, p in enumerate(names)]
    return files, open(str(tmp / (tag + ".per_read")), "rb").read()


def test_three_batches_through_the_stream(kslam, RS, world, tmp_path):
    """kslam_stream_classify, three batches of 300 pairs, depth 3: the four files are the split of the WHOLE input by the read set
    of the concatenated _PerRead; one lane, three lanes and the host twin's route (KSLAM_HOST_SAM_TEXT=1) write identical files"""
    r1, r2, n = world["case"]["r1"], world["case"]["r2"], world["n"]
    files, per_read = _stream_run(kslam, RS, world, tmp_path, "l3", 3)
    number = {i: k for k, i in enumerate(world["case"]["ids"])}
    sel = [number[line.split(b"\t")[0]] for line in per_read.split(b"\n") if line]
    assert sel == sorted(set(sel)) and n // 4 < len(sel) < 3 * n // 4
    exp, _ = R.split(r1, r2, sel)
    assert files == exp
    for tag, lanes, host in (("l1", 1, False), ("host", 2, True)):
        f, p = _stream_run(kslam, RS, world, tmp_path, tag, lanes, host_text=host)
        assert f == exp and p == per_read, tag
    # BGZF: every file its batches' members and the EOF marker
    z, _ = _stream_run(kslam, RS, world, tmp_path, "z", 2, bgzf=True)
    zh, _ = _stream_run(kslam, RS, world, tmp_path, "zh", 2, host_text=True, bgzf=True)
    for k in range(4):
        assert bgzf_check.check(z[k]) == exp[k] and z[k] == zh[k]


def test_single_end_through_the_stream(kslam, RS, world, tmp_path):
    r1, n = world["case"]["r1"], world["n"]
    files, per_read = _stream_run(kslam, RS, world, tmp_path, "se", 2, single=True)
    number = {i: k for k, i in enumerate(world["case"]["ids"])}
    sel = [number[line.split(b"\t")[0]] for line in per_read.split(b"\n") if line]
    assert 0 < len(sel) < n
    exp, _ = R.split(r1, None, sel)
    assert files == exp and R.merge(files[0], files[2], sel, n) == r1


def test_refusals(kslam, RS, world):
    L = RS.lib()
    c = _indexed_context(kslam, world)
    try:
        assert L.kslam_set_reads_out(c._h, 3) == ERR_STATE          # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        assert L.kslam_set_reads_out(c._h, 0) == 0
        c.set_pairing(stages=3)
        for mask in (4, 7, 255):
            assert L.kslam_set_reads_out(c._h, mask) == kslam.KSLAM_ERR_ARG
        assert RS.get_reads_out(c) == 0
        # a batch submitted by columns: no streams, the alignment as ever, and the context takes the next batch
        case, n = world["case"], world["n"]
        cat = np.frombuffer(b"".join(case["bases"]), dtype=np.uint8)
        qcat = np.frombuffer(b"".join(case["quals"]), dtype=np.uint8)
        off = np.zeros(2 * n + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in case["bases"]], out=off[1:])
        tk = c.submit_batch_columns(2 * n, cat.ctypes.data, qcat.ctypes.data, off.ctypes.data)
        ov0, _, _, _, release = c.collect_batch(tk)
        ov0, rp0 = ov0.copy(), c.last_pairs[0].copy()
        release()
        RS.set_reads_out(c, 3)
        tk = c.submit_batch_columns(2 * n, cat.ctypes.data, qcat.ctypes.data, off.ctypes.data)
        ov, _, _, _, release = c.collect_batch(tk)
        assert ov.tobytes() == ov0.tobytes() and c.last_pairs[0].tobytes() == rp0.tobytes() and len(ov) > 100
        ro = RS.ReadsOut()
        import ctypes
        ro_p = ctypes.byref(ro)
        assert L.kslam_collect_reads_out(c._h, tk, ro_p) == ERR_UNSUPPORTED
        assert b"kslam_submit_batch_fastq_text" in c._L.kslam_last_error(c._h)
        release()
        r1, r2 = case["r1"], case["r2"]
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        release = c.collect_batch(tk)[4]
        rp = c.last_pairs[0].copy()   # (the texts hold other bases than the columns above: half of their pairs are from nowhere)
        release()
        got = RS.collect_reads_out(c, tk)
        exp, n_exp = R.split(r1, r2, sorted(int(x) for x in rp["r1_read"]))
        assert got["n_records"] == n_exp == (len(rp), n - len(rp)) and got["blocks"] == exp and got["blocks"][0]
        h1.close()
        h2.close()
        RS.set_reads_out(c, 0)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        import ctypes as C
        # the ABI hands out no handle to a kslam_multi's contexts: kslam_multi begins with their std::vector, whose first word
        # points at the first of them
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)
        assert L.kslam_set_reads_out(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_set_reads_out_bgzf(h, 1) == ERR_UNSUPPORTED
    finally:
        m.close()
