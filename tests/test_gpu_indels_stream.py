"""The indel table through the lanes (kslam_stream_classify, include/kslam_indels.h): a synthetic world whose reads carry planted
indels inside homopolymers, in batches of 350 pairs with a ragged last one -- one lane, three lanes, the host's SAM text and the
pseudo-assembly left to the host stage.  Every run's file equals, byte for byte, the host twin's file over the concatenated final
arrays; every planted indel stands at its normalised position; and the other outputs of a run do not move with the switch."""
import importlib
import os

import numpy as np
import pytest

import indels_ref as R
from test_gpu_readsplit import _host_text, _indexed_context

pytestmark = pytest.mark.gpu
PER_BATCH = 350


@pytest.fixture(scope="module")
def ID(kslam):
    return importlib.import_module("kslam_amd.indels")


def plant(entry, n_sites=12, spacing=1000, first=700):
    """-> (the entry with one indel per site, [(kind, raw position in the entry, len, bases)]): at each site the nearest homopolymer
    of 3 or more bases loses or gains its LAST base -- the rightmost placement, so that the row stands elsewhere"""
    out, sites, at = bytearray(), [], 0
    for k in range(n_sites):
        p = first + k * spacing
        while not (entry[p] == entry[p - 1] == entry[p - 2] and entry[p + 1] != entry[p] and entry[p] in b"ACGT"):
            p += 1
        if k & 1:
            out += entry[at:p + 1] + entry[p:p + 1]          # one more of the run's base, behind its last
            sites.append((R.INS, p + 1, 1, entry[p:p + 1]))
            at = p + 1
        else:
            out += entry[at:p]                               # the run's last base is gone
            sites.append((R.DEL, p, 1, b""))
            at = p + 1
    out += entry[at:]
    return bytes(out), sites


@pytest.fixture(scope="module")
def indel_world(kslam, synth, tmp_path_factory):
    """tests/test_gpu_readsplit.py's world, but the pairs that came from nowhere there are error-free fragments of entry 0 with the
    planted indels here"""
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    tmp = tmp_path_factory.mktemp("indels")
    n = 900
    case = RL.make_case(synth, n_pairs=n, seed=7311)
    entry = bytes(case["entries"][0]["bases"])
    mutated, sites = plant(entry)
    rng = np.random.default_rng(5)
    bases = list(case["bases"])
    for i in range(1, n, 2):
        ln1, ln2 = len(bases[i]), len(bases[n + i])
        frag = int(rng.integers(max(ln1, ln2) + 20, 380))
        at = int(rng.integers(300, len(mutated) - 300 - frag))
        f = mutated[at:at + frag]
        if rng.random() < 0.5:
            f = R.reverse_complement(f)
        bases[i], bases[n + i] = f[:ln1], R.reverse_complement(f[-ln2:])
    case["r1"] = RL.fastq_text(bases[:n], case["quals"][:n], case["ids"], 1)
    case["r2"] = RL.fastq_text(bases[n:], case["quals"][n:], case["ids"], 2, eol=b"\r\n")
    RL.write_case(case, tmp, D)
    db = D.Database.load(os.path.join(str(tmp), "db", "database"))
    return {"case": case, "db": db, "tmp": tmp, "n": n, "sites": sites, "entry": entry}


def _fastq_bases(text):
    return [line.rstrip(b"\r") for line in text.split(b"\n")[1::4]]


def stream_files(kslam, ID, world, tmp, tag, lanes, env=None, single=False, indels=True):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        names = {k: str(tmp / (tag + "." + k)) for k in ("vcf", "per_read", "sam")}
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        P = T.TailParams.default(paired=not single)
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), PER_BATCH, P, taxdb=tax,
                                      sam_fd=fds["sam"], per_read_fd=fds["per_read"], depth=3, indels_fd=fds["vcf"] if indels else None,
                                      indels_min_alt=1, indels_min_depth=0)
        assert not ID.get_indels(c)   # the call switched it off again
        for fd in fds.values():
            os.close(fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return {k: open(p, "rb").read() for k, p in names.items()}, st


def twin_file(kslam, ID, world, single=False):
    """the same batches through the Python loop, which leaves the SAM text to the host: the final arrays of every batch with its
    CIGAR pool and its reads, concatenated, through the host twin and the VCF writer"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2, n = world["case"]["r1"], world["case"]["r2"], world["n"]
    b1, b2 = _fastq_bases(r1), _fastq_bases(r2)
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    got = []
    try:
        S.classify_stream(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), PER_BATCH,
                          T.TailParams.default(paired=not single), depth=3,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(ov), np.array(cg), np.array(rp), np.array(pr), np.array(reads.bases_off))))
    finally:
        c.close()
        h1.close()
        h2.close()
    assert len(got) == 3      # 350, 350 and a ragged 200
    ents = [bytes(e["bases"]) for e in world["case"]["entries"]]
    gbases = np.frombuffer(b"".join(ents), dtype=np.uint8)
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    whole = None
    for k, (ov, cg, rp, pr, bases_off) in enumerate(got):
        lo, hi = PER_BATCH * k, min(PER_BATCH * (k + 1), n)
        reads = b1[lo:hi] + ([] if single else b2[lo:hi])   # a batch is [R1 block | R2 block]
        roff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        assert roff.tolist() == (bases_off - bases_off[0]).tolist()
        part = {"name": "batch", "gbases": gbases, "goff": goff, "rbases": np.frombuffer(b"".join(reads), dtype=np.uint8), "roff": roff,
                "pool": cg.astype(np.uint32), "ov": ov.astype(R.V.OVERLAP_DT), "rp": rp.astype(R.V.READ_PAIR_DT), "pr": pr.astype(R.V.PAIRED_OVERLAP_DT)}
        whole = part if whole is None else R.concat_cases(whole, part)
    rows, stats = ID.tail_indels(whole["gbases"], whole["goff"], whole["ov"], whole["pool"], whole["rbases"], whole["roff"], whole["rp"], whole["pr"], 1, 0)
    ref_rows, ref_stats = R.table(whole, 1, 0)
    assert R.fields(rows) == ref_rows and stats == ref_stats and stats["n_skipped"] == 0 and stats["n_deletions"] > 100 and stats["n_insertions"] > 100
    return ID.report_bytes(world["db"], rows, stats), rows


def planted_rows(world):
    """the keys the planted indels must stand at: normalised against the unmutated entry"""
    return [(0,) + R.normalised(world["entry"], kind, p, n, s) for kind, p, n, s in world["sites"]]


def test_batches_through_the_stream(kslam, ID, indel_world, tmp_path):
    world = indel_world
    exp, rows = twin_file(kslam, ID, world)
    plain, _ = stream_files(kslam, ID, world, tmp_path, "plain", 1, indels=False)
    assert plain["vcf"] == b""
    files, st = stream_files(kslam, ID, world, tmp_path, "l1", 1)
    assert files["vcf"] == exp and st["batches_pseudo_on_host"] == 0
    assert files["sam"] == plain["sam"] and files["per_read"] == plain["per_read"] and len(plain["sam"]) > 10000   # nothing else moves
    assert stream_files(kslam, ID, world, tmp_path, "l3", 3)[0]["vcf"] == exp
    assert stream_files(kslam, ID, world, tmp_path, "host", 2, env={"KSLAM_HOST_SAM_TEXT": "1"})[0]["vcf"] == exp
    # pseudo-assembly left to the host for every batch: the keys come in through kslam_indels_add on the host stage's thread
    left, st = stream_files(kslam, ID, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st["batches_pseudo_on_host"] == 3 and left["vcf"] == exp
    # every planted indel at its normalised position -- which is not where it was planted
    have = {r[:5]: r for r in R.fields(rows)}
    for key, (kind, p, n, s) in zip(planted_rows(world), world["sites"]):
        assert key in have and key[1] < p - 2, (key, p)
        assert have[key][5] + have[key][6] >= 2 and have[key][5] > 0 and have[key][6] > 0
    name = str(tmp_path / "l1.vcf")
    parsed = ID.parse(name)
    assert len(parsed) == len(rows) and {r["type"] for r in parsed} == {"del", "ins"}


def test_single_end_through_the_stream(kslam, ID, indel_world, tmp_path):
    exp, rows = twin_file(kslam, ID, indel_world, single=True)
    assert len(rows) > 50
    assert stream_files(kslam, ID, indel_world, tmp_path, "se", 2, single=True)[0]["vcf"] == exp
