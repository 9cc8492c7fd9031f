"""kslam_stream_classify with EVERY opt-in output at once (host/stream.cpp: the eight file reports, the reads split and the reads
of chosen taxa): each file is byte for byte the one the same call writes with that output alone, on the route where the lanes
feed the reports and on the routes that leave the batch to the host stage; whatever the call's end, it leaves every switch off and
every per-call descriptor and parameter at its default.  The world of tests/test_gpu_readsplit.py, three batches of 300 pairs."""
import ctypes as C
import importlib
import os

import pytest

from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
ERR_STATE = 5   # include/kslam.h: kslam_status
# an output and the files it writes; non-default parameters, so that "back to the defaults" below says something
OUTPUTS = {"coverage": ["coverage"], "genes": ["genes"], "kreport": ["kreport"], "variants": ["vcf"], "consensus": ["fasta"],
           "read_qc": ["read_qc"], "align_qc": ["align_qc"], "depth": ["bedgraph"], "reads_out": ["c1", "c2", "u1", "u2"],
           "taxon_reads": ["x1", "x2"]}
ALWAYS = ["sam", "per_read"]
PARAMS = dict(variants_min_alt=1, variants_min_depth=2, consensus_params=(2, 600, 1, 2), depth_min=2, read_qc_max_cycles=100, align_qc_max_cycles=120)
ROUTES = {"lanes": {"KSLAM_LANES": "3"}, "host_text": {"KSLAM_LANES": "2", "KSLAM_HOST_SAM_TEXT": "1"},
          "host_pseudo": {"KSLAM_LANES": "2", "KSLAM_PSEUDO_CAP": "3"}}
# (the routes of tests/test_gpu_stream.py that leave work to the host; the cap at which this world's batches are handed back whole,
# as in the per-report stream tests)


def _modules():
    return {k: importlib.import_module("kslam_amd." + k) for k in ("stream", "tail", "taxonomy", "samtext", "readsplit", "taxreads", "coverage", "genes",
                                                                  "kreport", "variants", "consensus", "readqc", "alignqc", "depth")}


def _call(M, c, world, texts, tax, tmp, tag, wanted, chosen, with_tree=True, per_batch=300, params=None, header=b"@HD\tVN:1.0\n", report=None,
          instead=None):
    """one kslam_stream_classify with the outputs in `wanted` -> ({file: bytes}, statistics).  texts: ((R1 buffer, bytes), (R2
    buffer or None for single-end data, bytes)); params: the tail's parameters (default: paired, everything else as SLAM's);
    instead: {file: descriptor} the caller opened itself (and closes), used in place of the file of that name"""
    (h1, n1), (h2, n2) = texts
    single = h2 is None
    names = {f: str(tmp / (tag + "." + f)) for o in wanted for f in OUTPUTS[o] if not (single and f[-1] == "2")}
    names.update({f: str(tmp / (tag + "." + f)) for f in ALWAYS})
    own = {f: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for f, p in names.items()}
    fds = dict(own, **(instead or {}))
    fd = lambda o: fds[OUTPUTS[o][0]] if o in wanted else -1   # noqa: E731
    if "taxon_reads" in wanted:   # the chosen ids hold for one call
        M["samtext"].set_annotations(c, world["db"], tax)
        c.set_pairing(stages=7)
        M["taxreads"].set_taxon_reads(c, chosen, M["taxreads"].CHILDREN)
    try:
        st = M["stream"].classify_stream_native(
            c, world["db"], h1.ptr, n1, None if single else h2.ptr, n2, per_batch, params if params is not None else M["tail"].TailParams.default(paired=True),
            taxdb=tax if with_tree else None, report=report,
            sam_fd=fds["sam"], per_read_fd=fds["per_read"] if with_tree else -1, sam_header=header, depth=3,
            coverage_fd=fd("coverage"), genes_fd=fd("genes"), kreport_fd=fd("kreport"), variants_fd=fd("variants"), consensus_fd=fd("consensus"),
            read_qc_fd=fd("read_qc"), align_qc_fd=fd("align_qc"), depth_fd=fd("depth"),
            reads_out_fds=[fds.get(f, -1) for f in OUTPUTS["reads_out"]] if "reads_out" in wanted else None,
            taxon_reads_fds=[fds.get(f, -1) for f in OUTPUTS["taxon_reads"]] if "taxon_reads" in wanted else None, **PARAMS)
    finally:
        for f in own.values():
            os.close(f)
    return {f: open(p, "rb").read() for f, p in names.items()}, st


def _assert_put_away(M, c):
    """every switch off, every per-call descriptor -1 and every per-call parameter at its default"""
    L = M["depth"].lib()
    assert not M["coverage"].get_coverage(c) and not M["genes"].get_genes(c) and not M["kreport"].get_kreport(c)
    assert not M["variants"].get_variants(c) and not M["consensus"].get_consensus(c) and not M["depth"].get_depth(c)
    assert M["readqc"].get_read_qc(c) == (False, 0) and M["alignqc"].get_align_qc(c) == (False, 0)
    assert M["readsplit"].get_reads_out(c) == 0 and len(M["taxreads"].get_taxon_reads(c)[0]) == 0
    fd, a, b = C.c_int(5), C.c_uint32(77), C.c_uint32(77)
    for name in ("coverage", "genes", "kreport"):
        fd.value = 5
        assert getattr(L, "kslam_stream_get_" + name)(c._h, C.byref(fd)) == 0 and fd.value == -1, name
    for name, default in (("depth", 1), ("read_qc", 0), ("align_qc", 0)):
        fd.value, a.value = 5, 77
        assert getattr(L, "kslam_stream_get_" + name)(c._h, C.byref(fd), C.byref(a)) == 0 and (fd.value, a.value) == (-1, default), name
    fd.value = 5
    assert L.kslam_stream_get_variants(c._h, C.byref(fd), C.byref(a), C.byref(b)) == 0 and (fd.value, a.value, b.value) == (-1, 2, 1)
    fd.value, p = 5, M["consensus"].Params(9, 9, 9, 9)
    assert L.kslam_stream_get_consensus(c._h, C.byref(fd), C.byref(p)) == 0
    assert (fd.value, p.min_depth, p.call_permille, p.fill, p.min_covered) == (-1, 1, 500, M["consensus"].FILL_N, 1)
    four, two = (C.c_int * 4)(5, 5, 5, 5), (C.c_int * 2)(5, 5)
    assert L.kslam_stream_get_reads_out(c._h, C.byref(four)) == 0 and list(four) == [-1] * 4
    assert L.kslam_stream_get_taxon_reads(c._h, C.byref(two)) == 0 and list(two) == [-1] * 2


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_output_at_once_is_each_output_alone(kslam, world, tmp_path, monkeypatch, route):
    M = _modules()
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    texts = ((h1, len(r1)), (h2, len(r2)))
    tax = M["taxonomy"].TaxDB(world["case"]["taxdb"])
    try:
        plain, st = _call(M, c, world, texts, tax, tmp_path, "plain", [], None)
        _assert_put_away(M, c)
        assert st["n_batches"] == 3 and st["batches_pseudo_on_host"] == (3 if route == "host_pseudo" else 0)
        ids = [int(x) for x in st["tax_ids"] if x]
        chosen = [max(set(ids), key=ids.count)]
        both, st_all = _call(M, c, world, texts, tax, tmp_path, "all", list(OUTPUTS), chosen)
        _assert_put_away(M, c)
        assert st_all["batches_pseudo_on_host"] == st["batches_pseudo_on_host"] and st_all["tax_ids"].tolist() == st["tax_ids"].tolist()
        assert all(both[f] == plain[f] for f in ALWAYS)
        for output, files in OUTPUTS.items():
            alone, _ = _call(M, c, world, texts, tax, tmp_path, output, [output], chosen)
            _assert_put_away(M, c)
            for f in files + ALWAYS:
                assert both[f] == alone[f], (output, f)
            assert all(len(alone[f]) > 0 for f in files), output   # (every stream of this world has records: the files say something)
    finally:
        c.close()
        h1.close()
        h2.close()
        tax.close()


def test_a_call_refused_in_set_up_puts_everything_away(kslam, world, tmp_path, monkeypatch):
    """the Kraken-style report without a tree is refused behind the arming of coverage, variants, consensus, depth and the two QC
    reports: they are off again, no per-call setting is left behind and no file has grown"""
    M = _modules()
    monkeypatch.setenv("KSLAM_LANES", "2")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    wanted = [o for o in OUTPUTS if o not in ("reads_out", "taxon_reads")]
    try:
        with pytest.raises(kslam.KslamError) as e:
            _call(M, c, world, ((h1, len(r1)), (h2, len(r2))), None, tmp_path, "refused", wanted, None, with_tree=False)
        assert e.value.status == ERR_STATE and "the Kraken-style report needs a taxonomy tree" in str(e.value)
        _assert_put_away(M, c)
        for o in wanted:
            for f in OUTPUTS[o]:
                assert os.path.getsize(str(tmp_path / ("refused." + f))) == 0, f
        # and the context is good for the next call
        files, st = _call(M, c, world, ((h1, len(r1)), (h2, len(r2))), None, tmp_path, "after", ["coverage", "depth"], None, with_tree=False)
        assert st["n_batches"] == 3 and len(files["coverage"]) > 0 and len(files["bedgraph"]) > 0
        _assert_put_away(M, c)
    finally:
        c.close()
        h1.close()
        h2.close()
