"""The indexes that put every seam of the one-time index build under one of its own kernels, and the routes of the build.

Shared by tests/test_index_ref.py (CPU: each family reaches the seam it is named for) and tests/test_gpu_index_build.py
(GPU: kslam_debug_index_export against tests/index_ref.py).  An index is a list of bytes, one per entry; every index is
built once per process and never changed.

Test infrastructure only (CPU, numpy).
"""
import functools

import numpy as np

import index_ref as R

K, GAP = R.K, R.GAP
SEG_KMERS = 128          # common.h: k-mers per extraction segment
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand(rng, n):
    return np.frombuffer(b"ACTG", dtype=np.uint8)[rng.integers(0, 4, int(n))].tobytes()


def revcomp(s):
    return s.translate(_COMP)[::-1]


def length_for(k):
    """the shortest entry with k k-mers"""
    return K + GAP * (k - 1) if k else 0


def words(rng, n):
    """n distinct 32-mers, none its own reverse complement"""
    out = []
    while len(out) < n:
        w = rand(rng, K)
        if w != revcomp(w) and w not in out and revcomp(w) not in out:
            out.append(w)
    return out


# ---- lengths ----------------------------------------------------------------------------------------------------------------
NAMED_LENGTHS = (0, 1, 31, 32, 33, 47, 48, 49, 2063, 2064, 2065, 2079, 2080, K + GAP * 8191, K + GAP * 8192)


def lengths_index():
    """Every named length; sixteen entries of 33 bases (one k-mer each) come first, so that an entry WITH k-mers starts
    at every residue mod 16, and entries of 1, 31 and 33 bases between the long ones move those over the residues mod 4."""
    rng = np.random.default_rng(101)
    lens = [33] * 16 + [0, 1, 31, 32, 47, 48, 49, 2063, 2064, 1, 2065, 31, 2079, 33, 1, K + GAP * 8191, 33, 2080, 1, 1,
                        K + GAP * 8192, 49, 32]
    return [rand(rng, n) for n in lens]


# ---- record count -----------------------------------------------------------------------------------------------------------
M_VALUES = (255, 256, 257, 4095, 4096, 4097)


def record_count_index(m):
    """two small entries (5 and 2 k-mers) and one whose length is tuned to m records in all; 5 spare bases at its end.
    One 32-mer is in all three entries and another in two of them, on either strand."""
    rng = np.random.default_rng(200 + m)
    w0, w1 = words(rng, 2)
    tuned = rand(rng, length_for(m - 7) + 5)
    return [w0 + w1 + rand(rng, 36), revcomp(w1) + w0 + tuned[64:], revcomp(w0) + revcomp(w1)[:18]]


# ---- ids --------------------------------------------------------------------------------------------------------------------
ID_COUNTS = (1, 128, 129, 257, 32768, 32769)
PLANT_AT = (0, 127, 128, 255, 256, 32767, 32768)
N_PLANTED = 12


def ids_index(n):
    """n entries.  Up to 257 entries they are of 1100-1200 bases (more than 64 k-mers each: the sort's run histogram is on);
    32 768 and 32 769 entries are of 48-64 bases, most of them 64 (more than 2^20 / 12 records: the automatic filter grows
    to 2^21 bits).  The entries PLANT_AT that exist are longer than that rule: each carries the same twelve 32-mers at
    sampled offsets, forward or reverse-complemented by turns, because one entry of 64 bases has room for three k-mers
    only and the equal-key groups have to differ in every meta pass's digit ten times over.  The last planted entry also
    carries twelve 32-mers of its own on both strands: groups that differ in the revComp bit alone."""
    rng = np.random.default_rng(300 + n)
    if n <= 257:
        lens = rng.integers(1100, 1201, n)
    else:
        lens = np.where(rng.random(n) < 0.85, 64, rng.integers(48, 64, n))
    entries = [rand(rng, L) for L in lens]
    shared, own = words(rng, N_PLANTED), words(rng, N_PLANTED)
    planted = [e for e in PLANT_AT if e < n]
    for p, e in enumerate(planted):
        body = b"".join(w if (p + j) % 2 == 0 else revcomp(w) for j, w in enumerate(shared))
        if e == planted[-1]:
            body += b"".join(w + revcomp(w) for w in own)
        entries[e] = body
    return entries


# ---- ratio switches ---------------------------------------------------------------------------------------------------------
UNIFORM_PLANT_AT = (0, 7, 19, 39)


def uniform_index(k, n=40):
    """n entries of exactly k k-mers each: meta_digits_in_runs is m / n >= 64.  Four of them begin with the same twelve
    32-mers, forward or reverse-complemented by turns: without equal keys in different entries the order the meta passes
    make could not be seen at all."""
    rng = np.random.default_rng(400 + k)
    entries = [rand(rng, length_for(k) + int(rng.integers(0, GAP))) for _ in range(n)]
    shared = words(rng, N_PLANTED)
    for p, e in enumerate(UNIFORM_PLANT_AT):
        body = b"".join(w if (p + j) % 2 == 0 else revcomp(w) for j, w in enumerate(shared))
        entries[e] = body + entries[e][len(body):]
    return entries


def segments_index(extra):
    """8 entries of 4 segments each (385 to 512 k-mers), so that n_segs == 4 n: the one-thread-per-entry segment fill; with
    `extra` the last entry has 513 k-mers, a fifth segment, and the wave-per-entry fill takes over"""
    rng = np.random.default_rng(450)
    ks = [385, 512, 400, 511, 386, 450, 512, 513 if extra else 512]
    return [rand(rng, length_for(k) + 3) for k in ks]


def n_segments(entries):
    return int(sum(-(-k // SEG_KMERS) for k in R.kmers_per_entry(entries)))


# ---- content ----------------------------------------------------------------------------------------------------------------
TANDEM_RECORDS = 4200
LAST_BUCKET_PALINDROME = b"G" * 16 + b"C" * 16


def _junk_entry(rng):
    """runs of N and of lower case laid across k-mer boundaries (offsets 16 i), and single ones inside k-mers"""
    s = bytearray(rand(rng, 1200))
    for a, b in ((14, 18), (31, 33), (60, 70), (127, 129), (250, 300), (511, 513)):
        s[a:b] = b"N" * (b - a)
    for a, b in ((90, 100), (158, 162), (400, 440), (639, 641)):
        s[a:b] = bytes(s[a:b]).lower()
    for p in (200, 333, 700, 1199):
        s[p] = ord("n")
    for p, ch in ((720, b"U"), (721, b"u"), (760, b"R"), (800, b"-"), (801, b"@"), (802, b"[")):
        s[p] = ch[0]
    return bytes(s)


def content_index():
    rng = np.random.default_rng(500)
    twice = rand(rng, 3000)
    pal = bytearray(rand(rng, 32 * 40))
    for j in range(0, 40, 2):                                # palindromic 32-mers at sampled offsets
        h = rand(rng, 16)
        pal[32 * j:32 * j + 32] = h + revcomp(h)
    pal[32 * 7:32 * 8] = LAST_BUCKET_PALINDROME
    unit = rand(rng, 16)
    return [b"A" * 500, twice, b"T" * 500, _junk_entry(rng), bytes(pal), twice, unit * (2 + TANDEM_RECORDS - 1) + unit[:7],
            rand(rng, 5000)]


def sparse_index():
    """a handful of distinct keys: at 2^20 filter bits (four blocks) some block receives no word"""
    unit = np.random.default_rng(510).integers(0, 4, 16)
    unit = np.frombuffer(b"ACTG", dtype=np.uint8)[unit].tobytes()
    return [b"A" * 200, b"T" * 200, LAST_BUCKET_PALINDROME * 2, unit * 20]


# ---- empty ------------------------------------------------------------------------------------------------------------------
def short_only_index():
    rng = np.random.default_rng(600)
    return [rand(rng, n) for n in (0, 31, 1, 17, 31, 0, 5)]


_BUILDERS = {"lengths": lengths_index, "content": content_index, "sparse": sparse_index,
             "uniform/63": lambda: uniform_index(63), "uniform/64": lambda: uniform_index(64),
             "segments/4n": lambda: segments_index(False), "segments/4n+1": lambda: segments_index(True),
             "empty/no_entries": lambda: [], "empty/short_only": short_only_index}
_BUILDERS.update({"m/%d" % m: functools.partial(record_count_index, m) for m in M_VALUES})
_BUILDERS.update({"ids/%d" % n: functools.partial(ids_index, n) for n in ID_COUNTS})
NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def index(name):
    return tuple(_BUILDERS[name]())


@functools.lru_cache(maxsize=None)
def sorted_records(name):
    recs = R.records(index(name))
    return recs[R.order(recs)]


# ---- routes -----------------------------------------------------------------------------------------------------------------
# name -> (environment, KSLAM_BUCKET_BITS_EXACT or None, KSLAM_FILTER_BITS or None, through kslam_set_index_device)
BIG_BUCKET_BITS = 20          # well above log2 m of every index that takes it (m <= 2^15)
ROUTES = {
    "default": ({}, None, None, False),
    "atomics": ({"KSLAM_FILTER_BUILD": "atomics"}, None, None, False),
    "no_digit_bytes": ({"KSLAM_SORT_DIGIT_BYTES": "0"}, None, None, False),
    "filter_bits/0": ({"KSLAM_FILTER_BITS": "0"}, None, 0, False),
    "filter_bits/20": ({"KSLAM_FILTER_BITS": "20"}, None, 20, False),
    "filter_bits/21": ({"KSLAM_FILTER_BITS": "21"}, None, 21, False),
    "filter_bits/28": ({"KSLAM_FILTER_BITS": "28"}, None, 28, False),
    "bucket_bits/8": ({"KSLAM_BUCKET_BITS_EXACT": "8"}, 8, None, False),
    "bucket_bits/12": ({"KSLAM_BUCKET_BITS_EXACT": "12"}, 12, None, False),
    "bucket_bits/%d" % BIG_BUCKET_BITS: ({"KSLAM_BUCKET_BITS_EXACT": str(BIG_BUCKET_BITS)}, BIG_BUCKET_BITS, None, False),
    "device": ({}, None, None, True),
}
DEVICE_FIRST_OFFSET = 7       # not 0 and not a multiple of 4

_SORT_AND_FILTER = ("atomics", "no_digit_bytes", "filter_bits/0", "filter_bits/20", "filter_bits/21")
_BUCKETS = ("bucket_bits/8", "bucket_bits/12", "bucket_bits/%d" % BIG_BUCKET_BITS)


def routes_of(name):
    """each route on the families where it changes a kernel"""
    r = ["default"]
    if name in ("lengths", "content", "sparse", "uniform/63", "uniform/64", "ids/129", "ids/257", "ids/32769", "segments/4n+1",
                "empty/short_only") or name.startswith("m/"):
        r += _SORT_AND_FILTER                    # the sort's first digits, the split (fused or not) and either filter build
    if name in ("content", "m/4097"):
        r.append("filter_bits/28")               # two sort passes over the probe words
    if name in ("lengths", "content", "sparse", "ids/257", "m/256", "m/257", "m/4096", "m/4097", "empty/short_only"):
        r += _BUCKETS                            # the bucket fill, fused or not
    if name in ("lengths", "content", "m/257", "ids/129", "empty/no_entries"):
        r.append("device")                       # the upload
    return r


CASES = [(name, route) for name in NAMES for route in routes_of(name)]


@functools.lru_cache(maxsize=None)
def expected(name, route):
    _env, bucket_exact, filter_env, _dev = ROUTES[route]
    return R.build(list(index(name)), bucket_exact, filter_env, sorted_recs=sorted_records(name))


def reads_of(name, n=8, length=100):
    """a few reads cut from the index's entries (every other one reverse-complemented), and one that is in no entry"""
    entries = index(name)
    rng = np.random.default_rng(700)
    have = [i for i, e in enumerate(entries) if len(e) >= K]
    pick = sorted(set(have[:2] + have[-2:] + [have[int(j)] for j in rng.integers(0, len(have), n)])) if have else []
    reads = []
    for j, i in enumerate(pick[:n]):
        e = entries[i]
        a = int(rng.integers(0, max(1, len(e) - length + 1)))
        s = e[a:a + length]
        reads.append(revcomp(s) if j % 2 else s)
    reads.append(rand(rng, length))
    return reads
