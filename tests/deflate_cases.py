"""The inputs and histograms that tests/test_deflate_ref.py (CPU) and tests/test_gpu_bgzf_dynamic.py (GPU) share, and the
restatement's bytes for each input, computed once per process."""
import functools
import os

import numpy as np

import deflate_ref as D

M = D.MEMBER_IN
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slam_loop.npz")


@functools.lru_cache(maxsize=None)
def golden_text(tag):
    return np.load(_GOLDEN)[tag + "_sam"].tobytes()


def _text(n):
    t = golden_text("a")
    return (t * (n // len(t) + 1))[:n]


def _pattern(seed, period):
    pat = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8).tobytes()
    return (pat * 8)[:3 * M + 3]


# name -> bytes; every input is at most 3 members and 17 bytes
INPUTS = {
    "empty": lambda: b"",
    "one_byte": lambda: b"x",
    "text_255": lambda: _text(255),              # one thread's range, one tile less a byte: no match is possible
    "text_256": lambda: _text(256),
    "text_257": lambda: _text(257),              # the second tile: the first candidates
    "text_member_less_1": lambda: _text(M - 1),
    "text_member": lambda: _text(M),
    "text_member_plus_1": lambda: _text(M + 1),
    "text_3_members_17": lambda: _text(3 * M + 17),
    "random_3000": lambda: np.random.default_rng(21).integers(0, 256, 3000, dtype=np.uint8).tobytes(),   # no match: two forced distance lengths
    "zeros_member": lambda: bytes(M),
    "all_bytes_x3": lambda: bytes(range(256)) * 3,
    "random_200000": lambda: np.random.default_rng(22).integers(0, 256, 200000, dtype=np.uint8).tobytes(),   # every member stored
    "pattern_32768": lambda: _pattern(23, 32768),   # the window edge: the last distance that fits ...
    "pattern_32769": lambda: _pattern(24, 32769),   # ... and the first that does not
    "ff_200": lambda: b"\xff" * 200,             # lengths 1 1 | 1 1: the header's repeat runs from the literal/length lengths into the distance lengths
}


@functools.lru_cache(maxsize=None)
def data(name):
    return INPUTS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """[(member bytes, MemberReport)] of the restatement"""
    return D.members(data(name), mode)


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _spread(n, pairs):
    c = [0] * n
    for s, v in pairs:
        c[s] = v
    return c


# name -> (counts, limit).  Fibonacci counts make the deepest tree there is: n symbols reach depth n - 1.
HISTOGRAMS = {
    "fib_8": (fib(8), 15), "fib_16": (fib(16), 15),      # depth 15: the last that fits
    "fib_17": (fib(17), 15),                             # depth 16: the first repair
    "fib_22": (fib(22), 15), "fib_30": (fib(30), 15),
    "fib_30_shuffled_in_286": (_spread(286, zip(np.random.default_rng(31).permutation(286)[:30].tolist(), fib(30))), 15),
    "cl_fib_6": (fib(6), 7), "cl_fib_7": (fib(7), 7), "cl_fib_8": (fib(8), 7),   # depth 7 fits, 9 symbols would not
    "cl_fib_19": (fib(19), 7),
    "cl_fib_9": (fib(9), 7),                             # depth 8: the first repair at limit 7
    "equal_286": ([7] * 286, 15), "equal_19": ([3] * 19, 7),
    "one_used_286": (_spread(286, [(65, 9)]), 15), "one_used_is_symbol_0": (_spread(30, [(0, 4)]), 15),
    "one_used_19": (_spread(19, [(18, 2)]), 7),
    "none_used_286": ([0] * 286, 15), "none_used_30": ([0] * 30, 15), "none_used_19": ([0] * 19, 7),
    "ones_and_65280": (_spread(286, [(s, 1) for s in range(0, 286, 3)] + [(32, 65280), (256, 1)]), 15),
    "ones_and_65280_cl": (_spread(19, [(s, 1) for s in range(0, 19, 2)] + [(8, 65280)]), 7),
    "two_symbols": ([5, 0], 15),
    "ties_286": ([1 + (s * 7) % 5 for s in range(286)], 15),
    "steep_286": ([1 << min(s // 10, 24) for s in range(286)], 15),
}
