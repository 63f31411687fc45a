"""Inputs for the tests of the Zstandard encoder's `long` word (tests/test_zstd_long_host.py,
tests/test_gpu_zstd_long.py, tests/golden/make_zstd_long_kat.py), and a plain-Python restatement of the
long-distance matcher defined at the top of dwarfs_amd/csrc/zstd_long_host.cpp.  Every family is built from seeded
random bytes, so nothing but the planted copies can match."""

import functools

import numpy as np

import zstd_enc_adaptive_cases as AC

CHUNK = 32768
WINDOW, GRID, MIN_MATCH, SHORT_MIN = 32, 32, 64, 4
EMPTY = 0xFFFFFFFF
PAIRS = ((0, 0), (0, 8 | 0x100), (3, 0), (3, 8 | 0x100))  # (options, search)
GAPS = (1, 31, 33, 65535, 65536, 100001)
SIZES = (0, 1, 63, 64, 95, 32768, 32769)


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def plant(buf, dst, src, length):
    buf[dst:dst + length] = buf[src:src + length]


def far_copies():
    R = rnd(100, 81920)
    out = [("far_rr", R + R)]
    for i, gap in enumerate(GAPS):
        out.append((f"far_gap_{gap}", R + rnd(200 + i, gap) + R))
    return out


def partial_copies():
    out = []
    for length, src in ((63, 1003), (64, 1003), (95, 1003), (64, 993), (64, 1024)):  # (993 = 31 * 32 + 1)
        b = bytearray(rnd(300 + length + src, 150000))
        plant(b, 120011, src, length)
        out.append((f"partial_{length}_from_{src}", bytes(b)))
    return out


def chunk_ends():
    b = bytearray(rnd(400, 4 * CHUNK))
    plant(b, 3 * CHUNK - 2000, 5000, 4000)  # spans a chunk's end: cut there, picked up again behind it
    c = bytearray(rnd(401, 3 * CHUNK + 200))
    plant(c, 3 * CHUNK - 40, 77, 140)  # 40 bytes before the end (not kept), 100 behind it (kept)
    return [("chunk_end_4000", bytes(b)), ("chunk_end_40_100", bytes(c))]


def mixed(seed, n=5 * CHUNK + 1234):
    """A far half with short-range repeats in and around its far copies, so that the merge trims heads and tails."""
    rng = np.random.default_rng(seed)
    b = bytearray(rnd(seed + 1, n))
    half = n // 2
    for _ in range(60):  # short-range repeats in the first half, which the far copies carry along
        length, back = int(rng.integers(4, 200)), int(rng.integers(1, 3000))
        dst = int(rng.integers(back, half - length))
        plant(b, dst, dst - back, length)
    for _ in range(40):  # far copies into the second half
        length = int(rng.integers(40, 3000))
        src = int(rng.integers(0, half - 70000 - length)) if half > 70000 + length + 1 else 0
        dst = int(rng.integers(half, n - length))
        if dst - src > 65535:
            plant(b, dst, src, length)
    for _ in range(120):  # short-range repeats across the far copies' ends
        length, back = int(rng.integers(4, 300)), int(rng.integers(1, 2000))
        dst = int(rng.integers(half, n - length))
        plant(b, dst, dst - back, length)
    return bytes(b)


def both_sides():
    """A short match of 100 bytes (offset 300) whose bytes 20 .. 90 also stand far back, on the grid, where the two
    copies of the 100 bytes do not: the long match takes the middle, the merge keeps a head of 20 and a tail of 10."""
    b, T = bytearray(rnd(900, 200000)), rnd(901, 100)
    b[3200:3270] = T[20:90]
    for at in (96002, 96302):
        b[at:at + 100] = T
    return [("both_sides", bytes(b))]


def first_occurrence():
    R, parts = rnd(500, 20000), [rnd(501 + i, 70000) for i in range(3)]
    return [("three_copies", parts[0] + R + parts[1] + R + parts[2] + R)]


def no_ops():
    return [("zeros_100000", bytes(100000)), ("period_7", bytes(range(7)) * 15000)]


def sizes():
    return [(f"size_{n}", rnd(600 + n, n)) for n in SIZES] + [(f"zeros_{n}", bytes(n)) for n in SIZES]


@functools.lru_cache(maxsize=None)
def own_inputs():
    """[(name, data)]: the families of this file"""
    return (far_copies() + partial_copies() + chunk_ends() + [(f"mixed_{s}", mixed(s)) for s in (700, 701, 702)] +
            both_sides() + first_occurrence() + no_ops() + sizes())


@functools.lru_cache(maxsize=None)
def inputs():
    """... and the 116 inherited ones behind them"""
    return own_inputs() + list(AC.inputs())


FAR = tuple(name for name, _ in far_copies())


@functools.lru_cache(maxsize=None)
def reach_20():
    """1.5 MiB whose last 64 KiB repeat its first: an offset code of 20"""
    R = rnd(800, 3 * CHUNK // 2 * 32)
    return R[:-65536] + R[:65536]


# ---------------------------------------------------------------------------
# the matcher, restated
# ---------------------------------------------------------------------------
def long_hash(window):
    h = 0
    for w in np.frombuffer(window, "<u4").tolist():
        h = ((((h << 5) | (h >> 27)) & 0xFFFFFFFF) ^ w) * 2654435761 & 0xFFFFFFFF
    h ^= h >> 16
    return h * 0x85EBCA6B & 0xFFFFFFFF


def table_log(n):
    log = 6
    while (1 << log) < n // 16:
        log += 1
    return log


def all_hashes(data):
    """long_hash of the window at every position 0 .. n - WINDOW, all at once (the same arithmetic in uint64)"""
    a = np.frombuffer(data, np.uint8).astype(np.uint64)
    words = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
    count, mask = len(data) - WINDOW + 1, np.uint64(0xFFFFFFFF)
    h = np.zeros(count, np.uint64)
    for k in range(WINDOW // 4):
        h = ((((h << np.uint64(5)) | (h >> np.uint64(27))) & mask) ^ words[4 * k:4 * k + count]) * np.uint64(2654435761) & mask
    h ^= h >> np.uint64(16)
    return h * np.uint64(0x85EBCA6B) & mask


def find_long(data):
    """[(pos, len, off)] of the block's long matches"""
    n, out = len(data), []
    if n < MIN_MATCH + 5:
        return out
    log = table_log(n)
    slots = (all_hashes(data) >> np.uint64(32 - log)).astype(np.int64)
    assert int(slots[0]) == long_hash(data[:WINDOW]) >> (32 - log)  # (the scalar form agrees)
    tab = np.full(1 << log, EMPTY, np.int64)
    grid = np.arange(0, n - WINDOW + 1, GRID)
    np.minimum.at(tab, slots[grid], grid)  # the lowest position of every entry
    cand = tab[slots]
    earlier = np.nonzero(cand < np.arange(len(slots)))[0].tolist()  # positions whose entry holds some q < p
    cursor = 0
    for p in earlier:
        cs = p // CHUNK * CHUNK
        lim_end = min(cs + CHUNK, n - 5)
        cursor = max(cursor, cs)  # (a chunk's cursor starts at its start)
        q = int(cand[p])
        if p < cursor or p + WINDOW > lim_end or data[q:q + WINDOW] != data[p:p + WINDOW]:
            continue
        fwd, back = WINDOW, 0
        while p + fwd < lim_end and data[q + fwd] == data[p + fwd]:
            fwd += 1
        while p - back - 1 >= cursor and q - back >= 1 and data[q - back - 1] == data[p - back - 1]:
            back += 1
        if fwd + back >= MIN_MATCH:
            out.append((p - back, fwd + back, p - q))
            cursor = p + fwd
    return out


def merge(shorts, longs, stats=None):
    """The final list: every long match, every short match clear of them, and heads and tails of the others."""
    out = list(longs)
    for a, length, off in shorts:
        b = a + length
        over = [(p, p + m) for p, m, _ in longs if p < b and p + m > a]
        if not over:
            out.append((a, length, off))
            continue
        head, tail = over[0][0] - a, b - over[-1][1]
        if head >= SHORT_MIN:
            out.append((a, head, off))
        if tail >= SHORT_MIN:
            out.append((over[-1][1], tail, off))
        if stats is not None:
            stats[("head" if head >= SHORT_MIN else "") + ("tail" if tail >= SHORT_MIN else "") or "gone"] += 1
    return sorted(out)
