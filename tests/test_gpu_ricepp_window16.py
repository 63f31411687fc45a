"""The fused decode's narrow fast-loop instance (fs 5..7, bs 128: 64 lane segments of 16 bits, ricepp_decode_fused.hip
``W16``) on constructed streams (tests/ricepp_build.py): sub-blocks that end around the end of its 1024-bit window,
terminators on every bit of a segment with all-ones remainders, three terminators per segment and empty segments,
and the hand-over to the 24-bit instance and back.

Every stream is decoded on the default and the ``fused`` path as tests/test_gpu_ricepp_constructed.py decodes its
families (0xFF behind every stream, guard samples between the outputs) and compared with the samples its field list
stands for; ``test_cases_match_oracle`` (no GPU) holds the same streams and samples against the CPU oracle and checks
that the families reach what they aim at.

The kernel's geometry is restated below only to aim the cases, never to compute a sample.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import ricepp_build as B
from ricepp_build import Cfg, Fields, Rice, Zero

WIN16 = 64 * 16   # ricepp_decode_fused.hip kWin16Bits
K_RETURN = 8      # ricepp_decode_fused.hip kW16Return
BS = 128
EDGE_LENGTHS = range(WIN16 - 12, WIN16 + 12 + 1)
PATHS = ["auto", "fused"]


def shortest(fs: int) -> int:
    return 4 + BS * (fs + 1)


def sized(rng, fs: int, bits: int, grow: str = "spread", ones: bool = False, n: int = BS) -> Rice:
    """A Rice sub-block of n codes that is exactly ``bits`` long, header included: short runs as an encoder that
    chose fs writes them, then the run of one code lengthened (``last``: the last code's, ``early``: code 3's) or the
    rest spread over all (``spread``).  ``ones``: every remainder all ones."""
    slack = bits - 4 - n * (fs + 1)
    assert slack >= 0, (fs, bits)
    q = np.minimum(rng.geometric(0.6, n) - 1, 5)
    while q.sum() > (slack if grow == "spread" else slack // 2):  # (leave the lengthened run at least half)
        q[int(rng.integers(n))] //= 2
    rest = slack - int(q.sum())
    if grow == "last":
        q[n - 1] += rest
    elif grow == "early":
        q[3] += rest
    else:
        q += np.asarray(B._spread(rng, rest, n))
    r = [(1 << fs) - 1] * n if ones else rng.integers(0, 1 << fs, n).tolist()
    return Rice(fs, tuple(zip(q.tolist(), r)))


def fit(rng, fs: int = 6) -> Rice:
    """A sub-block the narrow window holds, of a typical length (Poisson(1000): 985 bits at fs 6)."""
    return sized(rng, fs, max(shortest(fs), int(rng.integers(960, 1005))))


def long_(rng, fs: int = 6) -> Rice:
    """A sub-block whose last terminator lies behind the narrow window (and inside the 1536-bit one)."""
    return sized(rng, fs, int(rng.integers(WIN16 + 8 + 8, WIN16 + 120)))


def last_term(sub: Rice) -> int:
    """The last terminator's bit, counted from the sub-block's header."""
    return 4 + sum(q for q, _ in sub.codes) + len(sub.codes) * (sub.fs + 1) - 1 - sub.fs


def fits(sub) -> bool:
    return isinstance(sub, Rice) and 5 <= sub.fs <= 7 and len(sub.codes) == BS and last_term(sub) < WIN16


@functools.lru_cache(maxsize=None)
def edge_fields():
    """fs 5, 6, 7; every length from 1024 - 12 to 1024 + 12 that 128 codes can have (fs 7: from its shortest, 1028);
    reached by the last code's run and by an early one's; stream misalignments 0..3.  A typical sub-block before (the
    aimed one is parsed in the loop, its window read behind the one before) and two behind."""
    rng = np.random.default_rng(1016)
    out = []
    for fs in (5, 6, 7):
        for bits in EDGE_LENGTHS:
            if bits < shortest(fs):
                continue
            for grow in ("last", "early"):
                for mis in range(4):
                    first = (bits + mis + (grow == "early")) % 2 == 0  # (also as the stream's first: the prologue)
                    aimed = sized(rng, fs, bits, grow)
                    subs = ([] if first else [fit(rng)]) + [aimed, fit(rng, fs if fs < 7 else 6), fit(rng)]
                    out.append((f"edge16 fs={fs} bits={bits} {grow} mis={mis} first={first}", Cfg(BS),
                                Fields((513,), tuple(subs)), mis, aimed))
    return out


@functools.lru_cache(maxsize=None)
def reach_fields():
    """All-ones remainders behind a terminator on every bit of a segment.  fs 7: the first run 0..7 moves every
    terminator of a q = 0 sub-block over the bits 4..11 (and 12..15, 0..3 of the next segment) -- up to 3 the narrow
    window holds it, and with 3 the last terminator is bit 15 of lane 63's segment.  fs 6 has room for all 16 shifts
    inside the narrow window: codes of 8 bits (q = 1) behind a first run of 0..15."""
    rng = np.random.default_rng(1631)
    out = []
    for shift in range(8):
        aimed = Rice(7, ((shift, 127),) + ((0, 127),) * (BS - 1))
        out.append((f"reach fs=7 shift={shift}", Cfg(BS), Fields((40000,), (fit(rng), aimed, fit(rng))), shift % 4, aimed))
    for shift in range(16):
        aimed = Rice(6, ((shift, 63),) + ((1, 63),) * 110 + ((0, 63),) * (BS - 111))
        out.append((f"reach fs=6 shift={shift}", Cfg(BS), Fields((40000,), (fit(rng), aimed, fit(rng))), shift % 4, aimed))
    return out


@functools.lru_cache(maxsize=None)
def dense_fields():
    """fs 5, q = 0: codes of 6 bits, so the segments hold 3, 2, 3, 3, 2, ... terminators (every phase of 6 against
    16 by a first run of 0..5); and runs of 33 to 60 zeros (two terminators 39 or more bits apart) that leave one to
    three segments without a terminator."""
    rng = np.random.default_rng(563)
    out = []
    for shift in range(6):
        r = rng.integers(0, 32, BS).tolist()
        aimed = Rice(5, tuple((shift if i == 0 else 0, r[i]) for i in range(BS)))
        out.append((f"dense fs=5 shift={shift}", Cfg(BS), Fields((9,), (aimed, aimed, fit(rng, 5))), shift % 4, aimed))
    for run in (33, 40, 47, 60):
        for at in (0, 1, 64, 126, 127):
            r = rng.integers(0, 32, BS).tolist()
            aimed = Rice(5, tuple((run if i in (at, (at + 40) % BS) else 0, r[i]) for i in range(BS)))
            out.append((f"empty fs=5 run={run} at={at}", Cfg(BS), Fields((9,), (fit(rng, 5), aimed, fit(rng, 5))),
                        (run + at) % 4, aimed))
    return out


def _pattern(rng, text: str, cfg: Cfg = Cfg(BS)):
    """F: fitting, L: long, 4 / 8: typical fs 4 / fs 8, Z: zero, R: raw, t: a ragged tail of 50 codes (fs 6),
    T: a long ragged tail (50 codes of 1100 bits)."""
    subs = []
    for ch in text:
        one = {"F": lambda: fit(rng), "L": lambda: long_(rng), "4": lambda: B.typical(rng, 4, BS),
               "8": lambda: B.typical(rng, 8, BS), "Z": lambda: Zero(BS), "R": lambda: B.noise_raw(rng, BS),
               "t": lambda: B.typical(rng, 6, 50), "T": lambda: sized(rng, 6, 1100, "spread", n=50)}[ch]
        subs += [one() for _ in range(cfg.cs)]
    return subs


HANDOVER = ["FFFFFLFFFFFFFFFFFF", "LL" + "F" * (K_RETURN - 1) + "L" + "F" * K_RETURN + "F", "FL" * 10, "LF" * 6,
            "L" + "F" * (K_RETURN + 3) + "LL" + "F" * (K_RETURN + 1) + "L"]
HANDOVER += [f"FF{a}L{b}" + "F" * (K_RETURN + 2) for a in "48ZR" for b in "48ZR"]
HANDOVER += ["FFFL", "LLL", "FFFt", "FFLt", "FLT", "L" + "F" * K_RETURN + "t", "FFFT"]


@functools.lru_cache(maxsize=None)
def handover_fields():
    rng = np.random.default_rng(88)
    return [(f"handover {text}", Cfg(BS), Fields((1000,), tuple(_pattern(rng, text))), i % 4, None)
            for i, text in enumerate(HANDOVER)]


@functools.lru_cache(maxsize=None)
def config_fields():
    """Two component streams and a shifting pixel write (the kernel's CS and SH template arms), both byte orders."""
    rng = np.random.default_rng(2)
    out = []
    for cfg in (Cfg(BS, 2, True, 0), Cfg(BS, 2, False, 3), Cfg(BS, 1, True, 3), Cfg(BS, 1, False, 1), Cfg(BS, 2, True, 2)):
        for i, text in enumerate(("FFFLFFF", "LF" + "F" * K_RETURN + "Ft", "FF8LZFF")):
            out.append((f"config {cfg} {text}", cfg, Fields((321, 60000)[:cfg.cs], tuple(_pattern(rng, text, cfg))),
                        (i + cfg.ulsb) % 4, None))
    return out


FAMILIES = {"edge": edge_fields, "reach": reach_fields, "dense": dense_fields, "handover": handover_fields,
            "config": config_fields}


@functools.lru_cache(maxsize=None)
def cases(family: str):
    return [B.case(what, cfg, f, mis) for what, cfg, f, mis, _ in FAMILIES[family]()]


def test_cases_match_oracle():
    """The oracle decodes every stream to the samples its fields stand for, and the families reach their aims."""
    from oracle import oracle as O

    for family in FAMILIES:
        for c in cases(family):
            got = O.decode(O.cfg(c.cfg.bs, c.cfg.cs, c.cfg.big, c.cfg.ulsb), c.stream, c.n_samples)
            assert np.array_equal(got, c.want), c.what
    edge = edge_fields()
    for fs in (5, 6, 7):
        ends = {last_term(a) for _, _, _, _, a in edge if a.fs == fs}
        lengths = {last_term(a) + 1 + fs for _, _, _, _, a in edge if a.fs == fs}
        assert lengths == {b for b in EDGE_LENGTHS if b >= shortest(fs)}, fs
        # every bit of lane 63's segment that a last terminator can lie on, and the first bits behind the window
        assert ends >= set(range(max(WIN16 - 16, shortest(fs) - 1 - fs), WIN16 + 4)), (fs, sorted(ends))
        for grow in ("last", "early"):
            assert {m for w, _, _, m, a in edge if a.fs == fs and grow in w} == {0, 1, 2, 3}
    assert {fits(a) for *_, a in edge} == {True, False}
    reach7 = [a for w, *_, a in reach_fields() if "fs=7" in w]
    assert max(last_term(a) for a in reach7 if fits(a)) == WIN16 - 1           # bit 15 of lane 63's segment
    for fs, subs in ((7, reach7), (6, [a for w, *_, a in reach_fields() if "fs=6" in w])):
        lay = [B.layout(Cfg(BS), Fields((0,), (a,)))[0] for a in subs]
        assert {int(t - at.header) % 16 for at in lay for t in at.terms} == set(range(16)), fs
    assert all(fits(a) for w, *_, a in reach_fields() if "fs=6" in w)
    for _, _, _, _, a in dense_fields():
        at = B.layout(Cfg(BS), Fields((0,), (a,)))[0]
        per_seg = np.bincount((at.terms - at.header) // 16, minlength=64)
        assert fits(a) and per_seg.max() == 3
        assert (per_seg[:int((at.terms[-1] - at.header) // 16)] == 0).any() == (max(q for q, _ in a.codes) >= 33)
    for fields in (handover_fields(), config_fields()):
        kinds = [fits(s) for _, _, f, _, _ in fields for s in f.subs if isinstance(s, Rice) and s.fs == 6]
        assert any(kinds) and not all(kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_window16(family, path):
    import test_gpu_ricepp_constructed as G

    G.check(cases(family), path)


def _dec_stats():
    """The fused decode's loop counters (a -DRPP_STATS library only), cleared by the read."""
    from dwarfs_amd import _native

    L = _native.lib()
    if not hasattr(L, "rpp_dec_stats_fetch"):
        return None
    st = np.zeros(16, np.uint64)
    L.rpp_dec_stats_fetch.argtypes = [C.c_void_p, C.c_int]
    assert L.rpp_dec_stats_fetch(st.ctypes.data, 1) == 0
    return st


@pytest.mark.gpu
def test_counters():
    """Slot 0 counts the fast loops' sub-blocks and the general path's windows, slot 6 the general path's sub-blocks
    (one window each here: none is longer than 1536 bits), slot 3 the narrow instance's: all of a stream of fitting
    sub-blocks, none of a stream of long ones (whose first costs the narrow instance one parse, not a sub-block);
    after one long sub-block neither it nor the kW16Return that follow it count (whether the 24-bit instance or,
    where the ring has to be refilled first, the general path takes them)."""
    import test_gpu_ricepp_constructed as G

    if _dec_stats() is None:
        pytest.skip("the library is not a -DRPP_STATS build")
    rng = np.random.default_rng(5)
    mixed = "FFFL" + "F" * (K_RETURN + 4)
    for text in ("F" * 12, "L" * 12, mixed):
        c = B.case(text, Cfg(BS), Fields((7,), tuple(_pattern(rng, text))), 0)
        _dec_stats()
        G.check([c], "fused")
        total, narrow, general = (int(v) for v in _dec_stats()[[0, 3, 6]])
        fast = total - general
        print(text, "fast-loop sub-blocks", fast, "narrow", narrow, "general path", general)
        assert total == len(text) and fast > general
        if "L" not in text:
            assert narrow == fast
        elif "F" not in text:
            assert narrow == 0
        else:
            assert 3 <= narrow <= len(mixed) - 1 - K_RETURN
