"""A writer of ricepp streams from field lists, and the constructed-stream families of the ricepp decode tests.

Pure Python and numpy, for the tests only: it imports neither the package nor the oracle.  A stream is its initial
values (one 16-bit field per component stream) and its sub-blocks in stream order (with two component streams:
sub-block i of component 0, then sub-block i of component 1), each a ``Zero(n)``, a ``Raw(stored values)`` or a
``Rice(fs, ((q, r), ...))``.  ``build`` writes the bits LSB first into bytes, ``expand`` states the samples such
fields stand for by the obvious loop over the fields (decode.h:42-83; the expected output of every decoder; it is
no bit reader), ``layout`` says at which bit every header, terminator and remainder lies, ``lead`` / ``place`` put
sub-blocks in front so that the next header lands on a chosen bit counted from the 4-aligned word the kernels
count from (the stream's byte misalignment 0..3 is part of the aim), and ``cut`` states, again on the fields,
what a reader sees of a stream offered with fewer bytes (zeros up to the end of its last 8-byte packet).

The kernel geometry restated below is used only to aim the cases and to count what a family reaches, never to
compute an expected sample.

The families (``density``, ``window_edges``, ``long_runs``, ``class_pairs``, ``values``, ``end_of_input``,
``decoys``) return lists of :class:`Case`.
"""

from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

# ---- kernel geometry, restated to aim cases (never to compute a sample) ----
SEG24 = 24            # ricepp_tables.h kSegBits: bits per lane segment, fs 0..7
SEG32 = 32            # ricepp_decode_fused.hip `SB = W32 ? 32u : kSegBits`: fs 8..13 in the fast loops
WIN24 = 64 * SEG24    # ricepp_tables.h kWinBits = kWave * kSegBits = 1536
WIN32 = 64 * SEG32    # the fs 8..13 fast loop's window = 2048
WIN_ROWS = 16 * SEG24  # ricepp_decode_rows.hip: one 16-lane row per stream = 384
RING_WORDS = 1024     # ricepp_tables.h kRingWords (32768 bits)
CHUNK_WORDS = 256     # ricepp_tables.h kChunkWords = 4 * kWave (8192 bits)
ROWS_SLOTS = (4, 12, 24)  # ricepp_decode_rows.hip: terminators per segment of its three slot classes
SPEC_STEPS = 12       # ricepp_internal.h kSpecSteps
SPEC_VERIFY = 24      # ricepp_internal.h kSpecVerify

OK = 0
TRUNCATED = -2        # RPP_TRUNCATED_INPUT
M32 = 0xFFFFFFFF


class Cfg(NamedTuple):
    bs: int
    cs: int = 1
    big: bool = True
    ulsb: int = 0


class Zero(NamedTuple):
    n: int                       # samples the sub-block stands for


class Raw(NamedTuple):
    values: Tuple[int, ...]      # stored 16-bit values, as they lie in the output


class Rice(NamedTuple):
    fs: int
    codes: Tuple[Tuple[int, int], ...]  # (q, r): q zeros, a one, r in fs bits


Sub = Union[Zero, Raw, Rice]


class Fields(NamedTuple):
    init: Tuple[int, ...]        # one 16-bit field per component stream
    subs: Tuple[Sub, ...]        # stream order


class At(NamedTuple):
    """Bit positions of one sub-block, from the stream's first bit."""
    kind: str                    # "zero", "raw", "rice"
    fs: int                      # -1 unless rice
    header: int
    terms: Optional[np.ndarray]  # rice: each code's terminator (its remainder lies at terms + 1; its run starts
    end: int                     #       at the code before's terms + 1 + fs, or at header + 4)


class Case(NamedTuple):
    what: str
    cfg: Cfg
    stream: bytes                # what lies in the buffer from the stream's first byte on
    n_samples: int
    want: Optional[np.ndarray]   # uint16, as stored; None where status is not OK
    status: int
    mis: int = 0                 # the byte offset mod 4 the stream is to be packed at
    in_bytes: Optional[int] = None  # the size the decoder is offered (None: len(stream))
    inp: Optional[np.ndarray] = None  # encode cases: the input samples where they are not ``want`` (dropped dirt)
    fields: Optional[Fields] = None   # encode cases: the fields the stream was built from

    @property
    def size(self) -> int:
        return len(self.stream) if self.in_bytes is None else self.in_bytes


def count(sub: Sub) -> int:
    return sub.n if isinstance(sub, Zero) else len(sub.values) if isinstance(sub, Raw) else len(sub.codes)


def n_samples(fields: Fields) -> int:
    return sum(count(s) for s in fields.subs)


def check(cfg: Cfg, fields: Fields) -> None:
    """Chunks of cs sub-blocks of equal counts, bs each but for a shorter last one."""
    assert len(fields.init) == cfg.cs and len(fields.subs) % cfg.cs == 0
    groups = [fields.subs[i:i + cfg.cs] for i in range(0, len(fields.subs), cfg.cs)]
    for gi, g in enumerate(groups):
        c = count(g[0])
        assert all(count(s) == c for s in g)
        assert c == cfg.bs or (gi == len(groups) - 1 and 0 < c < cfg.bs), (gi, c)


def _emit(cfg: Cfg, fields: Fields):
    """(one uint8 per bit, [At])"""
    check(cfg, fields)
    total = 16 * cfg.cs
    for s in fields.subs:
        if isinstance(s, Raw):
            total += 4 + 16 * len(s.values)
        elif isinstance(s, Rice):
            total += 4 + sum(q for q, _ in s.codes) + len(s.codes) * (1 + s.fs)
        else:
            total += 4
    bits = np.zeros(total, np.uint8)

    def put(pos, v, nb):
        for j in range(nb):
            bits[pos + j] = (v >> j) & 1

    for c, v in enumerate(fields.init):
        assert 0 <= v <= 0xFFFF
        put(16 * c, v, 16)
    pos, ats = 16 * cfg.cs, []
    for s in fields.subs:
        if isinstance(s, Zero):
            ats.append(At("zero", -1, pos, None, pos + 4))
            pos += 4
        elif isinstance(s, Raw):
            put(pos, 15, 4)
            v = np.asarray(s.values, np.int64)
            assert ((v >= 0) & (v <= 0xFFFF)).all()
            bits[pos + 4:pos + 4 + 16 * len(v)] = ((v[:, None] >> np.arange(16)) & 1).ravel()
            ats.append(At("raw", -1, pos, None, pos + 4 + 16 * len(v)))
            pos += 4 + 16 * len(v)
        else:
            assert 0 <= s.fs <= 13
            put(pos, s.fs + 1, 4)
            qr = np.asarray(s.codes, np.int64).reshape(-1, 2)
            q, r = qr[:, 0], qr[:, 1]
            assert (q >= 0).all() and (r >= 0).all() and (r < (1 << s.fs)).all()
            lens = q + 1 + s.fs
            starts = pos + 4 + np.concatenate(([0], np.cumsum(lens)[:-1]))
            terms = starts + q
            bits[terms] = 1
            for j in range(s.fs):
                bits[terms + 1 + j] = (r >> j) & 1
            end = int(pos + 4 + lens.sum())
            ats.append(At("rice", s.fs, pos, terms, end))
            pos = end
    assert pos == total
    return bits, ats


def build(cfg: Cfg, fields: Fields) -> bytes:
    """The stream's bytes: bits LSB first, the last byte zero padded (bitstream_writer.h:110-145)."""
    return np.packbits(_emit(cfg, fields)[0], bitorder="little").tobytes()


def layout(cfg: Cfg, fields: Fields) -> List[At]:
    return _emit(cfg, fields)[1]


def _bswap(v: int) -> int:
    return ((v >> 8) | (v << 8)) & 0xFFFF


def px_read(cfg: Cfg, stored: int) -> int:
    return (_bswap(stored) if cfg.big else stored) >> cfg.ulsb


def px_write(cfg: Cfg, last: int) -> int:
    t = ((last & 0xFFFF) << cfg.ulsb) & 0xFFFF
    return _bswap(t) if cfg.big else t


def expand(cfg: Cfg, fields: Fields) -> np.ndarray:
    """The samples the fields stand for (decode.h:42-83): difference = ((q << fs) | r) mod 2^32, last += its
    zig-zag inverse mod 2^32, stored sample = (uint16)(last << ulsb), byte swapped for big endian; after a raw
    sub-block last = px_read of its final stored value; a zero sub-block repeats px_write(last)."""
    check(cfg, fields)
    out = np.zeros(n_samples(fields), np.uint16)
    last = list(fields.init)
    base = 0
    for g in range(0, len(fields.subs), cfg.cs):
        cnt = count(fields.subs[g])
        for c in range(cfg.cs):
            sub = fields.subs[g + c]
            for i in range(cnt):
                if isinstance(sub, Raw):
                    v = sub.values[i]
                    if i == cnt - 1:
                        last[c] = px_read(cfg, v)
                else:
                    if isinstance(sub, Rice):
                        q, r = sub.codes[i]
                        d = ((q << sub.fs) | r) & M32
                        last[c] = (last[c] + ((d >> 1) ^ (M32 if d & 1 else 0))) & M32
                    v = px_write(cfg, last[c])
                out[base + c + cfg.cs * i] = v
        base += cfg.cs * cnt
    return out


def first_header(cfg: Cfg, mis: int) -> int:
    """The first sub-block's header, in bits from the 4-aligned word that holds the stream's first byte."""
    return 8 * mis + 16 * cfg.cs


def lead(cfg: Cfg, bits: int, salt: int = 0) -> List[Sub]:
    """Whole chunks that take exactly ``bits`` bits: zero sub-blocks where that is a small multiple of 4, else one
    fs 0 sub-block whose runs add up to the rest (and a zero sub-block for the second component)."""
    if bits == 0:
        return []
    if bits % (4 * cfg.cs) == 0 and bits <= 16 * cfg.cs:
        return [Zero(cfg.bs)] * (bits // 4)
    rest = bits - 4 - cfg.bs - 4 * (cfg.cs - 1)
    if rest < 0:
        raise ValueError(f"no leading sub-blocks of {bits} bits for {cfg}")
    q = [rest // cfg.bs] * cfg.bs
    for i in range(rest % cfg.bs):
        q[(i * 7 + salt) % cfg.bs if cfg.bs % 7 else i] += 1
    return [Rice(0, tuple((x, 0) for x in q))] + [Zero(cfg.bs)] * (cfg.cs - 1)


def place(cfg: Cfg, mis: int, bit: int, before: Sequence[Sub] = (), modulo: int = 0, salt: int = 0) -> List[Sub]:
    """``before`` and padding chunks, so that the header of the sub-block put behind them lies at ``bit`` from the
    4-aligned word (with ``modulo``: at the first such position congruent to ``bit`` that can be reached)."""
    at = first_header(cfg, mis)
    if before:
        f = Fields((0,) * cfg.cs, tuple(before))
        at += layout(cfg, f)[-1].end - 16 * cfg.cs
    need = bit - at
    if modulo:
        need %= modulo
        while True:
            try:
                pad = lead(cfg, need, salt)
                break
            except ValueError:
                need += modulo
    else:
        pad = lead(cfg, need, salt)
    return list(before) + pad


def typical(rng, fs: int, n: int) -> Rice:
    """Codes as an encoder that chose fs would write them: short runs, any remainder."""
    q = np.minimum(rng.geometric(0.55, n) - 1, 6)
    r = rng.integers(0, 1 << fs, n)
    return Rice(fs, tuple(zip(q.tolist(), r.tolist())))


def noise_raw(rng, n: int) -> Raw:
    return Raw(tuple(rng.integers(0, 65536, n).tolist()))


def kind_sub(rng, kind: int, n: int) -> Sub:
    """Kind 0: zero, 1..14: Rice with fs = kind - 1, 15: raw (the 4-bit header's value)."""
    return Zero(n) if kind == 0 else noise_raw(rng, n) if kind == 15 else typical(rng, kind - 1, n)


def case(what: str, cfg: Cfg, fields: Fields, mis: int = 0) -> Case:
    return Case(what, cfg, build(cfg, fields), n_samples(fields), expand(cfg, fields), OK, mis)


def worst_case_bytes(cfg: Cfg, n: int) -> int:
    """codec.h:142-151, restated to show that the long-run streams exceed it."""
    per = n // cfg.cs
    return ((16 + 4 * -(-per // cfg.bs) + 16 * per) * cfg.cs + 7) // 8


def _cfg_for(i: int, bs: int, cs: int = 1) -> Cfg:
    return Cfg(bs, cs, i % 2 == 0, (0, 3, 0, 1)[i % 4])


# ---------------------------------------------------------------------------------------------------------------
# density
# ---------------------------------------------------------------------------------------------------------------

DENSITY_BS = [16, 32, 64, 128, 29, 256]
DENSITY_PATTERNS = ["all_q0", "every_bit", "full_empty"]


def seg_bits(fs: int) -> int:
    return SEG32 if fs >= 8 else SEG24


def _density_codes(pattern: str, fs: int, n: int, salt: int):
    k, sb = fs + 1, seg_bits(fs)
    rmask = (1 << fs) - 1
    if pattern == "all_q0":
        q = [0] * n
    elif pattern == "every_bit":  # terminators advance by 1 mod the segment width
        q = [(1 - k) % sb] * n
    else:  # as many codes as a segment holds, then a run that leaves at least one segment empty
        m = max(1, sb // k)
        q = [0 if (i + 1) % (m + 1) else 2 * sb for i in range(n)]
    return tuple((x, (salt * 131 + i * 2654435761 >> 7) & rmask) for i, x in enumerate(q))


@functools.lru_cache(maxsize=None)
def density_fields():
    out = []
    i = 0
    for fs in range(14):
        for bs in DENSITY_BS:
            for pattern in DENSITY_PATTERNS:
                cfg, mis = _cfg_for(i, bs), i % 4
                phase = (i * 7) % 48
                subs = place(cfg, mis, phase, modulo=96, salt=i)
                subs += [Rice(fs, _density_codes(pattern, fs, bs, i + j)) for j in range(3)]
                subs.append(Rice(fs, _density_codes(pattern, fs, max(1, bs // 3), i)))  # a ragged last chunk
                out.append((f"density fs={fs} bs={bs} {pattern} phase={phase} mis={mis}", cfg,
                            Fields((0x1234 + i,), tuple(subs)), mis, pattern))
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def density() -> List[Case]:
    """Every fs 0..13 at bs 16, 32, 64, 128, 29 and 256 with all q = 0 (the most terminators a segment can
    hold), a terminator on every bit of a segment in turn, and full segments alternating with empty ones; the
    first of these sub-blocks' headers at every bit phase 0..47 over the family."""
    return [case(what, cfg, f, mis) for what, cfg, f, mis, _ in density_fields()]


# ---------------------------------------------------------------------------------------------------------------
# window_edges
# ---------------------------------------------------------------------------------------------------------------

EDGE_ENDS = list(range(-5, 3))  # the sub-block's end = the next header, relative to the window's last bit + 1
EDGE_FOLLOWERS = ["zero", "raw", "same_class", "other_class"]
EDGE_PLACES = ["first_window", "after_fast_loop"]
EDGE_WINDOWS = {WIN_ROWS: [(bs, fs) for bs in (16, 32) for fs in range(1, 8)],
                WIN24: [(bs, fs) for bs in (64, 128) for fs in range(8)],
                WIN32: [(bs, fs) for bs in (64, 128) for fs in range(8, 14)]}


def _spread(rng, total: int, n: int) -> List[int]:
    """n run lengths that add up to ``total``."""
    cuts = np.sort(rng.integers(0, total + 1, n - 1))
    return np.diff(np.concatenate(([0], cuts, [total]))).tolist()


def _sized_rice(rng, fs: int, n: int, bits: int) -> Rice:
    """A Rice sub-block of n codes that takes exactly ``bits`` bits, header included."""
    slack = bits - 4 - n * (fs + 1)
    assert slack >= 0, (fs, n, bits)
    return Rice(fs, tuple(zip(_spread(rng, slack, n), rng.integers(0, 1 << fs, n).tolist())))


def _other_class(fs: int) -> int:
    return 10 if fs < 8 else 6


@functools.lru_cache(maxsize=None)
def window_edges_fields():
    out = []
    rng = np.random.default_rng(384)
    for W, pairs in EDGE_WINDOWS.items():
        for pi, (bs, fs) in enumerate(pairs):
            for di, d in enumerate(EDGE_ENDS):
                combo = (pi + di) % 8
                follower, where = EDGE_FOLLOWERS[combo % 4], EDGE_PLACES[combo // 4]
                cfg, mis = _cfg_for(pi + di, bs), (pi + di) % 4
                subs = [typical(rng, fs, bs) for _ in range(4)] if where == "after_fast_loop" else []
                aimed = len(subs)
                subs.append(_sized_rice(rng, fs, bs, W + d))
                subs.append({"zero": Zero(bs), "raw": noise_raw(rng, bs), "same_class": typical(rng, fs, bs),
                             "other_class": typical(rng, _other_class(fs), bs)}[follower])
                subs.append(typical(rng, fs, bs))
                out.append((f"edge W={W} bs={bs} fs={fs} end=W{d:+d} {follower} {where}", cfg,
                            Fields((0x8001,), tuple(subs)), mis, (W, d, follower, where, aimed)))
    for W, (bs, fss) in {WIN_ROWS: (16, (2, 7)), WIN24: (128, (0, 6)), WIN32: (128, (8, 13))}.items():
        for fs in fss:
            for windows in (2, 3):
                for d in (-1, 0, 1):
                    cfg = _cfg_for(d + windows, bs)
                    subs = [typical(rng, fs, bs), _sized_rice(rng, fs, bs, windows * W + d), typical(rng, fs, bs)]
                    out.append((f"edge W={W} bs={bs} fs={fs} end={windows}W{d:+d}", cfg, Fields((77,), tuple(subs)),
                                (d + windows) % 4, (W, windows, d)))
    return out


@functools.lru_cache(maxsize=None)
def window_edges() -> List[Case]:
    """A sub-block whose last code ends, and whose follower's header so lies, 5 bits before to 2 bits behind the
    end of the window that starts at its own header: 384 bits (bs 16 / 32, fs 1..7), 1536 (fs 0..7) and 2048
    (fs 8..13); as a stream's first sub-block and after four typical ones; followed by a zero, a raw, a same-class
    and an other-class sub-block.  Then sub-blocks of exactly two and three windows, one bit either way."""
    return [case(what, cfg, f, mis) for what, cfg, f, mis, _ in window_edges_fields()]


# ---------------------------------------------------------------------------------------------------------------
# long_runs
# ---------------------------------------------------------------------------------------------------------------

LONG_RUNS = [23, 24, 25, 31, 32, 33, 63, 64, 65, 383, 384, 385, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096,
             4097, 32767, 32768, 32769, 65535, 65536, 70000]
LONG_FS = [0, 1, 3, 6, 10, 13]
LONG_WHERE = ["first", "middle", "last"]
LONG_BS = [4, 16, 29, 128]
FILLER_Q = 17  # every other code is 18 bits or more, so the stream is longer than 16 bits per sample


def _long_fields(run: int, fs: int, where: str, bs: int, salt: int, nudge: int = 0):
    rmask = (1 << fs) - 1
    at = {"first": 0, "middle": bs // 2, "last": bs - 1}[where]
    codes = [(FILLER_Q, (salt + 5 * i) & rmask) for i in range(bs)]
    codes[at] = (run, (salt * 3 + 1) & rmask)
    if nudge:
        codes[at - 1] = (FILLER_Q + nudge, codes[at - 1][1])
    follow = tuple((FILLER_Q + (i & 1), (salt + 3 * i) & rmask) for i in range(bs))
    return Fields((0x00F0 + salt,), (Rice(fs, tuple(codes)), Rice(fs, follow))), at


@functools.lru_cache(maxsize=None)
def long_runs_fields():
    out = []
    i = 0
    for fs in LONG_FS:
        for where in LONG_WHERE:
            for run in LONG_RUNS:
                bs = LONG_BS[i % 4]
                cfg, mis = _cfg_for(i // 4, bs), (i // 2) % 4
                f, at = _long_fields(run, fs, where, bs, i)
                out.append((f"long run={run} fs={fs} {where} bs={bs} mis={mis}", cfg, f, mis, (run, fs, where, at)))
                i += 1
    # six chunks, so that the worst case of the sample count is more than one unit of 2^13 bits
    for fs in (1, 10):
        for run in (2049, 32768, 70000):
            cfg = Cfg(128, 1, True, 0)
            f, at = _long_fields(run, fs, "middle", 128, run % 251)
            f = Fields(f.init, f.subs + (f.subs[1],) * 4)
            out.append((f"long run={run} fs={fs} middle bs=128 six chunks", cfg, f, fs % 4, (run, fs, "six_chunks", at)))
    # a run whose terminator is the last bit of an 8-byte packet of the stream, and the first of the next
    for fs in (0, 6):
        for want_bit in (63, 0):
            cfg = Cfg(16, 1, True, 0)
            f, at = _long_fields(4096, fs, "middle", 16, fs)
            t = int(layout(cfg, f)[0].terms[at])
            f, at = _long_fields(4096, fs, "middle", 16, fs, nudge=(want_bit - t) % 64)
            out.append((f"long run=4096 fs={fs} terminator on packet bit {want_bit}", cfg, f, fs % 4,
                        (4096, fs, f"packet_bit_{want_bit}", at)))
    return out


@functools.lru_cache(maxsize=None)
def long_runs() -> List[Case]:
    """Unary runs around a segment (24, 32), 64 bits, each window (384, 1536, 2048), 4096, the whole 32768-bit
    ring, and 65535, 65536 and 70000 zeros, as the first, a middle and the last code of a sub-block, at fs 0, 1,
    3, 6, 10 and 13 (q << fs passes 2^16 and 2^17).  Every other code has a run of 17, so each stream is complete
    and longer than the worst case an encoder writes for its sample count."""
    return [case(what, cfg, f, mis) for what, cfg, f, mis, _ in long_runs_fields()]


# ---------------------------------------------------------------------------------------------------------------
# class_pairs
# ---------------------------------------------------------------------------------------------------------------

PAIR_BS = [16, 32, 64, 128]


def second_pair(a: int, b: int) -> Tuple[int, int]:
    """The pair the second component runs beside (a, b): another one, and over all pairs again all 256."""
    return (a + 5) % 16, (b + 11) % 16


@functools.lru_cache(maxsize=None)
def class_pairs_fields():
    out = []
    i = 0
    for bs in PAIR_BS:
        for cs in (1, 2):
            rng = np.random.default_rng(1000 * bs + cs)
            for a in range(16):
                for b in range(16):
                    cfg, mis = _cfg_for(i, bs, cs), i % 4
                    comps = [(a, b), second_pair(a, b)][:cs]
                    subs = []
                    for k in "AAAABBBBA":
                        for ka, kb in comps:
                            subs.append(kind_sub(rng, ka if k == "A" else kb, bs))
                    out.append((f"pair {a}->{b} bs={bs} cs={cs}", cfg,
                                Fields(tuple(0x4000 + 257 * c + i for c in range(cs)), tuple(subs)), mis, (a, b)))
                    i += 1
    return out


@functools.lru_cache(maxsize=None)
def class_pairs() -> List[Case]:
    """For every ordered pair (A, B) of the 16 kinds of sub-block (the header's 16 values) the stream
    A A A A B B B B A of full sub-blocks with typical codes, for bs 16, 32, 64, 128 and one and two component
    streams; the second component runs another pair, so a raw sub-block of one lies between Rice ones of the
    other."""
    return [case(what, cfg, f, mis) for what, cfg, f, mis, _ in class_pairs_fields()]


# ---------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------

def _zz(delta: int, fs: int) -> Tuple[int, int]:
    """The code of a signed difference at fs."""
    d = (delta << 1) if delta >= 0 else ((-delta << 1) - 1)
    return d >> fs, d & ((1 << fs) - 1)


def _diff_code(d: int, fs: int) -> Tuple[int, int]:
    return d >> fs, d & ((1 << fs) - 1)


@functools.lru_cache(maxsize=None)
def values() -> List[Case]:
    """Zig-zag extremes and `last` wrapping through 0 and through 0xFFFF >> ulsb, initial values with bits above
    16 - ulsb, raw sub-blocks with dirty low bits followed by Rice and zero sub-blocks, ulsb 0, 3 and 15 in both
    byte orders, ragged last chunks of 1, 2 and bs - 1 samples per component, n = 0 and n = cs."""
    out = []
    rng = np.random.default_rng(16)
    i = 0
    for ulsb in (0, 3, 15):
        for big in (True, False):
            top = 0xFFFF >> ulsb
            for bs, cs in ((16, 1), (128, 1), (32, 2), (29, 2)):
                cfg = Cfg(bs, cs, big, ulsb)
                mis = i % 4
                i += 1
                # differences 0xFFFF, 0xFFFE, 0x8000 (fs 10: q up to 63), and steps that wrap last both ways
                ext = [_diff_code(d, 10) for d in (0xFFFF, 0xFFFE, 0x8000, 1, 2, 0xFFFF, 0x8000, 0x7FFF)]
                wrap = [_zz(-3, 12), _zz(5, 12), _zz(-9, 12), _zz(top, 12), _zz(-top - 2, 12), _zz(top + 4, 12)]
                for init in dict.fromkeys((1, top, 0xFFFF, 0x8000 | (top >> 1))):  # (the last two: bits above 16 - ulsb)
                    subs = []
                    for c in range(cs):
                        subs.append(Rice(10, tuple(ext[(j + c) % len(ext)] for j in range(bs))))
                    for c in range(cs):
                        subs.append(Rice(12, tuple(wrap[(j + 2 * c) % len(wrap)] for j in range(bs))))
                    f = Fields(tuple((init + 0x1111 * c) & 0xFFFF for c in range(cs)), tuple(subs))
                    out.append(case(f"values extremes {cfg} init={init:#06x}", cfg, f, mis))
                # raw with dirty low bits (all 16 bits noise), then Rice and zero
                subs = []
                for kinds in ((15, 3), (15, 0), (15, 15), (6, 0), (15, 9), (0, 0), (15, 15), (0, 2)):
                    for c in range(cs):
                        subs.append(kind_sub(rng, kinds[c], bs))
                f = Fields((0xFFFF,) * cs, tuple(subs))
                out.append(case(f"values raw then rice and zero {cfg}", cfg, f, mis))
                for ragged in sorted({1, 2, bs - 1}):
                    for kind in (0, 4, 15, 11):
                        subs = [kind_sub(rng, 7, bs) for _ in range(cs)]
                        subs += [kind_sub(rng, (kind + 7 * c) % 16, ragged) for c in range(cs)]
                        f = Fields((0x0123, 0xFEDC)[:cs], tuple(subs))
                        out.append(case(f"values ragged {ragged} kind={kind} {cfg}", cfg, f, mis))
                out.append(case(f"values n=0 {cfg}", cfg, Fields((0xBEEF, 0x1234)[:cs], ()), mis))
                for kind in (0, 1, 8, 15):
                    f = Fields((0xBEEF, 0x1234)[:cs], tuple(kind_sub(rng, kind, 1) for _ in range(cs)))
                    out.append(case(f"values n=cs kind={kind} {cfg}", cfg, f, mis))
    return out


# ---------------------------------------------------------------------------------------------------------------
# end_of_input
# ---------------------------------------------------------------------------------------------------------------

def cut(cfg: Cfg, fields: Fields, in_bytes: int):
    """(status, fields) as a reader sees the stream's first ``in_bytes`` bytes (bitstream_reader.h:149-183): the
    bits behind them are zeros up to the end of the last 8-byte packet, 64 * ceil(in_bytes / 8), and a field
    with a bit at or behind that is the end (TRUNCATED).  Stated on the fields: a field that reaches over the cut
    loses its high bits; behind it every header reads as a zero sub-block, every raw value as 0, and a unary run
    finds no terminator."""
    C, L = 8 * in_bytes, 64 * ((in_bytes + 7) // 8)

    def seen(value, start, nb):  # (value as read, or None where the field reaches behind L)
        if start + nb > L:
            return None
        return value & ((1 << max(0, min(nb, C - start))) - 1)

    init = []
    for c, v in enumerate(fields.init):
        v = seen(v, 16 * c, 16)
        if v is None:
            return TRUNCATED, None
        init.append(v)
    pos, subs = 16 * cfg.cs, []
    for s in fields.subs:
        n = count(s)
        head = 0 if isinstance(s, Zero) else 15 if isinstance(s, Raw) else s.fs + 1
        h = seen(head, pos, 4)
        if h is None:
            return TRUNCATED, None
        same = h == head and pos + 4 <= C
        pos += 4
        if h == 0:
            subs.append(Zero(n))
        elif h == 15:
            vals = []
            for i in range(n):
                v = seen(s.values[i] if same else 0, pos, 16)
                if v is None:
                    return TRUNCATED, None
                vals.append(v)
                pos += 16
            subs.append(Raw(tuple(vals)))
        else:
            fs, codes = h - 1, []
            for i in range(n):
                if not same or pos + s.codes[i][0] >= C:  # no terminator before the zeros: the run meets L
                    return TRUNCATED, None
                q, r = s.codes[i]
                pos += q + 1
                r = seen(r, pos, fs)
                if r is None:
                    return TRUNCATED, None
                pos += fs
                codes.append((q, r))
            subs.append(Rice(fs, tuple(codes)))
    return OK, Fields(tuple(init), tuple(subs))


END_BITS = [63, 0, 1, 7]  # the bit of its 8-byte packet that holds the stream's last consumed bit
END_TAILS = ["remainders", "unary", "headers", "raw"]


def _end_base(tail: str, end_bit: int):
    """A bs 16 stream ending in ``tail`` whose last consumed bit is bit ``end_bit`` of a packet."""
    cfg = Cfg(16, 1, True, 0)
    def fields(extra):
        rng2 = np.random.default_rng(1000 + END_TAILS.index(tail))
        first = list(typical(rng2, 4, 16).codes)
        first[3] = (first[3][0] + extra, first[3][1])
        subs = [Rice(4, tuple(first)), noise_raw(rng2, 16), typical(rng2, 2, 16)]
        if tail == "remainders":
            subs.append(Rice(12, tuple((1 + (j & 1), 0xFFF - 17 * j) for j in range(16))))
        elif tail == "unary":
            subs.append(Rice(0, tuple((j % 3, 0) for j in range(15)) + ((90, 0),)))
        elif tail == "headers":
            subs += [Zero(16)] * 20 + [Rice(0, ((0, 0),) * 5)]
        else:
            subs.append(Raw(tuple(0x8001 | (j * 0x0F10) & 0xFFFF for j in range(16))))
        return Fields((0x0A0A,), tuple(subs))

    for extra in range(64):
        f = fields(extra)
        if (layout(cfg, f)[-1].end - 1) % 64 == end_bit:
            return cfg, f
    raise AssertionError


@functools.lru_cache(maxsize=None)
def end_of_input_fields():
    out = []
    for tail, end_bit in zip(END_TAILS, END_BITS):
        cfg, f = _end_base(tail, end_bit)
        full = build(cfg, f)
        for delta in range(-9, 10):
            for mis in range(4):
                out.append((f"end {tail} last bit {end_bit} in_bytes={len(full)}{delta:+d} mis={mis}", cfg, f, mis,
                            (tail, end_bit, delta, len(full) + delta)))
    return out


@functools.lru_cache(maxsize=None)
def end_of_input() -> List[Case]:
    """Streams whose last consumed bit is bit 63, 0, 1 or 7 of an 8-byte packet, offered with in_bytes from 9
    short to 9 long at every byte offset mod 4; the bytes from in_bytes on are 0xFF.  The cuts fall inside
    remainders, a unary run, headers and raw values.  Wanted by the packet rule, stated on the fields by
    ``cut``."""
    out = []
    for what, cfg, f, mis, (_, _, delta, nbytes) in end_of_input_fields():
        full = build(cfg, f)
        status, seen = cut(cfg, f, nbytes) if delta < 0 else (OK, f)
        stream = (full[:nbytes] if delta < 0 else full + b"\xff" * delta) + b"\xff" * 16
        want = expand(cfg, seen) if status == OK else None
        out.append(Case(what, cfg, stream, n_samples(f), want, status, mis, nbytes))
    return out


# ---------------------------------------------------------------------------------------------------------------
# decoys
# ---------------------------------------------------------------------------------------------------------------

DECOY_CONFIGS = [(16, 1), (64, 1), (128, 1), (16, 2), (64, 2), (128, 2)]
DECOY_SHIFTS = list(range(1, 16))
DECOY_SUBBLOCKS = 34
DECOY_FS = (5, 6, 7)  # headers 6..8: within a range of 4


def _decoy_chain(rng, bs: int, start: int, fixed: Sequence[int]):
    """Rice sub-blocks of bs codes from bit ``start`` on such that the 4 bits at each position of ``fixed`` (the
    true raw headers, 1111) fall wholly into a remainder, which is set to hold them.  [(fs, codes)], end."""
    fixed = list(fixed)
    pos, subs = start, []
    for _ in range(DECOY_SUBBLOCKS):
        fs = DECOY_FS[int(rng.integers(0, 3))]
        pos += 4
        codes = []
        for _ in range(bs):
            while fixed and fixed[0] < pos:
                fixed.pop(0)
            gap = fixed[0] - pos - 1 if fixed else 1 << 30  # the run that puts the terminator right before it
            if gap <= 16:
                assert gap >= 0, "a true header under a decoy header or terminator"
                q, r = gap, 15 | (int(rng.integers(0, 1 << fs)) & ~15)
            else:
                q, r = int(rng.integers(0, 3)), int(rng.integers(0, 1 << fs))
            codes.append((q, r))
            pos += q + 1 + fs
        subs.append(Rice(fs, tuple(codes)))
    return subs, pos


@functools.lru_cache(maxsize=None)
def decoys_fields():
    out = []
    for bs, cs in DECOY_CONFIGS:
        for shift in DECOY_SHIFTS:
            cfg, mis = Cfg(bs, cs, shift % 2 == 0, 0), shift % 4
            rng = np.random.default_rng(100 * bs + 10 * cs + shift)
            per = 4 + 16 * bs                 # bits of a raw sub-block
            h0 = 16 * cs                      # the first true header, from the stream's first bit
            start = h0 + 4 + shift            # the decoy chain's first header
            nraw = cs * (-(-(DECOY_SUBBLOCKS * (4 + bs * 11) + shift) // (cs * per)) + 1)
            chain, end = _decoy_chain(rng, bs, start, [h0 + j * per for j in range(1, nraw)])
            assert end <= h0 + nraw * per
            # the chain's bits, written by the same writer, laid over the raw sub-blocks' bits
            cbits, cats = _emit(Cfg(bs), Fields((0,), tuple(chain)))
            cbits = cbits[16:]
            bits = rng.integers(0, 2, nraw * per).astype(np.uint8)
            bits[:4 + shift] = 1
            for j in range(nraw):
                bits[j * per:j * per + 4] = 1
            bits[4 + shift:4 + shift + len(cbits)] = cbits
            raws = []
            for j in range(nraw):
                assert bits[j * per:j * per + 4].all()  # (the chain holds the true headers in its remainders)
                v = bits[j * per + 4:(j + 1) * per].reshape(bs, 16)
                raws.append(Raw(tuple((v.astype(np.int64) << np.arange(16)).sum(1).tolist())))
            subs = raws + [typical(rng, 6, bs) for _ in range(8 * cs)]
            f = Fields((0x0101,) * cs, tuple(subs))
            assert np.array_equal(_emit(cfg, f)[0][h0:h0 + nraw * per], bits)
            out.append((f"decoy bs={bs} cs={cs} shift={shift} mis={mis}", cfg, f, mis,
                        (start, [a.header + start - 16 for a in cats], nraw)))
    return out


@functools.lru_cache(maxsize=None)
def decoys() -> List[Case]:
    """Raw sub-blocks whose values, read as bits, hold a chain of 34 self-consistent Rice sub-blocks (fs 5..7,
    written by this writer) that starts 1..15 bits behind the first true header and runs on through the true raw
    headers (each lies in a decoy remainder); eight true Rice chunks follow.  The wanted output is the raw values
    and what follows."""
    return [case(what, cfg, f, mis) for what, cfg, f, mis, _ in decoys_fields()]


FAMILIES = {"density": density, "window_edges": window_edges, "long_runs": long_runs, "class_pairs": class_pairs,
            "values": values, "end_of_input": end_of_input, "decoys": decoys}


# ===============================================================================================================
# The encode side: streams an encoder writes, built from zig-zag deltas and a declared kind per sub-block
# ===============================================================================================================
#
# ``from_deltas`` turns zig-zag deltas and a kind per sub-block into ``Fields`` by the obvious loop (q = d >> fs,
# r = d & mask; a raw sub-block stores its pixels as they lie; a zero sub-block has no delta but 0).  ``split_rule``
# restates compute_best_split (encode.h:43-90) and ``wave_groups`` / ``flush_trace`` / ``seg_chunks_rule`` the
# encode kernels' geometry: like the decode geometry above they are used only to aim the cases and to count what a
# family reaches, never to compute an expected byte.  The expected bytes of every case are ``build(cfg, fields)``;
# that an encoder writes exactly these is proved on the CPU against the oracle and the compiled reference by
# tests/test_ricepp_encode_constructed_host.py.
#
# What the split rule can and cannot do (with avg = sum / n, start = max(0, bit_width(floor(avg)) - 2), so
# 2^(start+1) <= avg < 2^(start+2) unless start was clamped to 0, and x_i = d_i / 2^f):
#   * no step down: cost(f-1) <= cost(f) needs sum(floor(2x) - floor(x)) <= n, but floor(2x) - floor(x) >= x - 1/2
#     and at f = start the x sum to 2n or more, so the sum is at least 1.5 n.  A walk of direction -1 stays at
#     `start` (and with start 0 nothing lies below).
#   * at most one step up behind the first pair: at f = start + 1 the x sum to less than 2n and
#     floor(x) - floor(x/2) <= (x + 1) / 2, so one step (to start + 2) can be an equal or a lower cost; at
#     f = start + 2 the same sum is below x/4 + 1/2 each, less than n in all.
#   * fs < 14 implies bits < 16 n: the chosen fs is start, start + 1 or start + 2 and at each of them
#     sum(d >> fs) < 2n where fs is 12 or 13 (else bits < n (fs + 5) <= 16 n).  So raw is only ever reached
#     through fs 14 and 15, i.e. starts 12 (equal-cost step 13 -> 14), 13 and 14.
#   * the hill climb never ends above the lowest cost of any fs: cost(f + 1) - cost(f) = n - sum(g(x_i)) with
#     g(x) = floor(x) - floor(x / 2) = ceil(floor(x) / 2), and g(x / 2) <= g(x), so the cost is convex in fs and a
#     local minimum is the global one.  (A writer that takes the global minimum differs only in which of several
#     fs of equal cost it takes.)
# The host test asserts all four on every sub-block of every family.

ENC_WIN_WORDS = 1024      # ricepp_encode.hip kEncWin
ENC_FLUSH_WORDS = 256     # kEncFlushWords
ENC_SEG_MIN, ENC_SEG_MAX, ENC_TARGET_UNITS = 16, 256, 2048  # kEncSegChunksMin, kEncSegChunks, kEncTargetUnits


def enc_template(bs: int) -> Tuple[int, int]:
    """(SPL, G) of enc_kernel_for: samples per lane, lanes per sub-block."""
    spl = 16 if bs > 64 else 8
    m, g = -(-bs // spl), 1
    while g < m:
        g *= 2
    return spl, g


def seg_chunks_rule(total_samples: int, cfg: Cfg) -> int:
    """enc_seg_chunks: chunks per unit for a batch of total_samples."""
    chunks, c = total_samples // (cfg.bs * cfg.cs), ENC_SEG_MAX
    while c > ENC_SEG_MIN and chunks // c < ENC_TARGET_UNITS:
        c >>= 1
    return c


def zz(delta: int) -> int:
    """The zig-zag code of a signed 16-bit difference (encode.h:119)."""
    assert -32768 <= delta <= 32767
    return (delta << 1) if delta >= 0 else ((-delta << 1) - 1)


def unzz(d: int) -> int:
    return (d >> 1) ^ -(d & 1)


def split_cost(d, fs: int) -> int:
    d = np.asarray(d, np.int64)
    return int(len(d) * (fs + 1) + (d >> fs).sum())


class Walk(NamedTuple):
    start: int
    tie0: bool      # bits0 == bits1: no walk
    dir: int
    steps: int      # candidates taken behind the first pair
    tie_steps: int  # of these, at an equal cost
    fs: int
    bits: int
    best: int       # the lowest cost of any fs 0..15


def split_rule(d, n_for_start: Optional[int] = None) -> Walk:
    """compute_best_split (encode.h:43-90) restated, to aim cases only."""
    d = np.asarray(d, np.int64)
    n, total = len(d), int(d.sum())
    start = max(0, (total // (n_for_start or n)).bit_length() - 2)
    b0, b1 = split_cost(d, start), split_cost(d, start + 1)
    cand, bits, direction = (start + 1, b1, 1) if b1 <= b0 else (start, b0, -1)
    steps = ties = 0
    if b0 != b1:
        while 0 < cand < 14:
            t = split_cost(d, cand + direction)
            if t > bits:
                break
            ties += t == bits
            bits, cand, steps = t, cand + direction, steps + 1
    return Walk(start, b0 == b1, direction, steps, ties, cand, bits, min(split_cost(d, f) for f in range(16)))


def aim_kind(d):
    """"zero", "raw" or the fs an encoder takes for these deltas, by the restated rule."""
    if not int(np.asarray(d, np.int64).sum()):
        return "zero"
    w = split_rule(d)
    return w.fs if w.fs < 14 and w.bits < 16 * len(d) else "raw"


def stored(cfg: Cfg, px: int, dirt: int = 0) -> int:
    t = (((px & 0xFFFF) << cfg.ulsb) & 0xFFFF) | dirt
    return _bswap(t) if cfg.big else t


def from_deltas(cfg: Cfg, first_px: Sequence[int], subs, dirt=None):
    """(Fields, input samples) of sub-blocks given as (kind, zig-zag deltas) in stream order; kind is "zero",
    "raw" or fs.  The running pixel of a component starts at first_px (the stream's initial value: its first
    delta is 0, codec.h:72) and, with ulsb > 0, stays inside [0, 2^(16 - ulsb)).  ``dirt`` maps a sub-block's
    index to unused low bits per sample: a raw sub-block stores them as they lie, in a zero sub-block they are in
    the input only (the encoder drops them)."""
    top = 1 << (16 - cfg.ulsb)
    px = list(first_px)
    seen = [False] * cfg.cs
    out, dirty = [], {}
    pos = 0
    for i, (kind, d) in enumerate(subs):
        c = i % cfg.cs
        d = [int(x) for x in d]
        if not seen[c]:
            assert d[0] == 0 and 0 <= px[c] < top, "a component's first sample is its own reference"
            seen[c] = True
        low = list(dirt[i]) if dirt and i in dirt else [0] * len(d)
        assert all(0 <= x < (1 << cfg.ulsb) for x in low)
        vals = []
        for x in d:
            assert 0 <= x <= 0xFFFF
            p = px[c] + unzz(x)
            assert cfg.ulsb == 0 or 0 <= p < top, "the pixel leaves its range: not what a 16-bit difference sees"
            px[c] = p & 0xFFFF
            vals.append(px[c])
        if kind == "zero":
            assert not any(d)
            out.append(Zero(len(d)))
            if any(low):
                dirty[i] = [stored(cfg, v, l) for v, l in zip(vals, low)]
        elif kind == "raw":
            out.append(Raw(tuple(stored(cfg, v, l) for v, l in zip(vals, low))))
        else:
            assert not any(low)
            out.append(Rice(kind, tuple((x >> kind, x & ((1 << kind) - 1)) for x in d)))
        pos += len(d)
    f = Fields(tuple(first_px), tuple(out))
    inp = expand(cfg, f)
    if dirty:  # the input of a dirty zero sub-block: sample j of sub-block i lies at chunk base + comp + cs * j
        inp = inp.copy()
        base = 0
        for g in range(0, len(out), cfg.cs):
            for c in range(cfg.cs):
                if g + c in dirty:
                    inp[base + c:base + cfg.cs * count(out[g]):cfg.cs] = dirty[g + c]
            base += cfg.cs * count(out[g])
    return f, inp


def enc_case(what: str, cfg: Cfg, first_px, dsubs, kinds=None, dirt=None) -> Case:
    """A case from deltas; kinds default to what the restated rule aims at (the host test proves them)."""
    kinds = kinds or [aim_kind(d) for d in dsubs]
    f, inp = from_deltas(cfg, first_px, list(zip(kinds, dsubs)), dirt)
    want = expand(cfg, f)
    return Case(what, cfg, build(cfg, f), len(want), want, OK, 0, None, None if inp is want else inp, f)


def deltas_of(cfg: Cfg, c: Case) -> List[np.ndarray]:
    """The zig-zag deltas of each sub-block of a case's input, in stream order: pixel differences mod 2^16."""
    inp = c.want if c.inp is None else c.inp
    px = np.array([px_read(cfg, int(v)) for v in inp], np.int64)
    out, last = [], [int(v) for v in c.fields.init]
    base = 0
    for g in range(0, len(c.fields.subs), cfg.cs):
        cnt = count(c.fields.subs[g])
        for k in range(cfg.cs):
            p = px[base + k:base + cfg.cs * cnt:cfg.cs]
            diff = (np.diff(np.concatenate(([last[k]], p))) + 32768) % 65536 - 32768
            out.append(np.where(diff >= 0, diff << 1, (-diff << 1) - 1))
            last[k] = int(p[-1])
        base += cfg.cs * cnt
    return out


def sub_bits(s: Sub) -> int:
    if isinstance(s, Zero):
        return 4
    if isinstance(s, Raw):
        return 4 + 16 * len(s.values)
    return 4 + sum(q for q, _ in s.codes) + len(s.codes) * (1 + s.fs)


def ones(n: int, s: int, skip_first: bool = True) -> List[int]:
    """n deltas of 0 and 1 with s ones, 0 < s < n: an encoder takes fs 0 (start 0, n + s < 2n), 4 + n + s bits."""
    assert 0 < s < n
    d = [0] * n
    for j in range(s):
        d[n - 1 - j] = 1
    return d


def dial(cfg: Cfg, nchunks: int, extra: int, rng=None) -> List[List[int]]:
    """Deltas of nchunks full chunks that take 4 * cs * nchunks + extra bits: zero sub-blocks, fs 0 sub-blocks of
    zeros and ones (n + s bits more, 0 < s < n) and raw sub-blocks (16 n bits more, noise from rng)."""
    n, slots = cfg.bs, cfg.cs * nchunks
    subs = [[0] * n for _ in range(slots)]
    at = slots - 1
    while rng is not None and extra >= 16 * n + (2 * n + 2) or extra == 16 * n:
        subs[at] = [0] + [int(x) for x in rng.integers(0x7000, 0xFFFF, n - 1)]
        extra -= 16 * n
        at -= 1
    if extra:
        b = max(1, -(-extra // (2 * n - 1)))
        assert b * (n + 1) <= extra <= b * (2 * n - 1) and b <= at + 1, (cfg, nchunks, extra)
        for j in range(b):
            s = (extra - b * n) // b + (j < (extra - b * n) % b)
            subs[at - j] = ones(n, s)
    return subs


def noise(rng, n: int) -> List[int]:
    """Deltas an encoder stores raw (start 13 or 14)."""
    return [int(x) for x in rng.integers(0x9000, 0xFFFF, n)]


def wave_groups(cfg: Cfg, f: Fields, lo: int = 0, hi: Optional[int] = None):
    """The sub-blocks one wave takes per iteration (64 / G of them), as index lists."""
    spw = 64 // enc_template(cfg.bs)[1]
    hi = len(f.subs) if hi is None else hi
    return [list(range(s, min(s + spw, hi))) for s in range(lo, hi, spw)]


def flush_trace(cfg: Cfg, f: Fields):
    """(complete words since the last flush after each iteration, flushes) of a one-wave encode: enc_flush
    streams out when F = (base >> 5) & ~15 reaches win_w0 + 256 words."""
    base, w0, words, flushes = 16 * cfg.cs, 0, [], 0
    for grp in wave_groups(cfg, f):
        base += sum(sub_bits(f.subs[i]) for i in grp)
        words.append((base >> 5) - w0)
        assert words[-1] < ENC_WIN_WORDS - 1
        F = (base >> 5) & ~15
        if F >= w0 + ENC_FLUSH_WORDS:
            w0, flushes = F, flushes + 1
    return words, flushes


def segments_of(cfg: Cfg, f: Fields, segc: int = ENC_SEG_MIN):
    """(offsets o_k, lengths L_k in bits) of the units a stream of more than segc chunks is split into."""
    n = len(f.subs) // cfg.cs
    if n <= segc:
        return [0], [16 * cfg.cs + sum(sub_bits(s) for s in f.subs)]
    L = []
    for lo in range(0, n, segc):
        L.append(sum(sub_bits(s) for s in f.subs[lo * cfg.cs:(lo + segc) * cfg.cs]) + (16 * cfg.cs if lo == 0 else 0))
    return [sum(L[:k]) for k in range(len(L))], L


# ---------------------------------------------------------------------------------------------------------------
# enc_split_start
# ---------------------------------------------------------------------------------------------------------------

START_BS_ALL = (16, 29)          # every n in 1..bs
START_BS_SOME = (128, 200, 500)  # n in {1, 2, 3, 7, 8, 9, bs - 1, bs}


def start_ns(bs: int) -> List[int]:
    return list(range(1, bs + 1)) if bs in START_BS_ALL else [1, 2, 3, 7, 8, 9, bs - 1, bs]


@functools.lru_cache(maxsize=None)
def enc_split_start() -> List[Case]:
    """A zero chunk, then one sub-block of n deltas 2^m (m = 0..13) per component, one of them lowered by 1, left
    or raised by 1: sums n 2^m - 1, n 2^m, n 2^m + 1.  With all deltas 2^m the costs at m - 1 and m are equal,
    the walk stops at start + 1 and the chosen fs max(m, 1) reveals `start`.  n < bs is the ragged last chunk.
    The second component of a cs 2 stream runs m + 5 and the next variant."""
    out = []
    i = 0
    for bs in START_BS_ALL + START_BS_SOME:
        for n in start_ns(bs):
            for m in range(14):
                for var in (-1, 0, 1):
                    cfg = Cfg(bs, 1 + i % 2, i % 4 < 2, 0)
                    i += 1
                    subs = [[0] * bs] * cfg.cs
                    for c in range(cfg.cs):
                        mc, vc = (m + 5 * c) % 14, (var + 1 + c) % 3 - 1
                        d = [1 << mc] * n
                        d[n // 2] += vc
                        subs.append(d)
                    out.append(enc_case(f"start bs={bs} n={n} m={m} var={var:+d} cs={cfg.cs} {'be' if cfg.big else 'le'}",
                                        cfg, (0x4000 + i,) * cfg.cs, subs))
    return out


# ---------------------------------------------------------------------------------------------------------------
# enc_split_walk
# ---------------------------------------------------------------------------------------------------------------

WALK_BS = (16, 64, 128)


def _walk_subs(bs: int):
    """[(label, deltas)]: every walk the rule can take."""
    rng = np.random.default_rng(4300 + bs)
    out = []

    def mix(lo_hi_share):
        d = []
        for (lo, hi), share in lo_hi_share:
            d += [int(x) for x in rng.integers(lo, hi, max(1, round(share * bs)))]
        d = (d + [d[-1]] * bs)[:bs]
        return [d[j] for j in rng.permutation(bs)]

    for f in range(1, 14):
        s = f - 1  # the start aimed at
        out.append((f"tie_step start={s}", mix([((1 << f, 2 << f), 1.0)])))                  # start+1, = cost, start+2
        out.append((f"strict_step start={s}", mix([((1 << f, (1 << f) + 1), 0.6), ((3 << f, (3 << f) + 1), 0.4)])))
        out.append((f"down start={s + 1}", mix([(((1 << f) * 2 - 2, (1 << f) * 2), 0.49),    # direction -1 at start
                                                 (((3 << f) * 2 - 2, (3 << f) * 2), 0.51)])))
        out.append((f"plain start={s}", mix([((0, 2 << f), 1.0)])))
    out.append(("start0 down", mix([((0, 1), 0.7), ((1, 2), 0.3)])))
    out.append(("start0 up", mix([((1, 4), 1.0)])))
    # into fs 14 and 15
    out.append(("13->14 by an equal-cost step from start 12", mix([((1 << 13, 1 << 14), 1.0)])))
    out.append(("14 at the first pair from start 13, equal", mix([((1 << 14, 3 << 13), 1.0)])))
    out.append(("14 at the first pair from start 13, lower", mix([((3 << 13, 1 << 15), 1.0)])))
    out.append(("13 kept from start 13", mix([((0x1F00, 0x2000), 0.45), ((0x5F00, 0x6000), 0.55)])))
    out.append(("15 at the first pair from start 14, equal", [0x8000] * bs))
    out.append(("15 at the first pair from start 14, lower", mix([((0xC000, 0x10000), 1.0)])))
    out.append(("14 kept from start 14", mix([((0x3F00, 0x4000), 0.3), ((0xBF00, 0xC000), 0.7)])))
    return out


@functools.lru_cache(maxsize=None)
def enc_split_walk_fields():
    out = []
    for bs in WALK_BS:
        subs = _walk_subs(bs)
        for cs in (1, 2):
            per = 6 * cs
            for k in range(0, len(subs), per):
                part = subs[k:k + per]
                part = part + part[:(-len(part)) % cs]
                cfg = Cfg(bs, cs, (k // per) % 2 == 0, 0)
                dsubs = [[0] * bs] * cs + [d for _, d in part]
                out.append((f"walk bs={bs} cs={cs} #{k // per}", cfg, dsubs, [l for l, _ in part]))
    return out


@functools.lru_cache(maxsize=None)
def enc_split_walk() -> List[Case]:
    """Every walk the split rule can take (see the note above): direction -1 and +1 at the first pair, one more
    step at a lower and at an equal cost, fs 13 reached and kept, fs 14 from starts 12, 13 and 14 and fs 15 from
    start 14 (raw)."""
    return [enc_case(what, cfg, (0x2000 + 7 * i,) * cfg.cs, dsubs)
            for i, (what, cfg, dsubs, _) in enumerate(enc_split_walk_fields())]


# ---------------------------------------------------------------------------------------------------------------
# enc_emit_paths
# ---------------------------------------------------------------------------------------------------------------

EMIT_FULL = (8, 16, 32, 64, 128, 256, 512)  # bs == G * SPL: every lane full
EMIT_RAGGED = (29, 200)                     # SPL 8 and SPL 16 with empty lanes: the per-sample path
EMIT_T = (31, 32, 33, 34)                   # 2k + q of the largest odd-sample run


def _emit_target(rng, bs: int, fs: int, T: int):
    """A sub-block an encoder codes at fs whose largest odd-sample run is T - 2 (fs + 1), in one sample."""
    k = fs + 1
    q = T - 2 * k
    for _ in range(400):
        base = int(rng.integers(max(0, fs - 1), fs + 2))
        d = [int(x) for x in rng.integers(0, 2 << base, bs)] if bs > 1 else [0]
        at = 2 * int(rng.integers(0, bs // 2)) + 1
        d[at] = (q << fs) | int(rng.integers(0, 1 << fs))
        if d[at] > 0xFFFF or aim_kind(d) != fs:
            continue
        if sum(1 for j in range(1, bs, 2) if d[j] >> fs >= q) == 1:
            return d, at
    return None


def _emit_long_even(rng, bs: int, fs: int):
    """A sub-block coded at fs with an even-sample run of 1000 zeros or more and no odd run: the other deltas lie
    below 2^fs, so the average is about 2.5 * 2^fs (start = fs) and the run's ceil(q / 2) < n keeps the first
    pair from going up.  That needs n > 500: bs 512 only."""
    d = [int(x) for x in rng.integers(0, 1 << fs, bs)]
    at = 2 * int(rng.integers(0, bs // 2))
    d[at] = (int(rng.integers(1000, 1022)) << fs) | d[at]
    return d if aim_kind(d) == fs else None


@functools.lru_cache(maxsize=None)
def enc_emit_paths_fields():
    out = []
    for bs in EMIT_FULL + EMIT_RAGGED:
        spw = 64 // enc_template(bs)[1]
        for cs in ((1, 2) if bs in (16, 128, 29) else (1,)):
            rng = np.random.default_rng(77 * bs + cs)
            targets = []
            for fs in range(14):
                for T in EMIT_T:
                    t = _emit_target(rng, bs, fs, T)
                    if t:
                        targets.append(((fs, T), t[0]))
            if bs == 512:
                for fs in range(6):
                    d = _emit_long_even(rng, bs, fs)
                    if d:
                        targets.append(("long_even", d))
            # one target per iteration of the wave, at a varying place; the other sub-blocks of the iteration are
            # a short low-fs one (which moves the header's phase) and zero sub-blocks
            per_stream = max(1, 4096 // (spw * bs))
            for k in range(0, len(targets), per_stream):
                dsubs, meta = [], []
                for j, (label, d) in enumerate(targets[k:k + per_stream]):
                    group = [[0] * bs for _ in range(spw)]
                    group[0] = [0] + [int(x) for x in rng.integers(0, 4, bs - 1)]
                    if not any(group[0]):
                        group[0] = [0] * bs
                    at = cs + (k + j) % (spw - cs)
                    group[at] = d
                    meta.append((len(dsubs) + at, label))
                    dsubs += group
                cfg = Cfg(bs, cs, (k // per_stream) % 2 == 0, 0)
                out.append((f"emit bs={bs} cs={cs} #{k // per_stream}", cfg, dsubs, meta))
    return out


@functools.lru_cache(maxsize=None)
def enc_emit_paths() -> List[Case]:
    """For every full-lane shape and one ragged shape per SPL, and every fs 0..13: sub-blocks whose largest
    odd-sample run makes 2k + q 31, 32 (the pair path), 33 and 34 (the two-code path) in exactly one lane of the
    wave, the other sub-blocks of the iteration short or zero; even-sample runs of 1000 and more beside short odd
    ones; the headers at every bit phase mod 32."""
    return [enc_case(what, cfg, (0x7000 + i,) * cfg.cs, dsubs)
            for i, (what, cfg, dsubs, _) in enumerate(enc_emit_paths_fields())]


# ---------------------------------------------------------------------------------------------------------------
# enc_flush_edges
# ---------------------------------------------------------------------------------------------------------------

FLUSH_WORDS = (255, 256, 257, 271, 272, 273)
FLUSH_DIAL = ((29, 1), (29, 2))
FLUSH_RAW = tuple((bs, cs) for bs in (8, 16, 32, 64, 128, 256, 512) for cs in (1, 2))


def _flush_plan(cfg: Cfg, targets):
    """Raw sub-blocks per iteration such that the complete words since the last flush are each of ``targets`` in
    turn after some iteration, and below 255 after every iteration between."""
    spw = 64 // enc_template(cfg.bs)[1]
    zero_it, raw = 4 * spw, 16 * cfg.bs
    rel, plan = 16 * cfg.cs, []
    for W in targets:
        hit = None
        for k in range(1, 60):
            for R in range(0, spw * k + 1):
                end = rel + zero_it * k + raw * R
                last = min(spw, R)
                before = end - zero_it - raw * last
                if end >> 5 == W and (k == 1 or (before >> 5 < 255 and R - last <= spw * (k - 1))):
                    hit = (k, R, last)
                    break
            if hit:
                break
        if not hit:  # (not every count can follow every other: the next one of the list is tried)
            continue
        k, R, last = hit
        rest = R - last
        for j in range(k - 1):
            r = min(spw, rest)
            plan.append(r)
            rest -= r
        plan.append(last)
        rel += zero_it * k + raw * R
        F = (rel >> 5) & ~15
        if F >= ENC_FLUSH_WORDS:
            rel -= 32 * F
    return plan


@functools.lru_cache(maxsize=None)
def enc_flush_edges() -> List[Case]:
    """One-wave encodes whose complete words since the last flush are 255, 256, 257, 271, 272 and 273 after an
    iteration (raw and zero sub-blocks dial the bits), at least three flushes per stream, a last ragged fs 0
    chunk that takes the total bits to every residue mod 32; and all-raw streams (the worst case, 256 or 512
    words per iteration) for every kernel template and cs."""
    out = []
    i = 0
    for bs, cs in FLUSH_DIAL:
        cfg = Cfg(bs, cs, True, 0)
        spw = 64 // enc_template(bs)[1]
        rng = np.random.default_rng(900 + bs + cs)
        for r in range(32):
            targets = [FLUSH_WORDS[(r + j) % 6] for j in range(6)]
            dsubs = []
            for raws in _flush_plan(cfg, targets):
                dsubs += [noise(rng, bs) for _ in range(raws)] + [[0] * bs] * (spw - raws)
            dsubs[0] = [0] + dsubs[0][1:]
            if cs == 2:
                dsubs[1] = [0] + dsubs[1][1:]
            # the last chunk: n + s + 4 cs more bits, the total at residue r
            have = 16 * cs + sum(4 + 16 * bs * any(d) for d in dsubs) + 4 * cs
            t = 16 + (r - have - 16) % 32  # n + s
            n = t // 2 + 1
            s = t - n
            dsubs += [ones(n, s)] + [[0] * n] * (cs - 1)
            out.append(enc_case(f"flush dial bs={bs} cs={cs} r={r}", cfg, (0x0100 + i,) * cs, dsubs))
            i += 1
    for bs, cs in FLUSH_RAW:
        spl, g = enc_template(bs)
        rng = np.random.default_rng(950 + bs + cs)
        for ragged in (0, bs // 2 + 1):
            cfg = Cfg(bs, cs, ragged == 0, 0)
            nsub = (64 // g) * (5 if spl == 16 else 7) - cs
            dsubs = [noise(rng, bs) for _ in range(nsub)] + [noise(rng, ragged) for _ in range(cs if ragged else 0)]
            for c in range(cs):
                dsubs[c] = [0] + dsubs[c][1:]
            out.append(enc_case(f"flush all raw bs={bs} cs={cs} ragged={ragged}", cfg, (0x0100 + i,) * cs, dsubs,
                                ["raw"] * len(dsubs)))
            i += 1
    return out


# ---------------------------------------------------------------------------------------------------------------
# enc_shapes
# ---------------------------------------------------------------------------------------------------------------

SHAPE_BS = (1, 7, 8, 9, 16, 17, 29, 32, 33, 64, 65, 99, 128, 129, 200, 256, 257, 500, 512)
SHAPE_CFG = ((True, 0), (False, 3), (True, 6))


def wander(rng, cfg: Cfg, n: int, px: int, scale: int) -> Tuple[List[int], int]:
    """n zig-zag deltas of a random walk of the given scale that stays inside the pixel range."""
    top = (1 << (16 - cfg.ulsb)) - 1
    d = []
    for step in (rng.normal(0, scale, n) if scale else np.zeros(n)):
        p = min(top, max(0, px + min(32767, max(-32768, int(round(step))))))
        d.append(zz(p - px))
        px = p
    return d, px


def shape_ns(bs: int, cs: int) -> List[int]:
    chunk = bs * cs
    ns = {0, cs, 2 * cs, chunk - cs, chunk, chunk + cs} | {3 * chunk + cs * r for r in (1, 2, bs - 1) if 0 < r < bs}
    return sorted(x for x in ns if x >= 0)


@functools.lru_cache(maxsize=None)
def enc_shapes() -> List[Case]:
    """Every block size at which the kernel template, the lane count or the ragged handling changes, one and two
    components, three pixel formats; stream lengths 0, cs, 2 cs, one chunk and cs either way, and three chunks
    with a ragged last one of 1, 2 and bs - 1 samples.  Random walks whose scale changes per sub-block (zero,
    every fs, raw)."""
    out = []
    i = 0
    for bs in SHAPE_BS:
        for cs in (1, 2):
            for big, ulsb in SHAPE_CFG:
                cfg = Cfg(bs, cs, big, ulsb)
                rng = np.random.default_rng(5000 + 7 * bs + 3 * cs + ulsb)
                top = 1 << (16 - ulsb)
                for n in shape_ns(bs, cs):
                    i += 1
                    per = n // cs
                    first = [int(rng.integers(0, top)) for _ in range(cs)]
                    px, dsubs = list(first), []
                    for lo in range(0, per, bs):
                        for c in range(cs):
                            scale = (0, 1, 3, 40, 700, top // 3, 2, 9000)[int(rng.integers(0, 8))]
                            d = wander(rng, cfg, min(bs, per - lo), px[c], min(scale, top))[0]
                            if lo == 0:
                                d[0] = 0
                            d, px[c] = _rewalk(cfg, px[c], d)
                            dsubs.append(d)
                    out.append(enc_case(f"shape {cfg} n={n}", cfg, tuple(first) if n else (0,) * cs, dsubs))
    return out


def _rewalk(cfg: Cfg, px: int, d: List[int]) -> Tuple[List[int], int]:
    """The deltas clamped so that the walk from px stays in range, and its end."""
    top = (1 << (16 - cfg.ulsb)) - 1
    out = []
    for x in d:
        p = min(top, max(0, px + unzz(x)))
        out.append(zz(p - px))
        px = p
    return out, px


# ---------------------------------------------------------------------------------------------------------------
# enc_segments
# ---------------------------------------------------------------------------------------------------------------

SEG_SHORT = ("4", "4cs", "8", "20", "31", "32", "33")  # bits of a short last segment
SEG_SH = (0, 3, 8, 11, 24, 27, 28, 31)                # o_1 % 32 beside them


def _short_last(cfg: Cfg, name: str) -> List[List[int]]:
    """The chunks of a last segment of that many bits."""
    bits = 4 * cfg.cs if name == "4cs" else int(name)
    if bits % (4 * cfg.cs) == 0 and bits <= 8:
        full = bits // (4 * cfg.cs) - 1
        return [[0] * cfg.bs] * (cfg.cs * full) + [[0] * 3] * cfg.cs  # (zero chunks, the last ragged)
    ns = bits - 4 * cfg.cs  # n + s of a ragged fs 0 sub-block (the other component's is zero)
    n = ns // 2 + 1
    assert ns > 2 and n < cfg.bs, (cfg, name)
    return [ones(n, ns - n)] + [[0] * n] * (cfg.cs - 1)


@functools.lru_cache(maxsize=None)
def enc_segments_fields():
    out = []
    S = ENC_SEG_MIN
    i = 0
    for bs, cs in ((16, 1), (16, 2), (29, 1), (29, 2)):
        cfg = Cfg(bs, cs, bs == 16, 0)
        rng = np.random.default_rng(600 + bs + cs)
        base0 = 16 * cs + 4 * cs * S   # segment 0 of zero sub-blocks

        def seg(extra, raws=False):
            return dial(cfg, S, extra, rng if raws else None)

        def typical_tail(chunks, ragged):
            d = []
            for j in range(chunks * cs):
                d.append(wander(rng, cfg, bs, 0x4000, (0, 2, 30, 9000)[j % 4])[0])
            return d + ([wander(rng, cfg, ragged, 0x4000, 5)[0] for _ in range(cs)] if ragged else [])

        def add(what, segs, aim):
            nonlocal i
            dsubs = [list(d) for s in segs for d in s]
            for c in range(cs):
                dsubs[c][0] = 0
            # (ulsb 0: the deltas of walks drawn apart are one walk mod 2^16)
            out.append((f"seg {what} bs={bs} cs={cs}", cfg, (0x4000 + i,) * cs, dsubs, aim))
            i += 1

        for r in range(32):  # o_1 at every residue, two segments; then o_2, o_3 with three to five
            e = (r - base0) % 32 + 2 * bs + 2 + 32
            add(f"o1%32={r} two", [seg(e + 32 * (r % 3) * 3, raws=r % 2 == 1), typical_tail(1 + r % 5, r % bs)], ("o1", r))
            nseg = 3 + r % 3
            o_1 = base0 + 2 * bs + 2 + r
            mids = [seg((r - o_1 - 4 * cs * S) % 32 + 2 * bs + 2 + 32 if k == 1 else 2 * bs + 2 + (5 * r + 7 * k) % 29,
                        raws=(r + k) % 4 == 0) for k in range(1, nseg - 1)]
            add(f"o2%32={r} nseg={nseg}", [seg(2 * bs + 2 + r)] + mids + [typical_tail(r % 3, 1 + r % (bs - 1))], ("ok", r))
        for name in SEG_SHORT:
            if name == "4" and cs == 2:
                continue
            for sh in SEG_SH:
                e = (sh - base0) % 32 + 2 * bs + 2 + 32
                add(f"short last {name} sh={sh} two", [seg(e), _short_last(cfg, name)], ("short2", name, sh))
            for sh in SEG_SH[::3]:
                e = (sh - base0) % 32 + 2 * bs + 2 + 32
                add(f"short last {name} sh={sh} minimal middle", [seg(e), seg(0), _short_last(cfg, name)],
                    ("short3", name, sh))
                add(f"short last {name} sh={sh} four", [seg(e, raws=True), seg(0), seg(2 * bs + 9), _short_last(cfg, name)],
                    ("short4", name, sh))
    return out


@functools.lru_cache(maxsize=None)
def enc_segments() -> List[Case]:
    """Streams of more than 16 chunks, which a small batch splits into units of 16 chunks: two to five segments
    whose lengths zero, fs 0 and raw sub-blocks dial, so that o_1 % 32 and some o_k % 32 (k >= 2) take every
    residue, middle segments have the minimal 64 cs bits, and the last segment has 4, 4 cs, 8, 20, 31, 32 and 33
    bits beside o_1 % 32 of 0..31 (L_1 < 32 - sh in many)."""
    return [enc_case(what, cfg, first, dsubs) for what, cfg, first, dsubs, _ in enc_segments_fields()]


# ---------------------------------------------------------------------------------------------------------------
# enc_values
# ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def enc_values() -> List[Case]:
    """Differences of +-1, +-32767 and -32768, 0 -> 0xFFFF and back, initial values with the high bit set, both
    byte orders; with ulsb 3 and 15 dirty unused low bits in a sub-block that is otherwise all zero (dropped) and
    in a raw sub-block (stored as they lie); a raw sub-block followed by Rice and by zero."""
    out = []
    for bs, cs in ((16, 1), (128, 1), (32, 2), (29, 2)):
        for big in (True, False):
            rng = np.random.default_rng(8000 + bs + cs + big)
            cfg = Cfg(bs, cs, big, 0)
            ext = [zz(1), zz(-1), zz(32767), zz(-32768), zz(-32767), zz(1), zz(-1), zz(32767), zz(-32767), 0]
            for init in (0, 0xFFFF, 0x8000, 0x8001):
                subs = [[0] * bs] * cs
                subs += [[ext[(j + 3 * c) % len(ext)] for j in range(bs)] for c in range(cs)]       # (raw)
                subs += [[zz(1) if j % 2 else zz(-1) for j in range(bs)] for c in range(cs)]        # +-1
                subs += [[zz(-1)] + [0] * (bs - 1) for c in range(cs)]                              # one step
                subs += [[zz(32767 if j == 5 else -32768 if j == 9 else -32767 if j == 12 else j % 3 - 1)
                          for j in range(bs)] for c in range(cs)]                                   # extremes in Rice
                subs += [[0] * bs] * cs
                subs += [[zz(-1 if j == 0 else 1 if j == 1 else 0) for j in range(bs)] for c in range(cs)]
                out.append(enc_case(f"values extremes {cfg} init={init:#06x}", cfg, (init,) * cs, subs))
            # 0 -> 0xFFFF and back, alone in otherwise zero sub-blocks
            subs = [[0] * bs] * cs + [[0] * 3 + [zz(-1)] + [0] * (bs - 4)] * cs + [[zz(1)] + [0] * (bs - 1)] * cs
            out.append(enc_case(f"values 0 to 0xffff and back {cfg}", cfg, (0,) * cs, subs))
            for ulsb in (3, 15):
                cfg = Cfg(bs, cs, big, ulsb)
                top = 1 << (16 - ulsb)
                hi = top >> 1  # (the pixel's high bit)
                low = lambda n: [int(x) for x in rng.integers(0, 1 << ulsb, n)]
                step = [zz(1) if top > 2 else 0] + [0] * (bs - 1)
                back = [zz(-1) if top > 2 else 0] + [0] * (bs - 1)
                nz = lambda n: [0] + [int(x) for x in rng.integers(0, 2, n - 1) * (2 if top > 2 else 0)]
                # dirty zero, a raw sub-block (dirty) then Rice, then zero (dirty), raw then zero, a ragged dirty zero
                raw_d = [zz(int(x)) for x in rng.integers(-1, 2, bs)] if top > 2 else [0] * bs
                kinds, subs, dirt = [], [], {}
                def put(kind, d, dirty=False):
                    if dirty:
                        dirt[len(subs)] = low(len(d))
                    kinds.append(kind if kind != "aim" else aim_kind(d))
                    subs.append(d)
                for c in range(cs):
                    put("zero", [0] * bs, dirty=True)
                for c in range(cs):
                    # (13-bit pixels: raw needs every delta in [3 * 2^12, 2^14), the equal-cost step 13 -> 14)
                    put("raw", [0] * bs if top == 2 else ([zz(-6200), zz(6200)] * bs)[:bs], dirty=True)
                if top == 2:  # (one pixel bit: only the dirt makes a sub-block raw, so none is)
                    kinds[-cs:] = ["zero"] * cs
                for c in range(cs):
                    put("aim", step)
                for c in range(cs):
                    put("zero", [0] * bs, dirty=True)
                for c in range(cs):
                    put("aim", back)
                for c in range(cs):
                    put("raw" if top > 2 else "zero", [0] * bs if top == 2 else ([zz(6200), zz(-6200)] * bs)[bs % 2 == 0:][:bs])
                for c in range(cs):
                    put("zero", [0] * bs)
                for c in range(cs):
                    put("zero", [0] * 5, dirty=True)
                for init in ((6200, 6201) if top > 2 else (1, 0)):
                    out.append(enc_case(f"values dirt {cfg} init={init:#06x}", cfg, (init,) * cs, subs, kinds, dirt))
    return out


ENC_FAMILIES = {"enc_split_start": enc_split_start, "enc_split_walk": enc_split_walk,
                "enc_emit_paths": enc_emit_paths, "enc_flush_edges": enc_flush_edges, "enc_shapes": enc_shapes,
                "enc_segments": enc_segments, "enc_values": enc_values}
