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
