"""A FLAC frame writer driven by explicit fields, for the tests only.

Nothing here chooses anything: the caller names every header code, every
subframe kind, the predictor, the partition order and each partition's Rice
parameter or escape width, and gives the true samples; the writer computes
the residuals (RFC 9639 sections 9.2.6 and 9.2.7) in Python ints and lays the
bits down MSB first.  It records the bit position at which every code and
every partition starts and ends, so that a test can prove that a case has the
geometry it claims.  It imports neither of the readers nor the codec.
"""

from __future__ import annotations

from dataclasses import dataclass, field


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_T16 = []
for _v in range(256):
    _c = _v << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _T16.append(_c)


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


class BitWriter:
    """MSB-first; ``pos`` is the number of bits written."""

    def __init__(self):
        self.buf, self.acc, self.nacc, self.pos = bytearray(), 0, 0, 0

    def put(self, v: int, n: int):
        if n == 0:
            return
        assert 0 <= v < (1 << n), (v, n)
        self.acc = (self.acc << n) | v
        self.nacc += n
        self.pos += n
        if self.nacc >= 512:
            r = self.nacc & 7
            self.buf += (self.acc >> r).to_bytes((self.nacc - r) // 8, "big")
            self.acc &= (1 << r) - 1
            self.nacc = r

    def signed(self, v: int, n: int):
        if n == 0:
            assert v == 0
            return
        assert -(1 << (n - 1)) <= v < (1 << (n - 1)), (v, n)
        self.put(v & ((1 << n) - 1), n)

    def unary(self, q: int):
        self.put(1, q + 1)

    def align(self):
        self.put(0, -self.pos & 7)

    def bytes(self) -> bytes:
        assert self.pos % 8 == 0
        return bytes(self.buf) + (self.acc.to_bytes(self.nacc // 8, "big") if self.nacc else b"")


def utf8(v: int) -> bytes:
    """The coded number of a frame header: UTF-8's scheme extended to 36 bits (section 9.1.5)."""
    if v < 0x80:
        return bytes([v])
    for more in range(1, 7):
        if v < 1 << (6 * more + 6 - more):
            lead = (0xFF << (7 - more)) & 0xFF
            out = [lead | (v >> (6 * more))]
            out += [0x80 | ((v >> (6 * j)) & 0x3F) for j in range(more - 1, -1, -1)]
            return bytes(out)
    raise ValueError("coded number above 36 bits")


def blocksize_field(bs: int, code: int):
    """The extra header bytes of block-size ``code`` for ``bs``; raises when the code cannot express it."""
    if code == 1:
        ok, extra = bs == 192, b""
    elif 2 <= code <= 5:
        ok, extra = bs == 576 << (code - 2), b""
    elif code == 6:
        ok, extra = 1 <= bs <= 256, bytes([(bs - 1) & 0xFF])
    elif code == 7:
        ok, extra = 1 <= bs <= 65536, ((bs - 1) & 0xFFFF).to_bytes(2, "big")
    elif 8 <= code <= 15:
        ok, extra = bs == 256 << (code - 8), b""
    else:
        ok, extra = False, b""
    if not ok:
        raise ValueError(f"block size code {code} cannot express {bs}")
    return extra


SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


@dataclass
class Residual:
    """method: 0 (4-bit parameters) or 1 (5-bit); order: the partition order; params: per partition a Rice
    parameter, or ("esc", width) for raw samples of ``width`` bits."""
    method: int = 0
    order: int = 0
    params: tuple = (0,)


@dataclass
class Sub:
    kind: str                 # "constant", "verbatim", "fixed", "lpc", "raw"
    samples: list = None      # the true samples of this coded channel
    order: int = 0
    precision: int = 0
    shift: int = 0
    coefs: tuple = ()
    residual: Residual = None
    wasted: int = 0
    bits: list = None         # raw: [(value, width)] after which nothing is added
    raw_residual: list = None  # [(value, width)] in place of the residual section


def constant(samples, wasted=0):
    return Sub("constant", list(samples), wasted=wasted)


def verbatim(samples, wasted=0):
    return Sub("verbatim", list(samples), wasted=wasted)


def fixed(order, samples, residual=None, wasted=0, raw_residual=None):
    return Sub("fixed", list(samples), order=order, residual=residual or Residual(), wasted=wasted,
               raw_residual=raw_residual)


def lpc(order, precision, shift, coefs, samples, residual=None, wasted=0):
    return Sub("lpc", list(samples), order=order, precision=precision, shift=shift, coefs=tuple(coefs),
               residual=residual or Residual(), wasted=wasted)


def raw_subframe(bits, samples=()):
    """A subframe given as [(value, width)]: what the writer would refuse to write."""
    return Sub("raw", list(samples), bits=list(bits))


def residuals_of(sub: Sub, samples):
    """sample - prediction, in Python ints (coefficients newest sample first)."""
    if sub.kind == "fixed":
        coef, shift = FIXED[sub.order], 0
    else:
        coef, shift = sub.coefs, sub.shift
    o = sub.order
    out = []
    for i in range(o, len(samples)):
        acc = 0
        for j in range(o):
            acc += coef[j] * samples[i - 1 - j]
        out.append(samples[i] - (acc >> shift))
    return out


def fold(r: int) -> int:
    return (r << 1) if r >= 0 else ((-r - 1) << 1) | 1


def unfold(u: int) -> int:
    return -(u >> 1) - 1 if u & 1 else u >> 1


@dataclass
class Marks:
    """Bit positions of one subframe: ``start``/``end`` of the subframe, partitions as (start, end) from the
    parameter's first bit to the last code's end, ``first`` the first code's (or raw sample's) start per
    partition, codes as (start, end) per residual in order."""
    start: int = 0
    end: int = 0
    parts: list = field(default_factory=list)
    first: list = field(default_factory=list)
    codes: list = field(default_factory=list)
    params: list = field(default_factory=list)  # per partition ("rice", k) or ("esc", width)

    def shifted(self, by: int) -> "Marks":
        return Marks(self.start + by, self.end + by, [(a + by, b + by) for a, b in self.parts],
                     [a + by for a in self.first], [(a + by, b + by) for a, b in self.codes], list(self.params))


def write_residual(w: BitWriter, res: Residual, values, bs: int, order: int, m: Marks, allow_wide: bool):
    assert res.method in (0, 1)
    pbits = 5 if res.method else 4
    po = res.order
    if bs % (1 << po) or (bs >> po) < order:
        raise ValueError(f"partition order {po} does not fit block size {bs}, predictor order {order}")
    assert len(res.params) == 1 << po and len(values) == bs - order
    if not allow_wide and any(abs(v) >= 1 << 31 for v in values):
        raise ValueError("a residual outside the range of RFC 9639 section 9.2.7.3")
    w.put(res.method, 2)
    w.put(po, 4)
    at = 0
    for p, par in enumerate(res.params):
        n = (bs >> po) - (order if p == 0 else 0)
        start = w.pos
        if isinstance(par, tuple):
            width = par[1]
            assert par[0] == "esc" and 0 <= width < 32
            w.put((1 << pbits) - 1, pbits)
            w.put(width, 5)
            m.params.append(("esc", width))
            m.first.append(w.pos)
            for v in values[at:at + n]:
                a = w.pos
                w.signed(v, width)
                m.codes.append((a, w.pos))
        else:
            assert 0 <= par < (1 << pbits) - 1
            w.put(par, pbits)
            m.params.append(("rice", par))
            m.first.append(w.pos)
            for v in values[at:at + n]:
                u = fold(v)
                a = w.pos
                w.unary(u >> par)
                w.put(u & ((1 << par) - 1), par)
                m.codes.append((a, w.pos))
        m.parts.append((start, w.pos))
        at += n


def write_subframe(w: BitWriter, sub: Sub, bs: int, bps: int, allow_wide: bool = False) -> Marks:
    """``sub`` for a coded channel of ``bps`` bits (the side channel's extra bit included)."""
    m = Marks(start=w.pos)
    if sub.kind == "raw":
        for v, n in sub.bits:
            w.put(v, n)
        m.end = w.pos
        return m
    assert len(sub.samples) == bs
    ws = sub.wasted
    if not 0 <= ws < bps:
        raise ValueError("wasted bits leave no sample bits")
    if ws and any(v & ((1 << ws) - 1) for v in sub.samples):
        raise ValueError("a sample has a set bit among the wasted ones")
    b = bps - ws
    s = [v >> ws for v in sub.samples]
    if any(not -(1 << (b - 1)) <= v < (1 << (b - 1)) for v in s):
        raise ValueError(f"a sample does not fit {b} bits")
    kind = {"constant": 0, "verbatim": 1, "fixed": 8 + sub.order, "lpc": 31 + sub.order}[sub.kind]
    w.put(0, 1)
    w.put(kind, 6)
    w.put(1 if ws else 0, 1)
    if ws:
        w.unary(ws - 1)
    if sub.kind == "constant":
        if any(v != s[0] for v in s):
            raise ValueError("a constant subframe of differing samples")
        w.signed(s[0], b)
    elif sub.kind == "verbatim":
        m.first.append(w.pos)
        for v in s:
            w.signed(v, b)
    else:
        o = sub.order
        if sub.kind == "fixed" and not 0 <= o <= 4 or sub.kind == "lpc" and not 1 <= o <= 32:
            raise ValueError("predictor order")
        if o > bs:
            raise ValueError("predictor order above the block size")
        for v in s[:o]:
            w.signed(v, b)
        if sub.kind == "lpc":
            if not 1 <= sub.precision <= 15 or not 0 <= sub.shift <= 15 or len(sub.coefs) != o:
                raise ValueError("LPC precision, shift or coefficient count")
            w.put(sub.precision - 1, 4)
            w.signed(sub.shift, 5)
            for c in sub.coefs:
                w.signed(c, sub.precision)
        if sub.raw_residual is not None:
            for v, n in sub.raw_residual:
                w.put(v, n)
        else:
            write_residual(w, sub.residual, residuals_of(sub, s), bs, o, m, allow_wide)
    m.end = w.pos
    return m


@dataclass
class Frame:
    data: bytes
    blocksize: int
    channels: list   # decoded per-channel samples (after stereo reconstruction)
    marks: list      # one Marks per subframe, bits from the frame's first byte
    header_len: int


def frame(blocksize, subframes, bps, *, bs_code, rate_code=9, rate_extra=None, size_code=None, assignment=None,
          number=0, variable=False, allow_wide=False) -> Frame:
    """One frame.  ``assignment``: None for len(subframes) independent channels, or "left_side", "right_side",
    "mid_side" (two subframes; the side and mid subframes carry side and mid values).  ``size_code``: None for the
    explicit code of ``bps``, or 0 (from STREAMINFO)."""
    nsub = len(subframes)
    if assignment is None:
        if not 1 <= nsub <= 8:
            raise ValueError("1 to 8 independent channels")
        acode = nsub - 1
    else:
        acode = {"left_side": 8, "right_side": 9, "mid_side": 10}[assignment]
        if nsub != 2:
            raise ValueError("stereo assignments take two subframes")
    if size_code is None:
        size_code = SIZE_CODES[bps]
    if not 0 <= rate_code <= 14:
        raise ValueError("sample rate code")
    rx = {12: 1, 13: 2, 14: 2}.get(rate_code, 0)
    rate_extra = (rate_extra if rate_extra is not None else 1) if rx else 0
    h = bytes([0xFF, 0xF8 | (1 if variable else 0), (bs_code << 4) | rate_code, (acode << 4) | (size_code << 1)])
    h += utf8(number) + blocksize_field(blocksize, bs_code) + (rate_extra.to_bytes(rx, "big") if rx else b"")
    h += bytes([crc8(h)])
    w = BitWriter()
    for byte in h:
        w.put(byte, 8)
    marks = []
    for ch, sub in enumerate(subframes):
        side = (acode == 8 and ch == 1) or (acode == 9 and ch == 0) or (acode == 10 and ch == 1)
        marks.append(write_subframe(w, sub, blocksize, bps + (1 if side else 0), allow_wide))
    w.align()
    body = w.bytes()
    coded = [s.samples for s in subframes]
    if acode == 8:
        chans = [coded[0], [a - d for a, d in zip(*coded)]]
    elif acode == 9:
        chans = [[d + b for d, b in zip(*coded)], coded[1]]
    elif acode == 10:
        left, right = [], []
        for mid, d in zip(*coded):
            mid = (mid << 1) | (d & 1)
            left.append((mid + d) >> 1)
            right.append((mid - d) >> 1)
        chans = [left, right]
    else:
        chans = coded
    return Frame(body + crc16(body).to_bytes(2, "big"), blocksize, chans, marks, len(h))


@dataclass
class Stream:
    data: bytes
    samples: list    # interleaved
    frames: list     # (byte position in data, byte length)
    marks: list      # [frame][subframe] Marks, bits from the first frame's first byte (the decoder's input)
    channels: int
    bits: int
    max_blocksize: int
    total: int
    blocksizes: list

    @property
    def body(self) -> bytes:
        return self.data[42:]


def stream(channels: int, bits: int, frames, sample_rate: int = 44100, variable: bool = False) -> Stream:
    """fLaC, one STREAMINFO block (MD5 zero) and the frames back to back."""
    sizes = [f.blocksize for f in frames]
    if not variable and any(b != sizes[0] for b in sizes[:-1]):
        raise ValueError("fixed blocking needs equal block sizes except for the last frame")
    lo = min(sizes[:-1]) if len(sizes) > 1 else sizes[0]
    if not variable:
        lo = sizes[0]
    lo, hi = max(lo, 16), max(max(sizes), 16)
    lo = min(lo, hi)
    lens = [len(f.data) for f in frames]
    total = sum(sizes)
    v = (lo << 128) | (hi << 112) | (min(lens) << 88) | (max(lens) << 64) | (sample_rate << 44) | \
        ((channels - 1) << 41) | ((bits - 1) << 36) | total
    data = bytearray(b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(18, "big") + bytes(16))
    assert len(data) == 42
    samples, places, marks = [], [], []
    for f in frames:
        assert len(f.channels) == channels
        at = len(data)
        places.append((at, len(f.data)))
        marks.append([m.shifted(8 * (at - 42)) for m in f.marks])
        data += f.data
        for row in zip(*f.channels):
            samples.extend(row)
    return Stream(bytes(data), samples, places, marks, channels, bits, min(hi, 65535), total, sizes)
