"""An independent RFC 9639 (FLAC) reader in pure Python, for the tests only.

Written from the RFC alone: it shares no code with the GPU codec
(dwarfs_amd/csrc/flac_kernels.hip) or with the CPU restatement
(oracle/flac_oracle.c), and imports neither.  Python's unbounded ints carry
every intermediate value, so 32-bit samples and their 33-bit side channel
raise no overflow question.  ``decode`` is meant for inputs of a few thousand
samples; for larger streams use ``walk_frames`` (which still parses every
subframe to find where each frame ends, but keeps no samples).
"""

from __future__ import annotations

from typing import NamedTuple


class FlacError(ValueError):
    """The stream breaks a rule of RFC 9639."""


def crc8(data: bytes, crc: int = 0) -> int:
    """CRC-8, polynomial x^8 + x^2 + x + 1 (0x07), MSB first, initial value 0 (RFC 9639 section 9.1.8)."""
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def crc16(data: bytes, crc: int = 0) -> int:
    """CRC-16, polynomial x^16 + x^15 + x^2 + 1 (0x8005), MSB first, initial value 0 (section 9.3)."""
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x8005) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def _table(step, top, mask):
    t = []
    for v in range(256):
        c = v << (top - 7)
        for _ in range(8):
            c = ((c << 1) ^ step) & mask if c & (1 << top) else (c << 1) & mask
        t.append(c)
    return t


_T16 = _table(0x8005, 15, 0xFFFF)


def crc16_fast(data: bytes, crc: int = 0) -> int:
    """crc16 by a byte table (the tests compare the two)."""
    t = _T16
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ t[(crc >> 8) ^ b]
    return crc


class StreamInfo(NamedTuple):
    min_blocksize: int
    max_blocksize: int
    min_framesize: int
    max_framesize: int
    sample_rate: int
    channels: int
    bits: int
    total_samples: int
    md5: bytes
    frames_at: int  # byte offset of the first frame
    blocks: tuple   # (type, length) of every metadata block, in order


def parse_streaminfo(stream: bytes) -> StreamInfo:
    """STREAMINFO's fields and the offset of the first frame; every other metadata block is skipped by its
    length (section 8)."""
    if stream[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    at, first, info, blocks = 4, True, None, []
    while True:
        if at + 4 > len(stream):
            raise FlacError("metadata truncated")
        last, kind = stream[at] >> 7, stream[at] & 0x7F
        length = int.from_bytes(stream[at + 1:at + 4], "big")
        at += 4
        if kind == 127:
            raise FlacError("metadata block type 127 is forbidden")
        if at + length > len(stream):
            raise FlacError("metadata block runs past the stream")
        if first:
            if kind != 0 or length != 34:
                raise FlacError("the first metadata block is not a 34-byte STREAMINFO")
            v = int.from_bytes(stream[at:at + 18], "big")  # 144 bits
            info = (v >> 128, (v >> 112) & 0xFFFF, (v >> 88) & 0xFFFFFF, (v >> 64) & 0xFFFFFF, (v >> 44) & 0xFFFFF,
                    ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1), bytes(stream[at + 18:at + 34]))
            first = False
        elif kind == 0:
            raise FlacError("a second STREAMINFO")
        blocks.append((kind, length))
        at += length
        if last:
            break
    if info[0] < 16 or info[1] < 16 or info[0] > info[1]:
        raise FlacError(f"STREAMINFO block sizes {info[0]}..{info[1]}")
    if info[6] < 4:
        raise FlacError("STREAMINFO bit depth below 4")
    return StreamInfo(*info, at, tuple(blocks))


class Header(NamedTuple):
    length: int      # bytes, CRC-8 included
    variable: int    # blocking strategy bit
    coded: int       # frame number (fixed blocking) or first sample (variable)
    blocksize: int
    bs_code: int
    rate_code: int
    assignment: int  # channel bits: 0-7 independent (n + 1 channels), 8 left/side, 9 side/right, 10 mid/side
    size_code: int   # sample-size bits
    crc8: int        # as stored
    crc8_ok: bool


_SIZES = (0, 8, 12, None, 16, 20, 24, 32)


def parse_header(data: bytes, p: int) -> Header:
    """The frame header at byte p (section 9.1); raises FlacError on a reserved bit, an invalid code or
    truncation.  The CRC-8 is reported, not enforced."""
    n = len(data)
    if p + 5 > n:
        raise FlacError("frame header truncated")
    if data[p] != 0xFF or (data[p + 1] & 0xFC) != 0xF8:
        raise FlacError(f"no frame sync code at byte {p}")
    if data[p + 1] & 2:
        raise FlacError("reserved bit after the sync code is set")
    variable = data[p + 1] & 1
    bc, rc = data[p + 2] >> 4, data[p + 2] & 15
    assign, sc = data[p + 3] >> 4, (data[p + 3] >> 1) & 7
    if data[p + 3] & 1:
        raise FlacError("reserved bit after the sample size is set")
    if bc == 0:
        raise FlacError("block size code 0 is reserved")
    if rc == 15:
        raise FlacError("sample rate code 15 is invalid")
    if assign > 10:
        raise FlacError(f"channel assignment {assign} is reserved")
    if sc == 3:
        raise FlacError("sample size code 3 is reserved")
    q = p + 4
    b0 = data[q]
    q += 1
    if b0 < 0x80:
        more, num = 0, b0
    else:
        more = 8 - (b0 ^ 0xFF).bit_length() - 1  # leading ones - 1
        if more < 1 or more > 6:
            raise FlacError(f"coded number starts with {b0:#x}")
        num = b0 & (0x7F >> (more + 1))
        if q + more > n:
            raise FlacError("coded number truncated")
        for _ in range(more):
            if (data[q] & 0xC0) != 0x80:
                raise FlacError("coded number continuation byte")
            num = (num << 6) | (data[q] & 0x3F)
            q += 1
    if not variable and num >> 31:
        raise FlacError("frame number above 31 bits")
    extra = (1 if bc == 6 else 2 if bc == 7 else 0) + (1 if rc == 12 else 2 if rc in (13, 14) else 0)
    if q + extra + 1 > n:
        raise FlacError("frame header truncated")
    if bc == 1:
        bs = 192
    elif bc <= 5:
        bs = 576 << (bc - 2)
    elif bc == 6:
        bs = data[q] + 1
        q += 1
    elif bc == 7:
        bs = ((data[q] << 8) | data[q + 1]) + 1
        q += 2
    else:
        bs = 256 << (bc - 8)
    q += 1 if rc == 12 else 2 if rc in (13, 14) else 0
    c = crc8(data[p:q])
    return Header(q + 1 - p, variable, num, bs, bc, rc, assign, sc, data[q], c == data[q])


def header_candidates(body: bytes, channels: int, bits: int, max_blocksize: int = 65536) -> list:
    """The byte positions of ``body`` (the frames, without metadata) at which a frame header of a ``channels`` x
    ``bits`` stream parses with a valid CRC-8 and a block size of at most ``max_blocksize``: what a decoder that
    looks for frames at every byte at once has to tell apart.  Like such a scan it wants room for the longest
    header after the coded number (block size, sample rate: 4 bytes) and takes a sample-size code that is 0 or
    names ``bits``."""
    body = bytes(body)
    n, found, p = len(body), [], body.find(b"\xff")
    while p >= 0:
        if p + 6 <= n and (body[p + 1] & 0xFE) == 0xF8:
            try:
                h = parse_header(body, p)
            except (FlacError, IndexError):
                h = None
            if h is not None and h.crc8_ok:
                more = 0 if body[p + 4] < 0x80 else 8 - (body[p + 4] ^ 0xFF).bit_length() - 1
                room = p + 5 + more + 4 <= n
                size_ok = h.size_code == 0 or _SIZES[h.size_code] == bits
                chans = h.assignment + 1 if h.assignment < 8 else 2
                if room and size_ok and chans == channels and h.blocksize <= max_blocksize:
                    found.append(p)
        p = body.find(b"\xff", p + 1)
    return found


def count_header_candidates(body: bytes, channels: int, bits: int, max_blocksize: int = 65536) -> int:
    """len(header_candidates(...))."""
    return len(header_candidates(body, channels, bits, max_blocksize))


class _Bits:
    """MSB-first bit reader over bytes; reading past the end raises."""

    def __init__(self, data: bytes, byte_pos: int):
        self.d, self.p, self.acc, self.n = data, byte_pos, 0, 0

    def _refill(self):
        chunk = self.d[self.p:self.p + 32]
        if not chunk:
            raise FlacError("frame truncated")
        self.acc = (self.acc << (8 * len(chunk))) | int.from_bytes(chunk, "big")
        self.n += 8 * len(chunk)
        self.p += len(chunk)

    def read(self, k: int) -> int:
        while self.n < k:
            self._refill()
        self.n -= k
        v = self.acc >> self.n
        self.acc &= (1 << self.n) - 1
        return v

    def signed(self, k: int) -> int:
        if k == 0:
            return 0
        v = self.read(k)
        return v - (1 << k) if v >> (k - 1) else v

    def unary(self) -> int:
        """The number of 0 bits before the next 1 bit, which is consumed."""
        q = 0
        while not self.acc:
            q += self.n
            self.n = 0
            self._refill()
        z = self.n - self.acc.bit_length()
        self.n -= z + 1
        self.acc &= (1 << self.n) - 1
        return q + z

    def bit_pos(self) -> int:
        return 8 * self.p - self.n

    def skip(self, bits: int):
        while bits > self.n:
            bits -= self.n
            self.n = self.acc = 0
            self._refill()
        self.n -= bits
        self.acc &= (1 << self.n) - 1

    def align(self):
        pad = self.n & 7
        if self.read(pad):
            raise FlacError("non-zero padding bits before the CRC-16")


_RES_MIN = -(1 << 31)  # excluded by section 9.2.7.3: "a 32-bit signed integer, excluding the most negative value"


def _residual(r: _Bits, bs: int, order: int, keep: bool, plan: dict | None = None):
    """The residual section (section 9.2.7): bs - order values, or None when not kept.  A residual of -2^31,
    Rice coded or in an escaped partition, is refused whether the values are kept or not (section 9.2.7.3)."""
    method = r.read(2)
    if method > 1:
        raise FlacError("residual coding method is reserved")
    pbits = 5 if method else 4
    po = r.read(4)
    if bs % (1 << po) or (bs >> po) < order:
        raise FlacError(f"partition order {po} does not fit block size {bs}, predictor order {order}")
    out = [] if keep else None
    params = []
    for part in range(1 << po):
        count = (bs >> po) - (order if part == 0 else 0)
        k = r.read(pbits)
        if k == (1 << pbits) - 1:  # escape: raw signed values
            w = r.read(5)
            params.append(("esc", w))
            if keep:
                vals = [r.signed(w) for _ in range(count)]
                if _RES_MIN in vals:  # (out of reach of the 5-bit width field, at most 31 bits; kept for the rule)
                    raise FlacError("an escaped residual of -2^31 (section 9.2.7.3)")
                out.extend(vals)
            else:
                r.skip(w * count)
        else:
            params.append(k)
            unary, read = r.unary, r.read
            worst = 0xFFFFFFFF  # the folded -2^31
            if keep:
                for _ in range(count):
                    u = (unary() << k) | read(k)
                    if u == worst:
                        raise FlacError("a residual of -2^31 (section 9.2.7.3)")
                    out.append(-(u >> 1) - 1 if u & 1 else u >> 1)
            else:
                for _ in range(count):
                    if (unary() << k) | read(k) == worst:
                        raise FlacError("a residual of -2^31 (section 9.2.7.3)")
    if plan is not None:
        plan.update(partition_order=po, method=method, params=tuple(params))
    return out


_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


class SubframePlan(NamedTuple):
    """What a subframe's fields say about how it was coded (walk_plans)."""
    kind: str             # "constant", "verbatim", "fixed", "lpc"
    order: int
    wasted: int
    partition_order: int  # fixed and lpc; else 0
    method: int           # 0: 4-bit Rice parameters, 1: 5-bit
    params: tuple         # per partition the Rice parameter k, or ("esc", width)
    precision: int        # lpc; else 0
    shift: int
    coefs: tuple          # lpc: newest sample first
    bits: int             # the subframe's length in the stream


def _subframe(r: _Bits, bs: int, bits: int, keep: bool, plans: list | None = None):
    """One subframe of ``bits``-bit samples (section 9.2)."""
    start = r.bit_pos()
    plan = {} if plans is not None else None
    if r.read(1):
        raise FlacError("subframe padding bit is set")
    kind = r.read(6)
    wasted = r.unary() + 1 if r.read(1) else 0
    if wasted >= bits:
        raise FlacError("wasted bits leave no sample bits")
    b = bits - wasted
    if kind == 0:
        v = r.signed(b)
        out = [v] * bs if keep else None
    elif kind == 1:
        if keep:
            out = [r.signed(b) for _ in range(bs)]
        else:
            r.skip(b * bs)
            out = None
    elif 8 <= kind <= 12 or kind >= 32:
        order = kind - 8 if kind < 32 else kind - 31
        if order > bs:
            raise FlacError("predictor order above the block size")
        warm = [r.signed(b) for _ in range(order)]
        if kind >= 32:
            prec = r.read(4) + 1
            if prec == 16:
                raise FlacError("LPC precision code 15 is invalid")
            shift = r.signed(5)
            if shift < 0:
                raise FlacError("negative LPC shift")
            coef = [r.signed(prec) for _ in range(order)]
        else:
            shift, coef = 0, _FIXED[order]
        res = _residual(r, bs, order, keep, plan)
        if plan is not None:
            plan.update(order=order)
            if kind >= 32:
                plan.update(precision=prec, shift=shift, coefs=tuple(coef))
        out = None
        if keep:
            out = warm
            if order == 0:
                out = res
            else:
                rc = tuple(reversed(coef))  # oldest sample first
                for i, e in enumerate(res):
                    acc = 0
                    for c, s in zip(rc, out[i:i + order]):
                        acc += c * s
                    out.append(e + (acc >> shift))
    else:
        raise FlacError(f"subframe type {kind} is reserved")
    if plans is not None:
        name = "constant" if kind == 0 else "verbatim" if kind == 1 else "fixed" if kind < 32 else "lpc"
        plans.append(SubframePlan(name, plan.get("order", 0), wasted, plan.get("partition_order", 0),
                                  plan.get("method", 0), plan.get("params", ()), plan.get("precision", 0),
                                  plan.get("shift", 0), plan.get("coefs", ()), r.bit_pos() - start))
    if keep:
        lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        if any(v < lo or v > hi for v in out):
            raise FlacError(f"a sample does not fit {b} bits")
        if wasted:
            out = [v << wasted for v in out]
    return out


class Frame(NamedTuple):
    pos: int         # byte offset in the stream
    length: int      # bytes, CRC-16 included
    coded: int
    blocksize: int
    assignment: int
    size_code: int
    variable: int
    crc8_ok: bool
    crc16_ok: bool
    first_sample: int
    samples: object  # per-channel lists after stereo reconstruction (decode), else None


def frame_at(data: bytes, pos: int, channels: int, bits: int, keep: bool = False, first_sample: int = 0,
             plans: list | None = None) -> Frame:
    """The frame at byte ``pos`` of a ``channels`` x ``bits`` stream, whatever its number: header, subframes,
    padding, CRC-16.  Raises FlacError where it does not parse; CRC mismatches are reported in the result.
    ``plans``: a list that receives one SubframePlan per subframe, in stream order."""
    h = parse_header(data, pos)
    if h.size_code and _SIZES[h.size_code] != bits:
        raise FlacError(f"frame sample size {_SIZES[h.size_code]} but STREAMINFO says {bits}")
    chans = h.assignment + 1 if h.assignment < 8 else 2
    if chans != channels:
        raise FlacError(f"frame has {chans} channels but STREAMINFO says {channels}")
    r = _Bits(data, pos + h.length)
    subs = []
    for ch in range(chans):
        side = (h.assignment == 8 and ch == 1) or (h.assignment == 9 and ch == 0) or (h.assignment == 10 and ch == 1)
        subs.append(_subframe(r, h.blocksize, bits + (1 if side else 0), keep, plans))
    r.align()
    end = r.bit_pos() >> 3
    if end + 2 > len(data):
        raise FlacError("frame truncated before its CRC-16")
    ok16 = crc16_fast(data[pos:end]) == (data[end] << 8) | data[end + 1]
    if keep:
        if h.assignment == 8:
            subs[1] = [a - s for a, s in zip(subs[0], subs[1])]
        elif h.assignment == 9:
            subs[0] = [s + b for s, b in zip(subs[0], subs[1])]
        elif h.assignment == 10:
            left, right = [], []
            for m, s in zip(subs[0], subs[1]):
                m = (m << 1) | (s & 1)
                left.append((m + s) >> 1)
                right.append((m - s) >> 1)
            subs = [left, right]
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        if any(v < lo or v > hi for c in subs for v in c):
            raise FlacError(f"a sample does not fit {bits} bits")
    return Frame(pos, end + 2 - pos, h.coded, h.blocksize, h.assignment, h.size_code, h.variable, h.crc8_ok, ok16,
                 first_sample, subs if keep else None)


def _frames(stream: bytes, info: StreamInfo, keep: bool, plans: list | None = None):
    stream = bytes(stream)
    pos, done, frames, variable = info.frames_at, 0, [], None
    total = info.total_samples
    while (done < total) if total else (pos < len(stream)):
        if pos >= len(stream):
            raise FlacError(f"stream ends after {done} of {total} samples")
        sub_plans = [] if plans is not None else None
        f = frame_at(stream, pos, info.channels, info.bits, keep, done, sub_plans)
        if plans is not None:
            plans.append(sub_plans)
        if variable is None:
            variable = f.variable
        elif variable != f.variable:
            raise FlacError("blocking strategy changes inside the stream")
        if variable:
            if f.coded != done:
                raise FlacError(f"frame {len(frames)} starts at sample {f.coded}, expected {done}")
        elif f.coded != len(frames):
            raise FlacError(f"frame number {f.coded}, expected {len(frames)}")
        if f.blocksize > info.max_blocksize:
            raise FlacError(f"block size {f.blocksize} above the STREAMINFO maximum {info.max_blocksize}")
        if total and done + f.blocksize > total:
            raise FlacError("frames hold more samples than STREAMINFO's total")
        frames.append(f)
        done += f.blocksize
        pos += f.length
    # every frame but the last holds at least the minimum block size (section 8.2)
    for f in frames[:-1]:
        if f.blocksize < info.min_blocksize:
            raise FlacError(f"block size {f.blocksize} below the STREAMINFO minimum before the last frame")
    return frames


def walk_frames(stream: bytes, info: StreamInfo | None = None) -> list:
    """Every frame in order from the first (samples not kept).  Raises FlacError on a set reserved bit, an
    invalid code, a sample size or channel count that disagrees with STREAMINFO, frame numbers that are not
    consecutive (sample numbers that do not continue, with variable blocking), a block size above the
    STREAMINFO maximum, or below the minimum on any frame but the last.  CRC mismatches are reported in the
    frames (crc8_ok, crc16_ok), not raised."""
    return _frames(stream, info or parse_streaminfo(stream), False)


def walk_plans(stream: bytes, info: StreamInfo | None = None) -> tuple:
    """(frames, plans): walk_frames' result and, per frame, one SubframePlan per subframe in stream order (for a
    stereo assignment: the two coded channels, as the assignment names them)."""
    plans = []
    return _frames(stream, info or parse_streaminfo(stream), False, plans), plans


def decode(stream: bytes) -> list:
    """The stream's samples, interleaved, as Python ints; raises FlacError as walk_frames does, and on a CRC
    mismatch."""
    info = parse_streaminfo(stream)
    out = []
    for f in _frames(stream, info, True):
        if not (f.crc8_ok and f.crc16_ok):
            raise FlacError(f"CRC mismatch in the frame at byte {f.pos}")
        for row in zip(*f.samples):
            out.extend(row)
    return out


def pcm_le(samples, bits: int) -> bytes:
    """The bytes FLAC's MD5 is taken over: each interleaved sample as a signed little-endian integer of
    ceil(bits / 8) bytes (section 8.2)."""
    nb = (bits + 7) // 8
    return b"".join(int(v).to_bytes(nb, "little", signed=True) for v in samples)
