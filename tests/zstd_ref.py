"""An independent reader of the Zstandard frame format (RFC 8878) in pure Python, for the tests only.

Written from the RFC: it shares no code with the kernels (dwarfs_amd/csrc/zstd_kernels.hip) or with the host
restatement (dwarfs_amd/csrc/zstd_host.cpp) and imports neither.  It plays the role tests/lz4_ref.py plays for
LZ4.  One frame, no dictionary, the content checksum skipped; what it refuses is what the decode contract at the
top of zstd_host.cpp names.

``frame_info`` parses the frame header, ``count_blocks`` walks the block headers, ``decode`` produces the bytes
and, given a ``collections.Counter``, counts how often each feature of the format is reached (``FEATURES``
lists the keys): the fixture's coverage record.
"""

from __future__ import annotations

from collections import Counter
from typing import List, NamedTuple, Optional, Tuple

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 << 10
MAX_WINDOW_LOG = 31

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                             32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = ([4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4, 6)
OF_DEFAULT = ([1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5, 5)
ML_DEFAULT = ([1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7, 6)
# (name, default distribution, largest accuracy log, largest symbol)
TABLES = (("ll", LL_DEFAULT, 9, 35), ("of", OF_DEFAULT, 8, 31), ("ml", ML_DEFAULT, 9, 52))
MODES = ("predefined", "rle", "fse", "repeat")
LITERAL_TYPES = ("raw", "rle", "compressed", "treeless")

FEATURES = tuple(
    [f"block:{t}" for t in ("raw", "rle", "compressed")] +
    [f"literals:{t}:{sf}" for t in ("raw", "rle") for sf in (0, 1, 3)] +  # (size format 2 is format 0's twin)
    [f"literals:{t}:{sf}" for t in ("compressed", "treeless") for sf in range(4)] +
    ["weights:direct", "weights:fse"] +
    [f"{name}:{m}" for name, *_ in TABLES for m in MODES] +
    [f"seqcount:{k}" for k in ("zero", "1byte", "2byte", "3byte")] +
    [f"rep:{c}:{w}" for c in (1, 2, 3) for w in ("ll", "ll0")] +
    ["offset_beyond_128k", "frame:windowed", "frame:single_segment", "frame:checksum"] +
    [f"fcs_bytes:{n}" for n in (1, 2, 4, 8)])


class ZstdError(ValueError):
    """The frame breaks the format, or does not produce its stated size."""


class FrameInfo(NamedTuple):
    header_bytes: int
    content_size: Optional[int]  # None: the frame does not state it
    window: int
    single_segment: bool
    checksum: bool
    fcs_bytes: int


def frame_info(data: bytes) -> FrameInfo:
    data = bytes(data)
    if len(data) < 5 or int.from_bytes(data[:4], "little") != MAGIC:
        raise ZstdError("no frame magic")
    fhd = data[4]
    fcs_flag, single, reserved, checksum, did_flag = fhd >> 6, bool(fhd & 0x20), fhd & 0x08, bool(fhd & 0x04), fhd & 3
    if reserved:
        raise ZstdError("reserved header bit")
    at = 5
    window = 0
    if not single:
        if at >= len(data):
            raise ZstdError("header cut")
        log = 10 + (data[at] >> 3)
        if log > MAX_WINDOW_LOG:
            raise ZstdError("window too large")
        window = (1 << log) + ((1 << log) >> 3) * (data[at] & 7)
        at += 1
    did_bytes = (0, 1, 2, 4)[did_flag]
    if at + did_bytes > len(data):
        raise ZstdError("header cut")
    if int.from_bytes(data[at:at + did_bytes], "little") != 0:
        raise ZstdError("dictionary needed")
    at += did_bytes
    fcs_bytes = (1 if single else 0, 2, 4, 8)[fcs_flag]
    if at + fcs_bytes > len(data):
        raise ZstdError("header cut")
    content = None
    if fcs_bytes:
        content = int.from_bytes(data[at:at + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
    at += fcs_bytes
    if single:
        window = content
    return FrameInfo(at, content, window, single, checksum, fcs_bytes)


def block_headers(data: bytes) -> List[Tuple[int, int, int, bool]]:
    """[(type, Block_Size, position of the block's content, last)]; ZstdError where a header is cut or a block
    passes the end.  Nothing behind the last block is looked at."""
    data = bytes(data)
    info = frame_info(data)
    at, out = info.header_bytes, []
    while True:
        if at + 3 > len(data):
            raise ZstdError("block header cut")
        h = int.from_bytes(data[at:at + 3], "little")
        last, kind, size = bool(h & 1), h >> 1 & 3, h >> 3
        at += 3
        if kind == 3:
            raise ZstdError("reserved block type")
        held = 1 if kind == 1 else size
        if at + held > len(data):
            raise ZstdError("block cut")
        out.append((kind, size, at, last))
        at += held
        if last:
            return out


def count_blocks(data: bytes) -> int:
    return len(block_headers(data))


class Forward:
    """Bits from the first byte on, lowest bit first (an FSE table description); zeros behind the end."""

    def __init__(self, data: bytes):
        self.data, self.pos = data, 0

    def read(self, n: int) -> int:
        lo = self.pos
        self.pos += n
        chunk = self.data[lo >> 3:(self.pos + 7) >> 3]
        return int.from_bytes(chunk, "little") >> (lo & 7) & ((1 << n) - 1)

    def bytes_used(self) -> int:
        return (self.pos + 7) >> 3


class Backward:
    """Bits from the last byte on, highest first, below the marker bit; ``pos`` is what is left and goes
    negative when more is read than the stream holds (zeros are supplied)."""

    def __init__(self, data: bytes):
        if not data or data[-1] == 0:
            raise ZstdError("bitstream without its end mark")
        self.data = data
        self.pos = 8 * (len(data) - 1) + data[-1].bit_length() - 1

    def peek(self, n: int) -> int:
        lo = self.pos - n
        if lo >= 0:
            chunk = self.data[lo >> 3:(self.pos + 7) >> 3]
            return int.from_bytes(chunk, "little") >> (lo & 7) & ((1 << n) - 1)
        if self.pos <= 0:
            return 0
        return (int.from_bytes(self.data[:(self.pos + 7) >> 3], "little") & ((1 << self.pos) - 1)) << -lo & ((1 << n) - 1)

    def read(self, n: int) -> int:
        v = self.peek(n)
        self.pos -= n
        return v


class FseTable(NamedTuple):
    log: int
    symbol: List[int]
    bits: List[int]
    base: List[int]


def fse_build(freq: List[int], log: int) -> FseTable:
    size = 1 << log
    symbol = [0] * size
    nxt = [0] * len(freq)
    high = size
    for s, f in enumerate(freq):
        if f == -1:
            high -= 1
            symbol[high] = s
            nxt[s] = 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, f in enumerate(freq):
        if f <= 0:
            continue
        nxt[s] = f
        for _ in range(f):
            symbol[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    if pos != 0:
        raise ZstdError("FSE table does not fill")
    bits, base = [0] * size, [0] * size
    for i in range(size):
        d = nxt[symbol[i]]
        nxt[symbol[i]] += 1
        bits[i] = log - (d.bit_length() - 1)
        base[i] = (d << bits[i]) - size
    return FseTable(log, symbol, bits, base)


def fse_read_description(data: bytes, max_log: int, max_symbol: int) -> Tuple[List[int], int, int]:
    """(probabilities, accuracy log, bytes used) of an FSE table description (RFC 8878 4.1.1)."""
    if not data:
        raise ZstdError("FSE description cut")
    r = Forward(data)
    log = 5 + r.read(4)
    if log > max_log:
        raise ZstdError("accuracy log too large")
    remaining, freq = 1 << log, []
    while remaining > 0 and len(freq) <= max_symbol:
        nbits = (remaining + 1).bit_length()
        val = r.read(nbits)
        lower = (1 << (nbits - 1)) - 1
        threshold = (1 << nbits) - 1 - (remaining + 1)
        if (val & lower) < threshold:
            r.pos -= 1
            val &= lower
        elif val > lower:
            val -= threshold
        p = val - 1
        remaining -= abs(p)
        freq.append(p)
        if p == 0:
            while True:
                rep = r.read(2)
                freq += [0] * rep
                if rep != 3:
                    break
    if remaining != 0 or len(freq) > max_symbol + 1:
        raise ZstdError("FSE description does not add up")
    if r.bytes_used() > len(data):
        raise ZstdError("FSE description cut")
    return freq, log, r.bytes_used()


def huffman_weights(data: bytes, stats: Optional[Counter]) -> Tuple[List[int], int]:
    """(weights without the last one, bytes used) of a Huffman tree description (RFC 8878 4.2.1)."""
    if not data:
        raise ZstdError("tree description cut")
    head = data[0]
    if head >= 128:
        n = head - 127
        used = 1 + (n + 1) // 2
        if used > len(data):
            raise ZstdError("tree description cut")
        w = []
        for i in range(n):
            b = data[1 + i // 2]
            w.append(b >> 4 if i % 2 == 0 else b & 15)
        if stats is not None:
            stats["weights:direct"] += 1
        return w, used
    if head == 0 or 1 + head > len(data):
        raise ZstdError("tree description cut")
    body = data[1:1 + head]
    freq, log, used = fse_read_description(body, 6, 12)
    t = fse_build(freq, log)
    if used >= len(body):
        raise ZstdError("no weight bits")
    bs = Backward(body[used:])
    s1 = bs.read(log)
    s2 = bs.read(log)
    w = []
    # two states take turns; the stream ends when the state whose turn it is cannot be refilled
    while True:
        if bs.pos < 0 or len(w) > 255:
            raise ZstdError("weight stream overrun")
        w.append(t.symbol[s1])
        if bs.pos < t.bits[s1]:
            w.append(t.symbol[s2])
            break
        s1 = t.base[s1] + bs.read(t.bits[s1])
        w.append(t.symbol[s2])
        if bs.pos < t.bits[s2]:
            w.append(t.symbol[s1])
            break
        s2 = t.base[s2] + bs.read(t.bits[s2])
    if len(w) > 255:
        raise ZstdError("too many weights")
    if stats is not None:
        stats["weights:fse"] += 1
    return w, 1 + head


class HuffmanTable(NamedTuple):
    log: int
    symbol: List[int]
    bits: List[int]


def huffman_build(weights: List[int]) -> HuffmanTable:
    if any(x > 11 for x in weights):
        raise ZstdError("weight above 11")
    total = sum(1 << (x - 1) for x in weights if x)
    if total == 0:
        raise ZstdError("no weights")
    log = total.bit_length()
    if log > 11:
        raise ZstdError("code length above 11")
    rest = (1 << log) - total
    if rest & (rest - 1):
        raise ZstdError("last weight is no power of two")
    weights = weights + [rest.bit_length()]
    if sum(1 for x in weights if x == 1) < 2 or sum(1 for x in weights if x == 1) % 2:
        raise ZstdError("odd number of longest codes")
    symbol, bits = [], []
    for wt in range(1, log + 1):
        for s, x in enumerate(weights):
            if x == wt:
                symbol += [s] * (1 << (wt - 1))
                bits += [log + 1 - wt] * (1 << (wt - 1))
    assert len(symbol) == 1 << log
    return HuffmanTable(log, symbol, bits)


def huffman_stream(t: HuffmanTable, data: bytes, n: int) -> bytes:
    bs = Backward(data)
    out = bytearray(n)
    sym, bits, log = t.symbol, t.bits, t.log
    for i in range(n):
        e = bs.peek(log)
        out[i] = sym[e]
        bs.pos -= bits[e]
    if bs.pos != 0:
        raise ZstdError("literal stream not used up exactly")
    return bytes(out)


class State:
    """What one block hands to the next."""

    def __init__(self):
        self.huffman: Optional[HuffmanTable] = None
        self.tables: List[Optional[FseTable]] = [None, None, None]
        self.rep = [1, 4, 8]


def literals_section(b: bytes, st: State, stats: Optional[Counter]) -> Tuple[bytes, int, int]:
    """(the literals, bytes of the section, bytes of its header)"""
    if not b:
        raise ZstdError("literals header cut")
    kind, sf = b[0] & 3, b[0] >> 2 & 3
    if kind < 2:
        hl = (1, 2, 1, 3)[sf]
        if len(b) < hl:
            raise ZstdError("literals header cut")
        v = int.from_bytes(b[:hl], "little")
        n = v >> 3 if hl == 1 else v >> 4
        if stats is not None:
            stats[f"literals:{LITERAL_TYPES[kind]}:{0 if sf == 2 else sf}"] += 1
        if n > BLOCK_MAX:
            raise ZstdError("literals above the block maximum")
        if kind == 0:
            if hl + n > len(b):
                raise ZstdError("raw literals cut")
            return b[hl:hl + n], hl + n, hl
        if hl + 1 > len(b):
            raise ZstdError("RLE literal cut")
        return bytes([b[hl]]) * n, hl + 1, hl
    hl = (3, 3, 4, 5)[sf]
    if len(b) < hl:
        raise ZstdError("literals header cut")
    v = int.from_bytes(b[:hl], "little") >> 4
    nb = (10, 10, 14, 18)[sf]
    regen, comp = v & ((1 << nb) - 1), v >> nb & ((1 << nb) - 1)
    streams = 1 if sf == 0 else 4
    if stats is not None:
        stats[f"literals:{LITERAL_TYPES[kind]}:{sf}"] += 1
    if regen > BLOCK_MAX or regen == 0:
        raise ZstdError("literals size out of range")
    if hl + comp > len(b):
        raise ZstdError("compressed literals cut")
    body = b[hl:hl + comp]
    if kind == 2:
        w, used = huffman_weights(body, stats)
        st.huffman = huffman_build(w)
        body = body[used:]
    elif st.huffman is None:
        raise ZstdError("treeless literals without a tree")
    t = st.huffman
    if streams == 1:
        if not body:
            raise ZstdError("no literal stream")
        return huffman_stream(t, body, regen), hl + comp, hl
    if len(body) < 10:
        raise ZstdError("four streams need 10 bytes")
    sizes = [int.from_bytes(body[2 * i:2 * i + 2], "little") for i in range(3)]
    if 6 + sum(sizes) >= len(body):
        raise ZstdError("jump table past the section")
    sizes.append(len(body) - 6 - sum(sizes))
    seg = (regen + 3) // 4
    if 3 * seg > regen:
        raise ZstdError("fewer literals than three segments")
    out, at = b"", 6
    for i, s in enumerate(sizes):
        if s == 0:
            raise ZstdError("empty literal stream")
        out += huffman_stream(t, body[at:at + s], seg if i < 3 else regen - 3 * seg)
        at += s
    return out, hl + comp, hl


def sequences_header_bytes(b: bytes) -> int:
    """Bytes of the sequence count and, where there are sequences, the modes byte."""
    return 1 if b[0] == 0 else (2 if b[0] < 128 else 3 if b[0] < 255 else 4)


def sequences_section(b: bytes, st: State, stats: Optional[Counter]) -> List[Tuple[int, int, int]]:
    """[(literal length, match length, offset value)]"""
    if not b:
        raise ZstdError("sequences header cut")
    if b[0] == 0:
        if len(b) != 1:
            raise ZstdError("bytes behind an empty sequences section")
        if stats is not None:
            stats["seqcount:zero"] += 1
        return []
    if b[0] < 128:
        n, at, key = b[0], 1, "1byte"
    elif b[0] < 255:
        if len(b) < 2:
            raise ZstdError("sequences header cut")
        n, at, key = ((b[0] - 128) << 8) + b[1], 2, "2byte"
        if n == 0:
            raise ZstdError("a count of 0 in two bytes")
    else:
        if len(b) < 3:
            raise ZstdError("sequences header cut")
        n, at, key = b[1] + (b[2] << 8) + 0x7F00, 3, "3byte"
    if stats is not None:
        stats[f"seqcount:{key}"] += 1
    if at >= len(b):
        raise ZstdError("no compression modes")
    modes = b[at]
    at += 1
    if modes & 3:
        raise ZstdError("reserved mode bits")
    for k, (name, default, max_log, max_symbol) in enumerate(TABLES):
        mode = modes >> (6 - 2 * k) & 3
        if stats is not None:
            stats[f"{name}:{MODES[mode]}"] += 1
        if mode == 0:
            st.tables[k] = fse_build(*default)
        elif mode == 1:
            if at >= len(b):
                raise ZstdError("RLE symbol cut")
            if b[at] > max_symbol:
                raise ZstdError("RLE symbol out of range")
            st.tables[k] = FseTable(0, [b[at]], [0], [0])
            at += 1
        elif mode == 2:
            freq, log, used = fse_read_description(b[at:], max_log, max_symbol)
            st.tables[k] = fse_build(freq, log)
            at += used
        elif st.tables[k] is None:
            raise ZstdError("repeat mode without a table")
    if at >= len(b):
        raise ZstdError("no sequence bits")
    bs = Backward(b[at:])
    ll_t, of_t, ml_t = st.tables
    ll_s, of_s, ml_s = bs.read(ll_t.log), bs.read(of_t.log), bs.read(ml_t.log)
    out = []
    for i in range(n):
        of_code, ml_code, ll_code = of_t.symbol[of_s], ml_t.symbol[ml_s], ll_t.symbol[ll_s]
        offset_value = (1 << of_code) + bs.read(of_code)
        ml = ML_BASE[ml_code] + bs.read(ML_BITS[ml_code])
        ll = LL_BASE[ll_code] + bs.read(LL_BITS[ll_code])
        out.append((ll, ml, offset_value))
        if i + 1 < n:
            ll_s = ll_t.base[ll_s] + bs.read(ll_t.bits[ll_s])
            ml_s = ml_t.base[ml_s] + bs.read(ml_t.bits[ml_s])
            of_s = of_t.base[of_s] + bs.read(of_t.bits[of_s])
        if bs.pos < 0:
            raise ZstdError("sequence bits overrun")
    if bs.pos != 0:
        raise ZstdError("sequence bits left over")
    return out


def resolve_offset(rep: List[int], ll: int, offset_value: int, stats: Optional[Counter]) -> int:
    """The match offset of a sequence; updates the repeat-offset history (RFC 8878 3.1.1.5)."""
    if offset_value > 3:
        off = offset_value - 3
        rep[:] = [off, rep[0], rep[1]]
        return off
    if stats is not None:
        stats[f"rep:{offset_value}:{'ll0' if ll == 0 else 'll'}"] += 1
    idx = offset_value + (1 if ll == 0 else 0)
    if idx == 1:
        return rep[0]
    off = rep[0] - 1 if idx == 4 else rep[idx - 1]
    if off == 0:
        raise ZstdError("offset 0 through the repeat rule")
    if idx == 2:
        rep[:] = [off, rep[0], rep[2]]
    else:
        rep[:] = [off, rep[0], rep[1]]
    return off


def decode(data: bytes, stats: Optional[Counter] = None, size: Optional[int] = None,
           trace: Optional[dict] = None) -> bytes:
    """The bytes of the one frame that ``data`` is; ZstdError if it is malformed, is followed by anything, or
    does not produce exactly its content size (``size``, where the caller states it: then the frame may lack
    the field, and must agree where it has it).  ``trace`` receives "spots", the positions of every header
    byte (frame, block, literals, sequences), and "spans", (frame position, output position, length) of the
    bytes that the frame holds as they are: Raw blocks and raw literal runs."""
    data = bytes(data)
    info = frame_info(data)
    if size is not None:
        if info.content_size not in (None, size):
            raise ZstdError("content size is not the stated size")
        info = info._replace(content_size=size, window=size if info.single_segment else info.window)
    if info.content_size is None:
        raise ZstdError("no content size")
    spots, spans = set(range(info.header_bytes)), []
    if trace is not None:
        trace.update(spots=spots, spans=spans)
    if stats is not None:
        stats["frame:single_segment" if info.single_segment else "frame:windowed"] += 1
        stats[f"fcs_bytes:{info.fcs_bytes}"] += 1
        if info.checksum:
            stats["frame:checksum"] += 1
    block_max = min(info.window, BLOCK_MAX)
    st = State()
    out = bytearray()
    blocks = block_headers(data)
    for kind, size, at, last in blocks:
        start = len(out)
        spots.update(range(at - 3, at))
        if kind == 0:
            spans.append((at, start, size))
            out += data[at:at + size]
        elif kind == 1:
            out += data[at:at + 1] * size
        else:
            if size < 3 or size > block_max:
                raise ZstdError("compressed block size out of range")
            body = data[at:at + size]
            lits, used, hl = literals_section(body, st, stats)
            spots.update(range(at, at + hl))
            if used >= len(body):
                raise ZstdError("sequences header cut")
            spots.update(range(at + used, at + min(used + sequences_header_bytes(body[used:]), size)))
            lit_at, raw = 0, body[0] & 3 == 0
            for ll, ml, ov in sequences_section(body[used:], st, stats):
                if lit_at + ll > len(lits):
                    raise ZstdError("literals run out")
                if raw:
                    spans.append((at + hl + lit_at, len(out), ll))
                out += lits[lit_at:lit_at + ll]
                lit_at += ll
                off = resolve_offset(st.rep, ll, ov, stats)
                if off > len(out) or off > info.window:
                    raise ZstdError("offset before the start of the output or beyond the window")
                if stats is not None and off > BLOCK_MAX:
                    stats["offset_beyond_128k"] += 1
                if len(out) - start + ml > block_max:
                    raise ZstdError("block above the block maximum")
                if off >= ml:
                    out += out[len(out) - off:len(out) - off + ml]
                else:
                    pattern = bytes(out[len(out) - off:])
                    out += (pattern * (ml // off + 1))[:ml]
            if raw:
                spans.append((at + hl + lit_at, len(out), len(lits) - lit_at))
            out += lits[lit_at:]
        if stats is not None:
            stats[f"block:{('raw', 'rle', 'compressed')[kind]}"] += 1
        if len(out) - start > block_max or len(out) > info.content_size:
            raise ZstdError("block above the block maximum or the content size")
    kind, size, at, _ = blocks[-1]
    end = at + (1 if kind == 1 else size) + (4 if info.checksum else 0)
    if end != len(data):
        raise ZstdError("checksum missing, or bytes behind the frame")
    if len(out) != info.content_size:
        raise ZstdError(f"the frame produced {len(out)} bytes, not {info.content_size}")
    return bytes(out)
