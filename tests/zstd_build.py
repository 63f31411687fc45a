"""A writer of Zstandard frames field by field (RFC 8878), and the constructed-frame families of the zstd tests.

Pure Python, for the tests only: no GPU, no libzstd, nothing from the package.  It takes table construction
from tests/zstd_ref.py (``fse_build``, ``huffman_build``, the base and bits lists), the independent reader that
is the reference here; the FSE encoder inverts the decode table: for the state the decoder must land in there
is one cell with the wanted symbol whose ``[base, base + 2^bits)`` holds it.

:class:`Frame` collects blocks (``raw``, ``rle``, ``compressed``) and writes the frame with any header the
format allows.  While it collects, a plain executor of the sequence lists (``Frame._run``: literals, the
repeat-offset rules of 3.1.1.5, byte-wise match copy) keeps the expected output; it is written separately from
``zstd_ref.decode`` and shares nothing with it.  ``Frame.case`` makes the :class:`Case` record.

The families (``FAMILIES``) return lists of :class:`Case`.  Their docstrings name the lines of
dwarfs_amd/csrc/zstd_kernels.hip they aim at; the ``W`` of ``watermark`` restates that kernel's store
watermark, to aim the cases, never to compute an expected byte.
"""

from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

from zstd_ref import (LL_BASE, LL_BITS, LL_DEFAULT, ML_BASE, ML_BITS, ML_DEFAULT, OF_DEFAULT, FseTable, fse_build,
                      huffman_build)

FILL = 0xA5  # what the tests fill output buffers with: the watermark family's literals avoid it
MAGIC = bytes.fromhex("28b52ffd")
KIB = 1024
BLOCK_MAX = 128 * KIB
DEFAULTS = (LL_DEFAULT, OF_DEFAULT, ML_DEFAULT)
MAX_LOG = (9, 8, 9)
Seq = Tuple[int, int, int]  # (literal length, match length, offset value: offset + 3, or a repeat code 1..3)


class Case(NamedTuple):
    what: str    # the parameters, for the assertion message
    frame: bytes
    out_n: int   # the output size the decoder is offered
    ok: bool     # the decode contract at the top of zstd_host.cpp accepts the frame at this size
    want: bytes  # ok: all out_n bytes; else what the blocks before the failing one produce (the output's start)
    blocks: int  # block headers in the frame; 1 where they cannot be walked, which is what a caller promises then


class BuildError(AssertionError):
    """The caller asked for something the format cannot say."""


def lits(n: int, salt: int = 0, avoid: Optional[int] = None, below: int = 256) -> bytes:
    """n bytes, any 256 in a row from the start all distinct (131 is odd), differing with ``salt``; with
    ``below`` only symbols under it (a power of two)."""
    out = bytearray((salt * 29 + 1 + i * 131 + (i >> 8) * 7) & (below - 1) for i in range(n))
    if avoid is not None:
        out = out.replace(bytes([avoid]), bytes([avoid ^ 0xFF]))
    return bytes(out)


class Lcg:
    """A small deterministic generator."""

    def __init__(self, seed: int):
        self.x = (seed * 2654435761 + 12345) & 0xFFFFFFFF

    def below(self, n: int) -> int:
        self.x = (self.x * 1103515245 + 12345) & 0xFFFFFFFF
        return (self.x >> 16) % n


# ---------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------
class Forward:
    """Bits from the first byte on, lowest bit first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v: int, n: int):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc |= v << self.n
        self.n += n

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) >> 3, "little")


def backward(reads: Sequence[Tuple[int, int]]) -> bytes:
    """A backward bitstream from (value, bits) in the order the decoder reads them: the end mark is the highest
    bit of the last byte, the value read last ends in bit 0 of the first byte."""
    text = ["1"]
    for v, n in reads:
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        if n:
            text.append(format(v, f"0{n}b"))
    text = "".join(text)
    return int(text, 2).to_bytes((len(text) + 7) >> 3, "little")


# ---------------------------------------------------------------------------
# FSE
# ---------------------------------------------------------------------------
def fse_description(norm: Sequence[int], log: int) -> Tuple[bytes, int]:
    """(bytes, bits used) of the table description of a normalised distribution (4.1.1): the one-bit-shorter
    small values, -1 for "less than 1", and behind a 0 the two-bit repeat flags (3 means three more zeros and
    another flag)."""
    if sum(abs(p) for p in norm) != 1 << log or any(p < -1 for p in norm):
        raise BuildError("the probabilities do not add up to the table size")
    b = Forward()
    b.put(log - 5, 4)
    remaining, i = 1 << log, 0
    while remaining > 0:
        p = norm[i]
        i += 1
        v = p + 1
        nbits = (remaining + 1).bit_length()
        lower, threshold = (1 << (nbits - 1)) - 1, (1 << nbits) - 1 - (remaining + 1)
        if v < threshold:
            b.put(v, nbits - 1)
        elif v <= lower:
            b.put(v, nbits)
        else:
            b.put(v + threshold, nbits)
        remaining -= abs(p)
        if p == 0:
            z = 0
            while i < len(norm) and norm[i] == 0:
                z, i = z + 1, i + 1
            while z >= 3:
                b.put(3, 2)
                z -= 3
            b.put(z, 2)
    if any(norm[i:]):
        raise BuildError("probabilities behind the full table")
    return b.bytes(), b.n


def normalise(counts: Dict[int, int], log: int, favour: Optional[int] = None) -> List[int]:
    """A distribution of table size 2^log in which every counted symbol has at least 1: shares by count, what
    is left to ``favour`` (default: the most frequent)."""
    syms, size = sorted(counts), 1 << log
    if not 2 <= len(syms) <= size:
        raise BuildError("an FSE table takes 2 symbols at least, and at most its size")
    norm = [0] * (syms[-1] + 1)
    total, rest = sum(counts.values()), size - len(syms)
    for s in syms:
        norm[s] = 1 + counts[s] * rest // total
    norm[max(syms, key=lambda s: counts[s]) if favour is None else favour] += size - sum(norm)
    return norm


def fse_states(t: FseTable, codes: Sequence[int], last=0) -> List[int]:
    """The states the decoder passes through to read ``codes`` from table ``t``, found from the last one back;
    ``last`` picks the last state among the cells of the last code (an index, or a function of (table, cells))."""
    cells: Dict[int, List[int]] = {}
    for i, s in enumerate(t.symbol):
        cells.setdefault(s, []).append(i)
    for c in codes:
        if c not in cells:
            raise BuildError(f"code {c} is not in the table")
    st = [0] * len(codes)
    own = cells[codes[-1]]
    st[-1] = last(t, own) if callable(last) else own[last % len(own)]
    for i in range(len(codes) - 2, -1, -1):
        nxt = st[i + 1]
        st[i] = next(c for c in cells[codes[i]] if t.base[c] <= nxt < t.base[c] + (1 << t.bits[c]))
    return st


def widest(t: FseTable, cells: List[int]) -> int:
    """The cell whose state update reads the most bits."""
    return max(cells, key=lambda c: t.bits[c])


def code_of(value: int, base: Sequence[int]) -> int:
    return max(i for i, b in enumerate(base) if b <= value)


def seq_codes(q: Seq) -> Tuple[int, int, int]:
    ll, ml, ov = q
    if ll > 131071 or not 3 <= ml <= 131074 or ov < 1:
        raise BuildError(f"no code for {q}")
    return code_of(ll, LL_BASE), ov.bit_length() - 1, code_of(ml, ML_BASE)


# ---------------------------------------------------------------------------
# Huffman
# ---------------------------------------------------------------------------
def weights_of_lengths(lengths: Dict[int, int]) -> List[int]:
    """The weights (the last symbol's included) of a complete prefix code given as {symbol: bits}."""
    log = max(lengths.values())
    if sum(1 << (log - n) for n in lengths.values()) != 1 << log:
        raise BuildError("the code is not complete")
    return [log + 1 - lengths[s] if s in lengths else 0 for s in range(max(lengths) + 1)]


def balanced_weights(symbols: Sequence[int]) -> List[int]:
    """A complete code over the symbols, all lengths k - 1 or k."""
    syms = sorted(set(symbols))
    n = len(syms)
    k = max((n - 1).bit_length(), 1)
    short = (1 << k) - n
    return weights_of_lengths({s: k - 1 if i < short else k for i, s in enumerate(syms)})


def unary_weights(symbols: Sequence[int]) -> List[int]:
    """Code lengths 1, 2, ..., n - 1, n - 1 in the order given: the deepest tree over n symbols."""
    n = len(symbols)
    return weights_of_lengths({s: min(i + 1, n - 1) for i, s in enumerate(symbols)})


def skewed_weights(symbols: Sequence[int], unary: int = 3) -> List[int]:
    """Code lengths 1..unary for the first symbols, the others share what is left in a balanced code."""
    lengths = {s: i + 1 for i, s in enumerate(symbols[:unary])}
    rest = balanced_weights(range(len(symbols) - unary))
    log = sum(1 << (w - 1) for w in rest).bit_length() - 1
    for s, w in zip(symbols[unary:], rest):
        lengths[s] = unary + log + 1 - w
    return weights_of_lengths(lengths)


def huffman_codes(weights: Sequence[int]) -> Dict[int, Tuple[int, int]]:
    """{symbol: (code, bits)} of a weight list that includes the last symbol's weight."""
    t = huffman_build(list(weights[:-1]))
    out = {}
    for i in range(len(t.symbol) - 1, -1, -1):
        out[t.symbol[i]] = (i >> (t.log - t.bits[i]), t.bits[i])
    assert [w > 0 for w in weights] == [s in out for s in range(len(weights))], "the last weight is not the deduced one"
    return out


def huffman_stream(codes, data: bytes) -> bytes:
    return backward([codes[b] for b in data])


def tree_description(weights: Sequence[int], how: str = "direct", log: int = 6) -> bytes:
    """The tree description of a weight list (its last weight is left out: the reader deduces it): ``direct``
    4-bit weights, or ``fse``: the weights FSE-compressed with two states that take turns."""
    w = list(weights[:-1])
    if how == "direct":
        if not 1 <= len(w) <= 128:
            raise BuildError("direct weights are 1..128")
        w2 = w + [0]
        return bytes([127 + len(w)]) + bytes(w2[i] << 4 | w2[i + 1] for i in range(0, len(w), 2))
    if len(w) < 2:
        raise BuildError("FSE-compressed weights are 2 at least")
    counts: Dict[int, int] = {}
    for x in w:
        counts[x] = counts.get(x, 0) + 1
    norm = normalise(counts, log)
    t = fse_build(norm, log)
    desc, _ = fse_description(norm, log)

    def refillable(t, cells):  # the state whose turn it is at the end must ask for a bit the stream lacks
        return next(c for c in cells if t.bits[c] > 0)

    a, b = w[0::2], w[1::2]
    ends_on_a = len(w) % 2 == 0
    sa = fse_states(t, a, refillable if ends_on_a else 0)
    sb = fse_states(t, b, 0 if ends_on_a else refillable)
    reads = [(sa[0], log), (sb[0], log)]
    for j in range(1, len(sa)):
        reads.append((sa[j] - t.base[sa[j - 1]], t.bits[sa[j - 1]]))
        if j < len(sb):
            reads.append((sb[j] - t.base[sb[j - 1]], t.bits[sb[j - 1]]))
    body = desc + backward(reads)
    if len(body) >= 128:
        raise BuildError("the compressed weights take 128 bytes or more")
    return bytes([len(body)]) + body


# ---------------------------------------------------------------------------
# sections and blocks
# ---------------------------------------------------------------------------
def literals_header(kind: int, sf: int, regen: int, comp: int = 0) -> bytes:
    if kind < 2:
        if sf in (0, 2):
            if regen >= 32:
                raise BuildError("size format 0 holds 5 bits")
            return bytes([kind | regen << 3])
        nbits, nbytes = (12, 2) if sf == 1 else (20, 3)
        if regen >> nbits:
            raise BuildError("literals size does not fit its format")
        return (kind | sf << 2 | regen << 4).to_bytes(nbytes, "little")
    nbits, nbytes = ((10, 3), (10, 3), (14, 4), (18, 5))[sf]
    if regen >> nbits or comp >> nbits:
        raise BuildError("literals sizes do not fit their format")
    return (kind | sf << 2 | regen << 4 | comp << (4 + nbits)).to_bytes(nbytes, "little")


def sequence_count(n: int, nbytes: Optional[int] = None) -> bytes:
    if nbytes is None:
        nbytes = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if nbytes == 1 and n < 128:
        return bytes([n])
    if nbytes == 2 and 0 < n < 0x7F00:
        return bytes([128 + (n >> 8), n & 255])
    if nbytes == 3 and 0x7F00 <= n <= 0x7F00 + 0xFFFF:
        return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")
    raise BuildError(f"a count of {n} does not go into {nbytes} bytes")


def block_header(kind: int, size: int, last: bool) -> bytes:
    if size >> 21:
        raise BuildError("Block_Size has 21 bits")
    return (int(last) | kind << 1 | size << 3).to_bytes(3, "little")


def window_descriptor(need: int) -> Tuple[int, int]:
    """(the byte, the window) of the smallest Window_Descriptor that covers ``need`` bytes."""
    for exp in range(22):
        for mant in range(8):
            w = (1 << (10 + exp)) + ((1 << (10 + exp)) >> 3) * mant
            if w >= need:
                return exp << 3 | mant, w
    raise BuildError("no window that large")


def rep_step(rep: List[int], ll: int, ov: int) -> int:
    """The offset of a sequence, the history updated in place (3.1.1.5); 0 for "repeat offset 1 minus 1" = 0,
    which leaves the history alone."""
    if ov > 3:
        rep[:] = [ov - 3, rep[0], rep[1]]
        return ov - 3
    k = ov + (1 if ll == 0 else 0)
    if k == 1:
        return rep[0]
    if k == 2:
        rep[:] = [rep[1], rep[0], rep[2]]
    elif k == 3:
        rep[:] = [rep[2], rep[0], rep[1]]
    elif rep[0] - 1 == 0:
        return 0
    else:
        rep[:] = [rep[0] - 1, rep[0], rep[1]]
    return rep[0]


class Frame:
    """One frame in the making.  ``window``: a Window_Descriptor frame with the smallest window that covers it
    (None: the smallest, 1 KiB at least, that covers the whole output, so that no block is refused for its
    size); ``single``: a single-segment frame.  ``fcs_bytes`` 0/1/2/4/8, ``did_bytes`` 0/1/2/4 (a Dictionary_ID
    of 0), ``checksum``: the flag, and 4 arbitrary bytes behind the last block."""

    def __init__(self, window: Optional[int] = None, single: bool = False, fcs_bytes: Optional[int] = None,
                 did_bytes: int = 0, checksum: bool = False):
        self.window, self.single, self.fcs_bytes = window, single, fcs_bytes
        self.did_bytes, self.checksum = did_bytes, checksum
        self.blocks: List[Tuple[int, int, bytes]] = []  # (type, Block_Size, content)
        self.out = bytearray()   # what the blocks so far produce; it stops growing at the first refused block
        self.nominal = 0         # what all blocks would produce if each were accepted
        self.dead = False
        self.rep = [1, 4, 8]
        self.tables: List[Optional[FseTable]] = [None, None, None]
        self.weights: Optional[List[int]] = None

    # -- the executor ------------------------------------------------------------------------------------
    def refuse(self):
        """The next block is one the contract refuses: the expected bytes end here."""
        self.dead = True

    def _run(self, literals: bytes, seqs: Sequence[Seq]):
        self.nominal += len(literals) + sum(ml for _, ml, _ in seqs)
        if self.dead:
            return
        out, at, start = self.out, 0, len(self.out)
        for ll, ml, ov in seqs:
            out += literals[at:at + ll]
            at += ll
            off = rep_step(self.rep, ll, ov)
            if off == 0 or off > len(out) or at > len(literals):
                del out[start:]
                self.dead = True
                return
            for _ in range(ml):
                out.append(out[len(out) - off])
        out += literals[at:]

    # -- blocks ------------------------------------------------------------------------------------------
    def raw(self, data: bytes):
        self.blocks.append((0, len(data), bytes(data)))
        self._run(data, [])
        return self

    def rle(self, byte: int, n: int):
        self.blocks.append((1, n, bytes([byte])))
        self._run(bytes([byte]) * n, [])
        return self

    def literals_section(self, literals: bytes, kind: str = "raw", sf: Optional[int] = None,
                         weights: Optional[Sequence[int]] = None, tree: str = "direct", tree_log: int = 6) -> bytes:
        n = len(literals)
        if kind in ("raw", "rle"):
            if sf is None:
                sf = 0 if n < 32 else 1 if n < 4096 else 3
            if kind == "rle":
                if len(set(literals)) != 1:
                    raise BuildError("RLE literals are one byte repeated")
                return literals_header(1, sf, n) + literals[:1]
            return literals_header(0, sf, n) + literals
        body = b""
        if kind == "compressed":
            self.weights = list(weights) if weights is not None else balanced_weights(literals)
            body = tree_description(self.weights, tree, tree_log)
        elif self.weights is None:  # (a frame that is refused for it: any tree serves to write the streams)
            self.weights = balanced_weights(literals)
        codes = huffman_codes(self.weights)
        if sf is None:
            sf = 0 if n < 1024 else 2 if n < 16384 else 3
        if sf == 0:
            body += huffman_stream(codes, literals)
        else:
            seg = (n + 3) // 4
            parts = [huffman_stream(codes, literals[i * seg:(i + 1) * seg]) for i in range(4)]
            body += b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
            self.stream_bytes = [len(p) for p in parts]
        return literals_header(2 if kind == "compressed" else 3, sf, n, len(body)) + body

    def sequences_section(self, seqs: Sequence[Seq], modes=("predefined",) * 3, count_bytes: Optional[int] = None,
                          last=(0, 0, 0)) -> bytes:
        """``modes``: per table (LL, OF, ML) "predefined", "rle", "repeat", "fse" (a distribution made from the
        codes at the table's largest accuracy log) or ("fse", distribution, accuracy log).  ``last``: which cell
        each table's last state takes (see ``fse_states``)."""
        if not seqs:
            return b"\0"
        codes = list(zip(*[seq_codes(q) for q in seqs]))
        head, byte = b"", 0
        for k, mode in enumerate(modes):
            name = mode if isinstance(mode, str) else mode[0]
            byte |= ("predefined", "rle", "fse", "repeat").index(name) << (6 - 2 * k)
            if name == "predefined":
                self.tables[k] = fse_build(*DEFAULTS[k])
            elif name == "rle":
                if len(set(codes[k])) != 1:
                    raise BuildError("an RLE table has one code")
                self.tables[k] = FseTable(0, [codes[k][0]], [0], [0])
                head += bytes([codes[k][0]])
            elif name == "fse":
                if isinstance(mode, str):
                    counts: Dict[int, int] = {}
                    for c in codes[k]:
                        counts[c] = counts.get(c, 0) + 1
                    norm, log = normalise(counts, MAX_LOG[k]), MAX_LOG[k]
                else:
                    norm, log = mode[1], mode[2]
                self.tables[k] = fse_build(list(norm), log)
                head += fse_description(norm, log)[0]
            elif self.tables[k] is None:  # (a frame that is refused for it: any table serves to write the bits)
                self.tables[k] = fse_build(*DEFAULTS[k])
        llt, oft, mlt = self.tables
        lls, ofs, mls = (fse_states(t, c, w) for t, c, w in zip(self.tables, codes, last))
        reads = [(lls[0], llt.log), (ofs[0], oft.log), (mls[0], mlt.log)]
        for i, (ll, ml, ov) in enumerate(seqs):
            lc, oc, mc = codes[0][i], codes[1][i], codes[2][i]
            reads += [(ov - (1 << oc), oc), (ml - ML_BASE[mc], ML_BITS[mc]), (ll - LL_BASE[lc], LL_BITS[lc])]
            if i + 1 < len(seqs):
                reads += [(lls[i + 1] - llt.base[lls[i]], llt.bits[lls[i]]),
                          (mls[i + 1] - mlt.base[mls[i]], mlt.bits[mls[i]]),
                          (ofs[i + 1] - oft.base[ofs[i]], oft.bits[ofs[i]])]
        self.reads = reads  # (of the last sequences section written: for the tests that count its bits)
        return sequence_count(len(seqs), count_bytes) + bytes([byte]) + head + backward(reads)

    def compressed(self, literals: bytes, seqs: Sequence[Seq] = (), lit: Optional[dict] = None, modes=("predefined",) * 3,
                   count_bytes: Optional[int] = None, last=(0, 0, 0)):
        body = self.literals_section(literals, **(lit or {})) + self.sequences_section(seqs, modes, count_bytes, last)
        self.blocks.append((2, len(body), body))
        self._run(literals, seqs)
        return self

    def block(self, triples: Sequence[Tuple[bytes, int, int]], tail: bytes = b"", **kw):
        """A Compressed block from (literal bytes, match length, offset value) and the trailing literals."""
        return self.compressed(b"".join(t[0] for t in triples) + tail, [(len(a), ml, ov) for a, ml, ov in triples], **kw)

    # -- the frame ---------------------------------------------------------------------------------------
    def bytes(self, content: Optional[int] = None) -> bytes:
        """``content``: the Frame_Content_Size to state (default: what the blocks would produce)."""
        content = self.nominal if content is None else content
        fcs = self.fcs_bytes
        if fcs is None:
            fcs = 0 if not self.single else 1 if content < 256 else 2 if content < 65536 + 256 else 4
        if self.single and fcs == 0:
            raise BuildError("a single-segment frame states its size")
        if fcs == 1 and not self.single:
            raise BuildError("a 1-byte content size needs a single segment")
        head = bytearray(MAGIC)
        head.append({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs] << 6 | self.single << 5 | self.checksum << 2 |
                    {0: 0, 1: 1, 2: 2, 4: 3}[self.did_bytes])
        if not self.single:
            head.append(window_descriptor(self.window or max(KIB, self.nominal))[0])
        head += bytes(self.did_bytes)
        if fcs:
            head += (content - (256 if fcs == 2 else 0)).to_bytes(fcs, "little")
        for i, (kind, size, body) in enumerate(self.blocks):
            head += block_header(kind, size, i + 1 == len(self.blocks)) + body
        return bytes(head) + ((xxh64(bytes(self.out)) & 0xFFFFFFFF).to_bytes(4, "little") if self.checksum else b"")

    def case(self, what: str, ok: bool = True, out_n: Optional[int] = None, content: Optional[int] = None) -> Case:
        out_n = self.nominal if out_n is None else out_n
        if ok and (self.dead or len(self.out) != out_n):
            raise BuildError(f"{what}: the executor does not accept what the case calls valid")
        return Case(what, self.bytes(content), out_n, ok, bytes(self.out), len(self.blocks))


def xxh64(data: bytes) -> int:
    """XXH64 with seed 0: the low 4 bytes are a frame's Content_Checksum (3.1.1)."""
    P1, P2, P3, P4, P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579,
                          2870177450012600261)
    M = (1 << 64) - 1
    rotl = lambda x, r: (x << r | x >> (64 - r)) & M  # noqa: E731
    word = lambda i, n: int.from_bytes(data[i:i + n], "little")  # noqa: E731
    rnd = lambda acc, v: rotl((acc + v * P2) & M, 31) * P1 & M  # noqa: E731
    n, i = len(data), 0
    if n >= 32:
        v = [(P1 + P2) & M, P2, 0, -P1 & M]
        while i + 32 <= n:
            v = [rnd(v[k], word(i + 8 * k, 8)) for k in range(4)]
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = P5
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, word(i, 8)), 27) * P1 + P4) & M
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ word(i, 4) * P1 & M, 23) * P2 + P3) & M
        i += 4
    while i < n:
        h = rotl(h ^ data[i] * P5 & M, 11) * P1 & M
        i += 1
    h = (h ^ h >> 33) * P2 & M
    h = (h ^ h >> 29) * P3 & M
    return h ^ h >> 32


def ov_of(offset: int) -> int:
    return offset + 3


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------
OVERLAP_OFFSETS = list(range(1, 131)) + [191, 192, 193, 255, 256, 257]
OVERLAP_LENGTHS = [3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]


@functools.lru_cache(maxsize=None)
def overlap() -> List[Case]:
    """execute, the pattern copy (``at = lane % off``, ``adv = kWave % off``, the wrap ``at -= off``) and,
    where the length is at most the offset, ``wave_copy``.  Per offset one frame of 48 sequences: for every
    length four of them, each a fresh pattern of ``off`` distinct bytes repeated by one match whose first
    output byte lies at each misalignment mod 4 of the frame's output."""
    out = []
    for off in OVERLAP_OFFSETS:
        triples, pos = [], 0
        for n in OVERLAP_LENGTHS:
            for m in range(4):
                pad = (m - pos - off) % 4
                triples.append((lits(pad, n + m) + lits(off, off + m), n, ov_of(off)))
                pos += pad + off + n
        out.append(Frame().block(triples, lits(5, off)).case(f"overlap off={off}"))
    return out


APART_LENGTHS = [255, 256, 257, 511, 512, 513, 1023]
APART_GAPS = [0, 1, 3]
RESTS = [0, 1, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def apart() -> List[Case]:
    """execute, ``wave_copy`` (256-byte turns of 4 bytes per lane, then the byte tail) for literals, matches
    and trailing literals: a Raw block of 0..6 bytes, then one sequence whose literal run and match are both
    ``n`` bytes, the match's source ``gap`` bytes clear of its destination, the destination at each
    misalignment mod 4, and ``rest`` trailing literals."""
    out, i = [], 0
    for n in APART_LENGTHS:
        for gap in APART_GAPS:
            for d in range(4):
                pad = (d - n - gap) % 4
                rest = RESTS[i % len(RESTS)]
                i += 1
                f = Frame().raw(lits(pad + gap, d))
                f.block([(lits(n, n + gap), n, ov_of(n + gap))], lits(rest, 9))
                out.append(f.case(f"apart len={n} gap={gap} dst%4={d} rest={rest}"))
    return out


def _valid_seqs(rng: Lcg, n: int, have: int, rep: List[int], ll0_at=()) -> Tuple[List[Seq], int]:
    """n sequences that are valid behind ``have`` output bytes: new offsets 1..16 and repeat codes, literal
    lengths 0..4, match lengths 3..11; at the indices ``ll0_at`` a repeat code with no literals."""
    seqs, rep = [], list(rep)
    while len(seqs) < n:
        i = len(seqs)
        ll = 0 if i in ll0_at else rng.below(5)
        ov = 1 + rng.below(3) if i in ll0_at or rng.below(3) == 0 else ov_of(1 + rng.below(16))
        trial = list(rep)
        off = rep_step(trial, ll, ov)
        if off == 0 or off > have + ll:
            if i in ll0_at:
                ov = 1 + ov % 3
                off = rep_step(trial := list(rep), ll, ov)
                if off == 0 or off > have + ll:
                    raise BuildError("no valid repeat code here")
            else:
                continue
        rep = trial
        ml = 3 + rng.below(9)
        seqs.append((ll, ml, ov))
        have += ll + ml
    return seqs, have


GROUP_COUNTS = [1, 63, 64, 65, 127, 128, 129, 200]


@functools.lru_cache(maxsize=None)
def batches_of_64() -> List[Case]:
    """execute, the loop that deals sequences to the wave 64 at a time (``here = min(seq_count - t, kWave)``
    and the three ``__shfl``): blocks of 1..200 sequences, a repeat code without literals in the last sequence
    of one group of 64 and in the first of the next; each count in a frame of its own, then all in one frame,
    where the history is carried from block to block."""
    out = []
    both = Frame()
    both.raw(lits(20, 1))
    for n in GROUP_COUNTS:
        for f, what in ((Frame().raw(lits(20, n)), f"batches_of_64 count={n}"), (both, None)):
            rng = Lcg(n)
            ll0 = (63, 64, 127, 128) if n > 64 else ()
            seqs, _ = _valid_seqs(rng, n, len(f.out), f.rep, ll0)
            f.compressed(lits(sum(q[0] for q in seqs) + 3, n), seqs)
            if what:
                out.append(f.case(what))
    out.append(both.case("batches_of_64 all counts in one frame"))
    return out


WATERMARK_KINDS = ["ends_at_W", "ends_at_W_plus_1", "starts_at_W_minus_1", "in_previous_sequence",
                   "in_own_literals", "copies_previous_match"]


def _chain(kind: str, n: int, nlit: int, alternate: bool, seed: int):
    """A head sequence (24 literals and a match, after which W = 24) and n more with ``nlit`` literals each.
    W restates the execute kernel's rule: a match whose source ``[op - off, op - off + min(ml, off))`` ends
    above ``flushed`` waits for the wave's stores, and ``flushed`` becomes the position at which that match
    starts.  (sequences as (literal bytes, match length, offset value), [(kind, source start, source end, W)])"""
    rng = Lcg(seed)
    seqs = [(lits(24, seed, FILL), 6, ov_of(9))]
    placed = []
    W = 24                             # the head's match reads [15, 21) with W = 0: it waits at op = 24
    op, prev_start, pm_start, pm_len = 30, 0, 24, 6
    for j in range(1, n + 1):
        lit = lits(nlit, seed + j, FILL)
        at = op + nlit                 # where this match's output starts
        k = kind if not alternate or j % 2 else "in_previous_sequence"
        if k == "in_own_literals" and nlit == 0:
            k = "copies_previous_match"
        if k == "ends_at_W":
            m = 4 + rng.below(min(W, 40) - 3)
            s = W - m
        elif k == "ends_at_W_plus_1":
            m = 4 + rng.below(min(W + 1, 40) - 3)
            s = W + 1 - m
        elif k == "starts_at_W_minus_1":
            m = 4 + rng.below(37)      # (longer than at - s: an overlapped match, whose source ends at `at`)
            s = W - 1
        elif k == "in_previous_sequence":
            avail = op - prev_start
            m = 4 + rng.below(min(avail, 40) - 3)
            s = prev_start + rng.below(avail - m + 1)
        elif k == "in_own_literals":   # the source starts in the literals this sequence has just stored
            m = 3 + rng.below(13)
            s = op + rng.below(nlit)
        else:                          # copies_previous_match (overlapped where it is longer than what is there)
            m = 4 + rng.below(13)
            s = pm_start + rng.below(pm_len)
        off = at - s
        span = min(m, off)
        placed.append((k, s, s + span, W))
        seqs.append((lit, m, ov_of(off)))
        if s + span > W:
            W = at
        prev_start, pm_start, pm_len, op = op, at, m, at + m
    return seqs, placed


@functools.lru_cache(maxsize=None)
def watermark_chains():
    out = []
    for ki, kind in enumerate(WATERMARK_KINDS):
        for alternate in (False, True):
            if alternate and kind in ("in_previous_sequence", "copies_previous_match"):
                continue
            for n in range(2, 41, 5):
                for nlit in range(4):
                    what = f"watermark {kind}{' alternating' if alternate else ''} chain={n} literals={nlit}"
                    out.append((what, *_chain(kind, n, nlit, alternate, 1000 * ki + 500 * alternate + 4 * n + nlit)))
    return out


@functools.lru_cache(maxsize=None)
def watermark() -> List[Case]:
    """execute, the store watermark (``if (op - off + span > flushed)`` before a match: ``s_waitcnt vmcnt(0)``
    and ``flushed = op``): chains of matches whose source ends exactly at the last wait (no new wait), one
    byte past it, straddles it, lies in the literals the same sequence has just stored, in the sequence before
    or in the previous match's output; then matches without literals that read the last bytes of a Raw and of
    an RLE block right before the Compressed block.  Several hundred chains in one launch, so that many waves
    share a CU.  This pins the bytes at the rule's edges and makes a stale read possible to observe (the
    literals avoid the buffer's fill byte); it cannot make one certain, and whether a missing wait is
    observable on this hardware has not been measured."""
    out = [Frame().block(seqs, lits(5, len(seqs), FILL)).case(what) for what, seqs, _ in watermark_chains()]
    for n in (1, 3, 64, 257):
        for off in sorted({o for o in (1, 2, 3, n) if o <= n}):
            for ml in (3, 70):
                f = Frame().raw(lits(n, off, FILL)).block([(b"", ml, ov_of(off))], lits(2, 5, FILL))
                out.append(f.case(f"watermark behind a Raw block of {n}, off={off} ml={ml}"))
                f = Frame().raw(lits(3, 1, FILL)).rle((0x33 + off) & 255, n).block([(b"", ml, ov_of(off))])
                out.append(f.case(f"watermark behind an RLE block of {n}, off={off} ml={ml}"))
    return out


@functools.lru_cache(maxsize=None)
def repeat_offsets() -> List[Case]:
    """execute, ``resolve_offset`` and the ``rep[3]`` it carries over the blocks of a frame: the six cases
    rep:1..3 with and without literals, each several times between new offsets; the history carried across a
    Raw block, an RLE block, a Compressed block without sequences and from one Compressed block into the next;
    the initial history 1, 4, 8; and "repeat offset 1 minus 1", which is refused where it gives 0."""
    out = []
    # the six cases in every order of a fixed cycle, the three offsets kept distinct by new ones in between
    for turn in range(4):
        f = Frame().raw(lits(40, turn))
        triples = [(lits(2, 1), 4, ov_of(5 + turn)), (lits(1, 2), 5, ov_of(9 + turn)), (lits(3, 3), 3, ov_of(17 + turn))]
        for j, (code, ll) in enumerate([(1, 2), (2, 1), (3, 1), (1, 0), (2, 0), (3, 0)] * 3):
            code = 1 + (code - 1 + turn) % 3
            triples.append((lits(ll, j), 3 + (j + turn) % 7, code))
            if j % 4 == 3:
                triples.append((lits(1, j), 4, ov_of(6 + j + turn)))
        out.append(f.block(triples, lits(3, 7)).case(f"repeat_offsets six cases, turn {turn}"))
    # carried across blocks: every Compressed block opens with repeat codes that read the history left before
    for code in (1, 2, 3):
        for ll in (0, 2):
            f = Frame().raw(lits(40, code))
            f.block([(lits(2, 1), 4, ov_of(7)), (lits(1, 2), 5, ov_of(11)), (lits(3, 3), 3, ov_of(13))])
            f.raw(lits(9, 4))
            f.block([(lits(ll, 5), 6, code), (lits(1, 6), 4, ov_of(21))])
            f.rle(0x44, 5)
            f.block([(lits(ll, 7), 5, code), (lits(2, 8), 4, ov_of(19))])
            f.compressed(lits(6, 9))
            f.block([(lits(ll, 10), 7, code), (lits(1, 11), 3, ov_of(23))])
            f.block([(lits(ll, 12), 4, code), (lits(ll, 13), 5, 1 + code % 3)], lits(2, 14))
            out.append(f.case(f"repeat_offsets carried over blocks, code {code}, {ll} literals"))
    # the first sequences of a frame: 1, 4, 8
    for code, ll, off in ((1, 1, 1), (2, 1, 4), (3, 1, 8), (1, 0, 4), (2, 0, 8)):
        f = Frame().raw(lits(16, code)).block([(lits(ll, 3), 9, code), (lits(ll, 4), 5, 2), (lits(1, 5), 4, 3)], lits(1, 6))
        out.append(f.case(f"repeat_offsets initial history, code {code} with {ll} literals is offset {off}"))
    f = Frame().raw(lits(16, 9)).block([(b"", 4, 3)], lits(1, 6))
    out.append(f.case("repeat_offsets initial history, code 3 without literals is offset 0", ok=False))
    for first, ok in ((1, False), (2, True)):
        f = Frame().raw(lits(16, first)).block([(lits(2, 1), 4, ov_of(first)), (b"", 5, 3), (lits(1, 2), 3, 1)], lits(1, 6))
        out.append(f.case(f"repeat_offsets repeat offset 1 minus 1 with repeat offset 1 = {first}", ok=ok))
    return out


def _norm(symbols: Sequence[int], log: int, variant: int) -> Tuple[str, List[int], int]:
    """("fse", a distribution over the symbols, log): different for every ``variant``."""
    counts = {s: 1 + (i * 5 + variant * 3) % 7 for i, s in enumerate(sorted(set(symbols)))}
    return "fse", normalise(counts, log, sorted(counts)[variant % len(counts)]), log


LLS, OFS, MLS = range(0, 8), range(2, 5), range(0, 10)  # the codes the chain blocks draw on


def _chain_block(f: Frame, salt: int, modes, lit=None, n: int = 9, rle=(None, None, None)):
    """A block of n sequences (ll 0..7, ml 3..12, offsets 1..28) with the given table modes; an RLE table fixes
    that field to one code."""
    rng, seqs, have = Lcg(salt), [], len(f.out)
    for _ in range(n):
        ll = rle[0] if rle[0] is not None else rng.below(8)
        ml = 3 + (rle[2] if rle[2] is not None else rng.below(10))
        lo, hi = (1 << rle[1], (2 << rle[1]) - 1) if rle[1] is not None else (4, 31)
        ov = lo + rng.below(min(hi, have + ll + 3) - lo + 1)
        seqs.append((ll, ml, ov))
        have += ll + ml
    literals = lits(sum(q[0] for q in seqs) + 2, salt, below=16)
    return f.compressed(literals, seqs, lit=lit, modes=modes)


def _fse3(v: int):
    return (_norm(LLS, 5 + v % 3, v), _norm(OFS, 5 + (v + 1) % 3, v + 1), _norm(MLS, 5 + (v + 2) % 3, v + 2))


TREE_A = dict(kind="compressed", weights=skewed_weights([3, 1, 4, 0, 5, 9, 2, 6, 8, 7, 10, 11, 12, 13, 14, 15]))
TREE_B = dict(kind="compressed", weights=balanced_weights(range(16)))
TREE_C = dict(kind="compressed", weights=skewed_weights(list(range(15, -1, -1)), 5), tree="fse")


@functools.lru_cache(maxsize=None)
def chains() -> List[Case]:
    """index, ``walk_frame``'s ``last_huf`` / ``last_tab[3]`` -> ``huf_src`` / ``tab_src[3]``, and entropy,
    ``block_sequences`` with ``table_position``, which rebuild a Treeless tree or a Repeat table from the
    supplying block's bytes.  Every supplier has a distribution of its own, so a table taken from another
    block reads other sequences.  Of the blocks put in between, the raw-literals and the RLE-literals block with
    Predefined tables supply the tables themselves and leave only the tree to the real supplier; their twins
    with Repeat tables leave it the tables too."""
    out = []
    R3, P3 = ("repeat",) * 3, ("predefined",) * 3
    between = {
        "nothing": lambda f: f,
        "a Raw block": lambda f: f.raw(lits(7, 1)),
        "an RLE block": lambda f: f.rle(0x5A, 9),
        "a raw-literals block": lambda f: _chain_block(f, 70, P3),
        "an RLE-literals block": lambda f: f.compressed(b"\x07" * 9, [(4, 3, 5)], lit=dict(kind="rle")),
        "a raw-literals block with Repeat tables": lambda f: _chain_block(f, 71, R3),
        "an RLE-literals block with Repeat tables":
            lambda f: f.compressed(b"\x07" * 9, [(4, 3, 5)], lit=dict(kind="rle"), modes=R3),
        "a zero-sequence block": lambda f: f.compressed(lits(5, 3)),
        "a zero-sequence block with a tree of its own": lambda f: f.compressed(lits(40, 3, below=16), lit=TREE_B),
    }
    for name, put in between.items():
        for back in (1, 2, 5):
            if name == "nothing" and back > 1:
                continue
            f = Frame().raw(lits(30, back))
            _chain_block(f, 1, _fse3(0), lit=TREE_B)        # an older supplier, which must not be used
            _chain_block(f, 2, _fse3(back), lit=TREE_A)     # the supplier
            for _ in range(back - 1 if name != "nothing" else 0):
                put(f)
            treeless = "tree of its own" not in name
            _chain_block(f, 3, R3, lit=dict(kind="treeless") if treeless else None)
            out.append(f.case(f"chains supplier {back} back, {name} in between"))
    # LL, OF and ML each from a different block; then Repeat of a Repeat through to the real suppliers
    f = Frame().raw(lits(30, 7))
    a, b, c = _fse3(1), _fse3(2), _fse3(3)
    _chain_block(f, 10, a)
    _chain_block(f, 11, (b[0], "repeat", "repeat"))
    _chain_block(f, 12, ("repeat", c[1], "repeat"))
    _chain_block(f, 13, R3)
    _chain_block(f, 14, R3)
    _chain_block(f, 15, ("repeat", "repeat", b[2]))
    _chain_block(f, 16, R3)
    out.append(f.case("chains each table from another block, Repeat of a Repeat"))
    # Repeat of an RLE table and of a Predefined table, one table at a time
    for k, name in enumerate(("ll", "of", "ml")):
        for mode in ("rle", "predefined"):
            f = Frame().raw(lits(30, k))
            first = list(_fse3(4 + k))
            first[k] = mode
            code = [5, 3, 7][k]
            rle = tuple(code if j == k and mode == "rle" else None for j in range(3))
            _chain_block(f, 20 + k, tuple(first), rle=rle)
            f.rle(1, 4)
            again = list(_fse3(5 + k))
            again[k] = "repeat"
            _chain_block(f, 23 + k, tuple(again), rle=rle)
            _chain_block(f, 26 + k, R3, rle=rle)
            out.append(f.case(f"chains Repeat of a {mode} {name} table"))
    # the supplier's table k behind FSE descriptions, an RLE byte, or a Repeat that takes no bytes
    shapes = {
        "ml behind two FSE descriptions": (lambda v: _fse3(v), (None, None, None)),
        "of behind one FSE description": (lambda v: _fse3(v), (None, None, None)),
        "of behind an RLE byte": (lambda v: ("rle",) + _fse3(v)[1:], (4, None, None)),
        "ml behind two RLE bytes": (lambda v: ("rle", "rle", _fse3(v)[2]), (4, 3, None)),
        "ml behind an RLE byte and an FSE description": (lambda v: ("rle",) + _fse3(v)[1:], (2, None, None)),
        "of behind a Repeat": (lambda v: ("repeat",) + _fse3(v)[1:], (None, None, None)),
        "ml behind two Repeats": (lambda v: ("repeat", "repeat", _fse3(v)[2]), (None, None, None)),
        "ml behind a Repeat and an FSE description": (lambda v: ("repeat",) + _fse3(v)[1:], (None, None, None)),
    }
    for v, (name, (modes, rle)) in enumerate(shapes.items()):
        f = Frame().raw(lits(30, v))
        _chain_block(f, 30 + v, _fse3(v + 6))
        _chain_block(f, 40 + v, modes(v + 7), rle=rle)
        f.raw(lits(3, v))
        _chain_block(f, 50 + v, R3, rle=rle)
        out.append(f.case(f"chains supplier with {name}"))
    # Treeless: 1 stream from 4 and the reverse, twice in a row, and the tree FSE-compressed
    for tree, tname in ((TREE_A, "direct"), (TREE_C, "fse")):
        for first, then in ((0, 1), (1, 0)):
            f = Frame().raw(lits(30, first))
            _chain_block(f, 60, P3, lit=dict(TREE_B, sf=then))
            f.compressed(lits(900, 5, below=16), [(5, 4, 9)], lit=dict(tree, sf=first))
            f.compressed(lits(777, 6, below=16), [(700, 3, 8)], lit=dict(kind="treeless", sf=then))
            f.compressed(lits(401, 7, below=16), lit=dict(kind="treeless", sf=first))
            f.compressed(lits(50, 8, below=16), [(9, 3, 1)], lit=dict(kind="treeless", sf=1))
            out.append(f.case(f"chains Treeless, {tname} tree with {'4' if first else '1'} stream(s) "
                              f"into {'4' if then else '1'}, twice more"))
    # refused
    f = Frame().raw(lits(30, 1))
    f.refuse()
    f.compressed(lits(40, 1, below=16), [(5, 4, 9)], lit=dict(kind="treeless", sf=0))
    out.append(f.case("chains Treeless in the first Compressed block", ok=False))
    f = Frame().raw(lits(30, 2)).compressed(lits(9, 3))  # (raw literals: it leaves no tree)
    f.refuse()
    f.compressed(lits(40, 1, below=16), lit=dict(kind="treeless", sf=0))
    out.append(f.case("chains Treeless behind raw literals only", ok=False))
    for k, name in enumerate(("ll", "of", "ml")):
        modes = tuple("repeat" if j == k else "predefined" for j in range(3))
        f = Frame().raw(lits(30, 3))
        f.refuse()
        _chain_block(f, 80, modes)
        out.append(f.case(f"chains Repeat {name} in the first Compressed block", ok=False))
        f = Frame().raw(lits(30, 4)).compressed(lits(9, 3)).compressed(lits(8, 4))
        f.refuse()
        _chain_block(f, 81, modes)
        out.append(f.case(f"chains Repeat {name} behind zero-sequence blocks only", ok=False))
    return out


@functools.lru_cache(maxsize=None)
def isolation() -> List[Case]:
    """index and entropy across frames of one batch: ``last_huf`` / ``last_tab`` start at kNone in every frame
    and ``fblocks`` is the frame's own block list, so a frame that opens with Treeless or Repeat behind a frame
    that left a tree and tables is refused; the workgroup barrier of the entropy kernel
    (``__syncthreads`` behind the tree build) with waves that hold Raw, RLE, raw-literals and Huffman blocks of
    different frames.  The order of the list is the order in the batch.  It opens with a frame of two Raw
    blocks whose third block header is cut: ``walk_frame`` counts the two (``fr.nblocks``) although the caller
    could promise only one, and the dealer of slots must not let them cost a valid frame behind it its own
    (the two passes over the frames).  It ends with frames whose blocks are all sound and which are refused for
    what follows the last block (``fr.nblocks = nb`` before that check)."""
    out = []
    P3, R3 = ("predefined",) * 3, ("repeat",) * 3
    a, b, c = lits(70, 1), lits(33, 2), lits(9, 3)
    whole = Frame().raw(a).raw(b).raw(c)
    out.append(Case("isolation two Raw blocks, then a block header cut after 2 bytes", whole.bytes()[:-len(c) - 1],
                    whole.nominal, False, a + b, 1))

    def leaves(salt):  # one block that leaves a tree and three tables
        f = Frame().raw(lits(12, salt)) if salt % 2 else Frame()
        if not salt % 2:
            f.raw(lits(30, salt))
        return _chain_block(f, salt, _fse3(salt), lit=TREE_A if salt % 3 else TREE_B)

    out.append(leaves(1).case("isolation frame that leaves a tree and tables (1)"))
    f = Frame()
    f.refuse()
    f.compressed(lits(40, 1, below=16), [(5, 4, 4)], lit=dict(kind="treeless", sf=0))
    out.append(f.case("isolation opens with Treeless behind another frame's tree", ok=False))
    out.append(leaves(2).case("isolation frame that leaves a tree and tables (2)"))
    f = Frame().raw(lits(30, 5))
    f.refuse()
    _chain_block(f, 5, R3)
    out.append(f.case("isolation opens with Repeat behind another frame's tables", ok=False))
    out.append(leaves(3).case("isolation frame that leaves a tree and tables (3)"))
    # the barrier: blocks of every kind side by side in a workgroup's four waves
    f = Frame().raw(lits(33, 6))
    _chain_block(f, 6, P3, lit=TREE_A)
    f.rle(9, 70)
    _chain_block(f, 7, P3)
    f.compressed(b"\x08" * 20, [(4, 3, 5)], lit=dict(kind="rle"))
    _chain_block(f, 8, ("repeat", "predefined", "repeat"), lit=dict(kind="treeless", sf=1), n=40)
    out.append(f.case("isolation mixed blocks: Raw, Huffman, RLE, raw literals, RLE literals, Treeless"))
    out.append(Frame().rle(0x11, 300).case("isolation one RLE block"))
    f = Frame()
    _chain_block(f.raw(lits(20, 9)), 9, _fse3(9), lit=TREE_B)
    _chain_block(f, 10, R3, lit=dict(kind="treeless", sf=0))
    out.append(f.case("isolation Huffman and Treeless blocks"))
    out.append(Frame().raw(lits(257, 3)).case("isolation one Raw block"))
    for checksum in (False, True):
        f = Frame(checksum=checksum).raw(lits(20, 4)).block([(lits(4, 1), 5, ov_of(7))], lits(1, 2))
        whole = f.case("whole")
        out.append(whole._replace(what="isolation a byte behind the frame" + " and its checksum" * checksum,
                                  frame=whole.frame + b"\0", ok=False))
    out.append(whole._replace(what="isolation the checksum's last byte missing", frame=whole.frame[:-1], ok=False))
    return out


ISOLATION_BATCHES = [1, 2, 3, 4, 5, 9]


def isolation_batch(nblocks: int) -> List[Case]:
    """Valid frames of ``isolation``, in its order, that hold ``nblocks`` blocks together: of the choices the
    one with the most frames."""
    valid = [c for c in isolation() if c.ok]
    best: List[Case] = []
    for mask in range(1 << len(valid)):
        pick = [c for i, c in enumerate(valid) if mask >> i & 1]
        if sum(c.blocks for c in pick) == nblocks and len(pick) > len(best):
            best = pick
    assert best
    return best


def _huf_frame(what: str, literals: bytes, lit: dict, seqs: Sequence[Seq] = (), ok: bool = True, lead: bytes = b""):
    f = Frame()
    if lead:
        f.raw(lead)
    if not ok:
        f.refuse()
    f.compressed(literals, seqs, lit=lit)
    return f.case(what, ok=ok), f


DEEP = [65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76]  # a tree of depth 11 over 12 symbols: 'A' has 1 bit


@functools.lru_cache(maxsize=None)
def literals() -> List[Case]:
    """entropy: the literals of every type and size format (``wave_copy`` for raw, the lane loop for RLE), the
    four Huffman streams in four lanes (``huf_four_streams``, ``lits + lane * cnt[0]``, ``__all(mine)``),
    ``BackwardBits::refill``'s 8-byte and byte-wise paths with streams of 1..17 bytes, the last peeks
    zero-padded below the stream's start, and trees at the format's limits.  (Three of four streams hold the
    same number of literals and the last at most 3 fewer, and a literal takes 1 to 11 bits: a stream of 1 byte
    cannot lie beside one of 300.  The most unequal ones the format holds are here: 38 beside 413 bytes, and
    1 beside 14.)"""
    out = []
    add = lambda what, *a, **kw: out.append(_huf_frame("literals " + what, *a, **kw)[0])  # noqa: E731
    for n, sfs in ((0, (1, 3)), (1, (0, 1, 3)), (31, (0, 1, 3)), (32, (1, 3)), (4095, (1, 3)), (4096, (3,))):
        for sf in sfs:
            add(f"raw {n} in size format {sf}", lits(n, n), dict(kind="raw", sf=sf), [(n, 3, 4)] if n else [],
                lead=lits(5, 2))
    for n, sfs in ((1, (0, 1, 3)), (7, (0, 1, 3)), (20, (0,)), (31, (0, 1, 3)), (32, (1, 3)), (300, (1,)), (4097, (3,))):
        for sf in sfs:
            add(f"rle {n} in size format {sf}", bytes([n & 255]) * n, dict(kind="rle", sf=sf), [(n // 2, 4, 5)],
                lead=lits(5, 3))
    # compressed and treeless in every size format, at the sizes where the format changes
    for n, sfs in ((1023, (0, 1, 2, 3)), (1024, (2, 3)), (16383, (2, 3)), (16384, (3,))):
        for sf in sfs:
            f = Frame()
            f.compressed(lits(n, sf, below=16), [(n - 3, 5, 7)], lit=dict(TREE_A, sf=sf))
            f.compressed(lits(n, sf + 4, below=16), [(1, 3, 1)], lit=dict(kind="treeless", sf=sf))
            out.append(f.case(f"literals compressed and treeless {n} in size format {sf}"))
    # four streams, the regenerated size at every remainder mod 4, from the smallest on
    for n in (4, 6, 7, 8, 9, 10, 11, 12, 13, 61, 62, 63, 64, 65, 66, 67):
        seg = (n + 3) // 4
        add(f"4 streams of {n} literals, the last holds {n - 3 * seg}", lits(n, n, below=16), dict(TREE_B, sf=1))
    # stream lengths in bytes: 'A' has a 1-bit code, so a stream of 8k - 1 of them is k bytes
    deep = dict(kind="compressed", weights=unary_weights(DEEP))
    for nbytes in list(range(1, 10)) + [15, 16, 17]:
        add(f"1 stream of {nbytes} bytes", b"A" * (8 * nbytes - 1), dict(deep, sf=0))
        add(f"1 stream of {nbytes} bytes, an 11-bit code first and a 1-bit code last",
            b"L" + b"A" * (8 * nbytes - 12) if nbytes > 1 else b"AAAAAAA", dict(deep, sf=0))
        seg = 8 * nbytes - 1
        text = b"A" * seg + (b"L" * 8 + b"A" * seg)[:seg] + b"A" * seg + b"K" * (seg - 2)
        add(f"4 streams of {nbytes} bytes and longer", text, dict(deep, sf=1))
    # the most unequal streams the format can hold: every stream but the last has the same number of literals
    add("4 streams of 38, 413, 38 and 413 bytes", b"A" * 300 + b"L" * 300 + b"A" * 300 + b"K" * 300, dict(deep, sf=2))
    add("4 streams of 14, 14, 14 and 1 bytes", b"L" * 10 + b"K" * 10 + b"L" * 10 + b"A" * 7, dict(deep, sf=1))
    add("4 streams of 2, 2, 2 and 1 bytes", b"A" * 30 + b"AAAAAAA", dict(deep, sf=1))
    # trees
    add("tree of 2 symbols", bytes([0, 1, 1, 0, 1, 0, 0, 0, 1] * 5), dict(kind="compressed", weights=[1, 1], sf=0))
    w129 = weights_of_lengths({s: 7 if s < 127 else 8 for s in range(129)})
    add("tree of 129 symbols, 128 direct weights (head byte 255)", lits(700, 1, below=128) + bytes([127, 128]) * 9,
        dict(kind="compressed", weights=w129, sf=1))
    w256 = weights_of_lengths({s: 7 if s == 0 else 9 if s in (100, 255) else 8 for s in range(256)})
    add("tree of 256 symbols, FSE-compressed weights", lits(1500, 2), dict(kind="compressed", weights=w256, tree="fse", sf=2))
    add("tree of 256 symbols, FSE-compressed weights at accuracy log 5", lits(600, 3),
        dict(kind="compressed", weights=w256, tree="fse", tree_log=5, sf=1))
    odd = weights_of_lengths({s: 2 if s < 3 else 3 for s in range(5)})  # an even count of FSE-compressed weights
    add("tree of 5 symbols, FSE-compressed weights", bytes([0, 1, 2, 3, 4] * 9), dict(kind="compressed", weights=odd, tree="fse", sf=0))
    add("tree of depth 11", bytes(DEEP) * 3, dict(deep, sf=0))
    deeper = DEEP + [77]
    f = Frame().raw(lits(9, 1))
    f.refuse()
    w = unary_weights(deeper)
    f.weights = w
    body = bytes([127 + 77]) + bytes((w + [0])[i] << 4 | (w + [0])[i + 1] for i in range(0, 77, 2))
    body += backward([(0, 12)] * 4)  # (no reader gets as far as the stream)
    f.blocks.append((2, 3 + len(body) + 1, literals_header(2, 0, 4, len(body)) + body + b"\0"))
    f.nominal += 4
    out.append(f.case("literals tree of depth 12", ok=False))
    return out


def _rle3(n: int, count_bytes=None):
    """n sequences of no literals and a match of 3 at offsets 1..4, all three tables RLE."""
    f = Frame().raw(lits(8, n))
    seqs = [(0, 3, 4 + (i * 7 + i // 5) % 4) for i in range(n)]
    return f.compressed(b"xyz", seqs, modes=("rle",) * 3, count_bytes=count_bytes)


WIDE = (65536 + 13107, 32771 + 19650, 65536 + 13000)  # with the two small sequences: the block maximum exactly


def wide_frame(q: Seq = WIDE, ok: bool = True) -> Frame:
    """The widest sequence: LL code 35, ML code 51 and the largest offset code the output allows (16), each with
    all its extra bits (16 + 15 + 16), in tables where each of these codes has one cell, whose state update
    reads the whole accuracy log: 9 + 9 + 8 bits behind the 47."""
    llw = [478] + [1] * 33 + [0, 1]
    ofw = [239] + [1] * 16 + [1]
    mlw = [461] + [1] * 51
    f = Frame(window=256 * KIB).raw(lits(100, 1))
    if not ok:
        f.refuse()
    assert (q[0] + q[1] == BLOCK_MAX + 1) == (not ok) and q[0] + 1 <= BLOCK_MAX
    return f.compressed(lits(q[0] + 1, 3), [q, (0, 3, 4), (1, 4, 1)],
                        modes=(("fse", llw, 9), ("fse", ofw, 8), ("fse", mlw, 9)), last=(widest,) * 3)


@functools.lru_cache(maxsize=None)
def sequences() -> List[Case]:
    """entropy, ``block_sequences`` / ``decode_sequences`` / ``table_setup`` on one lane: the count in 1, 2 and
    3 bytes, each table in each mode, FSE descriptions at the smallest and largest accuracy logs with -1
    probabilities, short values and zero runs, and the widest sequence the format holds, which makes
    ``BackwardBits`` refill in the middle of a sequence; execute's block-maximum check."""
    out = []
    for n in (127, 128, 0x7EFF, 0x7F00, 0x7F01):
        out.append(_rle3(n).case(f"sequences all tables RLE, {n} sequences"))
    out.append(_rle3(5, 2).case("sequences a count of 5 in two bytes"))
    # explicit distributions: -1 probabilities, values below the threshold (one bit shorter), zero runs 3,3,x
    ll5 = [8, 6, 0, 0, 0, 0, 0, 0, 0, 0, 5, 4, 3, 2, 1, 1, -1, -1]          # zeros behind symbol 2: flags 3, 3, 1
    ll9 = [300, 100, 50, 20, 10, 10, 5, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1]
    of5 = [0, 0, 10, 12, 6, 2, 1, -1]
    of8 = [0, 0, 100, 90, 40, 20, 1, 1, 1, 1, 1, -1]
    ml5 = [16, 8, 4, 1, 1, 1, -1]
    ml9 = [200, 150, 100, 30, 10, 5, 5, 5, 1, 1, 1, 1, 1, 1, -1]
    ends = set()
    for (ln, ll), (on, of), (mn, ml) in (((5, ll5), (5, of5), (5, ml5)), ((9, ll9), (8, of8), (9, ml9)),
                                         ((5, ll5), (8, of8), (5, ml5)), ((9, ll9), (5, of5), (9, ml9))):
        ends |= {fse_description(t, g)[1] % 8 == 0 for t, g in ((ll, ln), (of, on), (ml, mn))}
        fse = (("fse", ll, ln), ("fse", of, on), ("fse", ml, mn))
        for mix in ("fff", "frf", "rfr", "pfr", "fpf", "rrf", "ffp"):
            modes = tuple({"f": fse[k], "r": "rle", "p": "predefined"}[m] for k, m in enumerate(mix))
            f = Frame().raw(lits(40, ln + on))
            rng, seqs, have = Lcg(ln * on + len(out)), [], 40
            llc = [s for s, p in enumerate(ll) if p]
            mlc = [s for s, p in enumerate(ml) if p]
            ofc = [s for s, p in enumerate(of) if p]
            for i in range(60):
                q = (LL_BASE[10 if mix[0] == "r" else llc[(i * 3 + rng.below(2)) % len(llc)]],
                     ML_BASE[4 if mix[2] == "r" else mlc[(i + rng.below(3)) % len(mlc)]],
                     (1 << 3) + rng.below(8) if mix[1] == "r" else None)
                if q[2] is None:
                    code = ofc[(i + rng.below(2)) % len(ofc)]
                    while (1 << code) - 3 > have + q[0]:
                        code -= 1
                    code = max(code, min(ofc))
                    q = (q[0], q[1], (1 << code) + rng.below(min(1 << code, have + q[0] + 4 - (1 << code))))
                seqs.append(q)
                have += q[0] + q[1]
            f.compressed(lits(sum(q[0] for q in seqs), len(out)), seqs, modes=modes, last=(widest,) * 3)
            out.append(f.case(f"sequences logs {ln}/{on}/{mn}, modes {mix}"))
    assert ends == {True, False}, "descriptions that end on and off a byte boundary"
    for name, q, ok in (("the widest valid sequence", WIDE, True),
                        ("ll + ml one byte over the block maximum", (WIDE[0], WIDE[1] + 9, WIDE[2]), False)):
        out.append(wide_frame(q, ok).case("sequences " + name, ok=ok))
    # offset code 31 with all-ones extra bits: an offset of 4 GiB less 4, refused and not misread
    f = Frame().raw(lits(100, 2))
    f.refuse()
    f.compressed(lits(4, 1), [(2, 3, 0xFFFFFFFF)], modes=("predefined", "rle", "predefined"))
    out.append(f.case("sequences offset code 31, all extra bits set", ok=False))
    return out


def _edge(what, f: Frame, ok, out_n=None):
    return f.case("window_and_size " + what, ok=ok, out_n=out_n)


@functools.lru_cache(maxsize=None)
def window_and_size() -> List[Case]:
    """execute's checks (``off > op || off > fr.window``, ``len > fr.block_max - (op - start)``,
    ``len > out_n - op``, ``rest > ...``, ``r.size > out_n - op``) and index's ``size > fr.block_max``: each
    at its edge and one byte past it; and every frame header the format allows."""
    out = []
    # offset = window / window + 1 (a window of 1 KiB behind 2 KiB of output); offset = op / op + 1
    for d, ok in ((0, True), (1, False)):
        f = Frame(window=KIB).raw(lits(KIB, 1)).raw(lits(KIB, 2))
        if not ok:
            f.refuse()
        f.block([(lits(3, 3), 9, ov_of(KIB + d))], lits(2, 4))
        out.append(_edge(f"offset = window + {d}", f, ok))
        for n in (1, 7, 70):
            f = Frame().raw(lits(n, n))
            if not ok:
                f.refuse()
            f.block([(lits(2, 3), 9, ov_of(n + 2 + d))], lits(2, 4))
            out.append(_edge(f"offset = op + {d} = {n + 2 + d}", f, ok))
    f = Frame(window=256 * KIB).raw(lits(BLOCK_MAX, 1)).raw(lits(100, 2))
    f.block([(lits(3, 3), 40, ov_of(BLOCK_MAX + 50))], lits(2, 4))
    out.append(_edge("offset beyond 128 KiB", f, True))
    # Raw, RLE and Compressed blocks at the block maximum and one byte over it
    for d, ok in ((0, True), (1, False)):
        f = Frame(window=KIB).raw(lits(5, 1))
        if not ok:
            f.refuse()
        out.append(_edge(f"Raw block of block maximum + {d}", f.raw(lits(KIB + d, 2)), ok))
        f = Frame(window=KIB).raw(lits(5, 1))
        if not ok:
            f.refuse()
        out.append(_edge(f"RLE block of block maximum + {d}", f.rle(7, KIB + d), ok))
        f = Frame(window=KIB).raw(lits(5, 1))
        if not ok:
            f.refuse()
        out.append(_edge(f"a block's literals and match end at block maximum + {d}",
                         f.block([(lits(500, 2), KIB - 500 + d, ov_of(300))]), ok))
        f = Frame(window=KIB).raw(lits(5, 1))
        if not ok:
            f.refuse()
        out.append(_edge(f"a block's trailing literals end at block maximum + {d}",
                         f.block([(lits(100, 2), 500, ov_of(30))], lits(KIB - 600 + d, 3)), ok))
        f = Frame(single=True).raw(lits(5, 1))  # single segment: the window is the content size
        f.block([(lits(3, 2), 4, ov_of(8))], lits(2, 3))
        c = _edge(f"single segment, Frame_Content_Size - {d} offered", f, ok, out_n=f.nominal - d)
        out.append(c if ok else c._replace(want=b""))
    # without a content size: one byte too few, exact, one too many, on each store path
    paths = {
        "literals": lambda f: f.block([(lits(9, 1), 4, ov_of(3)), (lits(300, 2), 3, ov_of(2))]),
        "match": lambda f: f.block([(lits(9, 1), 300, ov_of(3))]),
        "overlapped match of 3": lambda f: f.block([(lits(9, 1), 3, ov_of(1))]),
        "trailing literals": lambda f: f.block([(lits(9, 1), 4, ov_of(3))], lits(300, 3)),
        "Raw": lambda f: f.raw(lits(300, 4)),
        "RLE": lambda f: f.rle(0x21, 300),
    }
    for name, put in paths.items():
        for d in (-1, 0, 1):
            f = Frame().raw(lits(20, 1)).block([(lits(4, 1), 5, ov_of(7))], lits(1, 2))
            if d < 0:
                f.refuse()
            put(f)
            out.append(_edge(f"no content size, {name} last, {d:+d} offered", f, d == 0, out_n=f.nominal + d))
    # frame headers
    small = lambda f: f.raw(lits(20, 1)).block([(lits(4, 1), 5, ov_of(7))], lits(1, 2))  # noqa: E731
    for fcs in (1, 2, 4, 8):
        f = Frame(single=True, fcs_bytes=fcs)
        small(f)
        if fcs == 2:
            f.rle(3, 300)
        out.append(_edge(f"single segment, content size in {fcs} bytes", f, True))
    for fcs in (0, 2, 4, 8):
        for did in (0, 1, 2, 4):
            f = Frame(fcs_bytes=fcs, did_bytes=did, checksum=(fcs + did) % 3 == 0)
            small(f)
            if fcs == 2:
                f.rle(3, 300)
            out.append(_edge(f"windowed, content size in {fcs} bytes, Dictionary_ID in {did}, "
                             f"checksum {f.checksum}", f, True))
    for need in (KIB + 1, 5 * KIB, 7 * KIB + 1, 200 * KIB):  # exponents and mantissas
        f = Frame(window=need)
        small(f)
        out.append(_edge(f"window descriptor {window_descriptor(need)[0]:#04x}", f, True))
    f = Frame(fcs_bytes=4)
    small(f)
    out.append(f.case("window_and_size content size differs from the size offered", ok=False, out_n=f.nominal + 1)
               ._replace(want=b""))
    return out


FAMILIES = {"overlap": overlap, "apart": apart, "batches_of_64": batches_of_64, "watermark": watermark,
            "repeat_offsets": repeat_offsets, "chains": chains, "isolation": isolation, "literals": literals,
            "sequences": sequences, "window_and_size": window_and_size}


def all_cases() -> List[Case]:
    return [c for make in FAMILIES.values() for c in make()]
