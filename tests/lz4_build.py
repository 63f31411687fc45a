"""A writer of LZ4 blocks from sequence lists, and the constructed-block families of the LZ4 tests.

Pure Python, for the tests only: it imports neither the package nor tests/lz4_ref.py.  ``build`` writes a block
from ``(literal_bytes, offset, match_len)`` triples and a last literal run, ``expand`` states what such a list
stands for by the obvious byte-at-a-time loop (the expected output of every decoder), ``layout`` says where each
field of each sequence lies in the block, and ``lead`` / ``place`` pad with leading sequences so that a chosen
field lands at a chosen byte position.  ``window_trace`` and the ``W`` of ``watermark`` restate two rules of the
decode kernel (dwarfs_amd/csrc/lz4_kernels.hip: its 64-byte register window, and the watermark of its header
comment); they are used to aim the cases and to count what the families reach, never to compute an expected
byte.

The families (``overlap``, ``apart``, ``literals``, ``window_edges``, ``watermark``, ``output_size``,
``batch_shape``) return lists of :class:`Case`; ``encoder_inputs`` returns the inputs aimed at the encoder.
"""

from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Sequence, Tuple

FILL = 0xA5  # what the tests fill output buffers with: the watermark family's literals avoid it
Seq = Tuple[bytes, int, int]  # (literal bytes, offset, match length)


class Case(NamedTuple):
    what: str            # the parameters, for the assertion message
    block: bytes
    out_n: int           # the output size the decoder is offered
    want: bytes          # the bytes a decoder leaves at the output's start (all out_n of them where ok)
    ok: bool             # the decode contract accepts the block at this size (RPP_OK), else RPP_CORRUPT_INPUT
    end_rules: bool      # the block keeps the end-of-block rules, so liblz4 accepts it too where ok
    out_mis: Optional[int] = None  # wanted misalignment mod 4 of the output's first byte (None: any)


class Fields(NamedTuple):
    """Block byte positions of one sequence's fields (an absent extension has the position it would have)."""
    token: int
    lit_ext: int
    literals: int
    offset: int     # -1 for the last literal run
    match_ext: int  # -1 for the last literal run
    end: int


class Lcg:
    """A small deterministic generator (no numpy here)."""

    def __init__(self, seed: int):
        self.x = (seed * 2654435761 + 12345) & 0xFFFFFFFF

    def next(self) -> int:
        self.x = (self.x * 1103515245 + 12345) & 0xFFFFFFFF
        return self.x >> 16

    def below(self, n: int) -> int:
        return self.next() % n

    def noise(self, n: int) -> bytes:
        """n bytes in 1..255 (never 0, so that a run of zeros ends where noise begins)"""
        return bytes(1 + self.next() % 255 for _ in range(n))


def lits(n: int, salt: int = 0, avoid: Optional[int] = None) -> bytes:
    """n bytes, any 256 in a row from the start all distinct (131 is odd), differing with ``salt``."""
    out = bytearray((salt * 29 + 1 + i * 131 + (i >> 8) * 7) & 255 for i in range(n))
    if avoid is not None:
        out = out.replace(bytes([avoid]), bytes([avoid ^ 0xFF]))
    return bytes(out)


def length_ext(v: int) -> bytes:
    """The extension bytes behind a token nibble that stands for v: none below 15, else 255s and the rest."""
    if v < 15:
        return b""
    return b"\xff" * ((v - 15) // 255) + bytes([(v - 15) % 255])


def build(sequences: Sequence[Seq], tail: bytes, end_rules: bool = True) -> bytes:
    """The block: per sequence token, literal-length bytes, literals, little-endian offset, match-length bytes;
    then the last literal run.  With ``end_rules`` (the default) a block with a match must end in at least 12
    literals, which is more than LZ4_decompress_safe asks (last 5 bytes literals, last match 12 before the
    end)."""
    out = bytearray()
    for lit, off, mlen in sequences:
        assert mlen >= 4 and 0 < off <= 65535, (off, mlen)
        out.append(min(len(lit), 15) << 4 | min(mlen - 4, 15))
        out += length_ext(len(lit)) + bytes(lit) + bytes([off & 255, off >> 8]) + length_ext(mlen - 4)
    assert not end_rules or not sequences or len(tail) >= 12, "a block that keeps the end rules ends in 12 literals"
    out.append(min(len(tail), 15) << 4)
    out += length_ext(len(tail)) + bytes(tail)
    return bytes(out)


def expand(sequences: Sequence[Seq], tail: bytes = b"") -> bytes:
    """What the sequences stand for, one byte at a time."""
    out = bytearray()
    for lit, off, mlen in sequences:
        out += lit
        if off > len(out):
            raise ValueError(f"offset {off} with {len(out)} bytes produced")
        for _ in range(mlen):
            out.append(out[len(out) - off])
    return bytes(out + tail)


def layout(sequences: Sequence[Seq], tail: bytes = b"") -> List[Fields]:
    """Where the fields of every sequence, and of the last literal run, lie in ``build``'s block."""
    out, at = [], 0
    for lit, _, mlen in sequences:
        lit_at = at + 1 + len(length_ext(len(lit)))
        off_at = lit_at + len(lit)
        end = off_at + 2 + len(length_ext(mlen - 4))
        out.append(Fields(at, at + 1, lit_at, off_at, off_at + 2, end))
        at = end
    lit_at = at + 1 + len(length_ext(len(tail)))
    out.append(Fields(at, at + 1, lit_at, -1, -1, lit_at + len(tail)))
    return out


def lead(total: int, salt: int = 0) -> List[Seq]:
    """Leading sequences that take exactly ``total`` bytes of the block (0, or 4 and more): one run of
    literals with a match of 4 at offset 1, and zero-literal matches where a length byte leaves a gap."""
    if total == 0:
        return []
    for extra in range(3):
        t = total - 3 * extra
        for e in range(t // 255 + 2):
            n = t - 3 - e
            if n >= 1 and len(length_ext(n)) == e:
                return [(lits(n, salt), 1, 4)] + [(b"", 1, 4)] * extra
    raise ValueError(f"no leading sequences of {total} bytes")


def place(seq: Seq, field: str, position: int, before: Sequence[Seq] = (), salt: int = 0) -> List[Seq]:
    """``before``, padding, then ``seq`` with its ``field`` (a name of :class:`Fields`) at block byte
    ``position``."""
    used = layout(before)[-1].token if before else 0
    rel = getattr(layout([seq])[0], field)
    seqs = list(before) + lead(position - rel - used, salt) + [seq]
    assert getattr(layout(seqs)[len(seqs) - 1], field) == position
    return seqs


def window_trace(block: bytes):
    """The decode kernel's register window over a valid block: per sequence ``(lit, lit_rel, off_rel)``: the
    literal count, where the run starts relative to the window when it is copied (None: no window yet covers
    it), and where the offset's low byte is read relative to the window in force before that read (None for
    the last run).  A window is 64 bytes from the position of the peek that loaded it; literals load none."""
    win = None
    at = 0

    def peek(ip):
        nonlocal win
        if win is None or not win <= ip < win + 64:
            win = ip
        return block[ip]

    out = []
    while True:
        token = peek(at)
        at += 1
        lit = token >> 4
        if lit == 15:
            while True:
                x = peek(at)
                at += 1
                lit += x
                if x != 255:
                    break
        lit_rel = at - win if at >= win else None
        at += lit
        if at == len(block):
            out.append((lit, lit_rel, None))
            return out
        off_rel = at - win if win <= at < win + 64 else None
        peek(at)
        peek(at + 1)
        at += 2
        if token & 15 == 15:
            while peek(at) == 255:
                at += 1
            at += 1
        out.append((lit, lit_rel, off_rel))


def case(what: str, sequences: Sequence[Seq], tail: bytes, out_mis: Optional[int] = None) -> Case:
    want = expand(sequences, tail)
    return Case(what, build(sequences, tail), len(want), want, True, True, out_mis)


TAIL = lits(12, 77)

OVERLAP_OFFSETS = list(range(1, 131)) + [191, 192, 193, 255, 256, 257]
OVERLAP_LENGTHS = [4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]


def overlap() -> List[Case]:
    """A pattern of ``off`` bytes (all distinct up to 256) repeated by one match, the match's first output byte
    at every misalignment mod 4.  Lengths up to the offset take the apart path; the others the overlapped one,
    with one to five turns per lane."""
    out = []
    for off in OVERLAP_OFFSETS:
        for n in OVERLAP_LENGTHS:
            for m in range(4):
                pad = (m - off) % 4
                out.append(case(f"overlap off={off} len={n} op%4={m}", [(lits(pad, n) + lits(off, off), off, n)], TAIL,
                                out_mis=0))
    return out


APART_LENGTHS = [4, 255, 256, 257, 259, 260, 511, 512, 513, 1023]
APART_GAPS = [0, 1, 3]


def apart() -> List[Case]:
    """One match whose source ends ``gap`` bytes before its destination, the destination at every misalignment
    mod 4.  The source's misalignment follows from the three: ``apart_alignments`` lists the pairs, and over
    the family all 16 occur."""
    out = []
    for n in APART_LENGTHS:
        for gap in APART_GAPS:
            for d in range(4):
                off = n + gap
                pad = (d - off) % 4
                out.append(case(f"apart len={n} off-len={gap} src%4={pad} dst%4={d}", [(lits(pad + off, n), off, n)],
                                TAIL, out_mis=0))
    return out


def apart_alignments():
    return {((d - n - gap) % 4, d) for n in APART_LENGTHS for gap in APART_GAPS for d in range(4)}


LITERAL_RUNS = [0, 1, 14, 15, 16, 63, 64, 65, 255, 256, 257, 269, 270, 271, 512 + 3]


def literals() -> List[Case]:
    """A literal run of every listed length starting at block byte ``p`` (mod 64) for every p: behind short
    leading sequences, so the window still starts at byte 0 when the run begins below 64, and the run is
    stored from the window or by the wide copy as ``p + length`` falls on either side of 64."""
    out = []
    for n in LITERAL_RUNS:
        for p in range(64):
            seq = (lits(n, p), 1, 4)
            rel = layout([seq])[0].literals
            at = p
            while at - rel in (1, 2, 3) or at < rel or (at == rel and n == 0):  # (no match without a byte before it)
                at += 64
            out.append(case(f"literals run={n} at byte {at}", place(seq, "literals", at, salt=n), TAIL))
    return out


EDGE_TOKENS = [62, 63, 64, 65]
EDGE_RUNS = [1, 2, 63, 64, 65, 130]  # bytes of 255 in a length's extension


def window_edges() -> List[Case]:
    """Tokens, length extensions and offsets at chosen places relative to the 64-byte window."""
    out = []
    for at in EDGE_TOKENS:
        out.append(case(f"edge token at {at}", place((lits(3, at), 2, 6), "token", at), TAIL))
    for k in EDGE_RUNS:
        for at in [0] + EDGE_TOKENS:  # the extension follows the token: it crosses k // 64 or k // 64 + 1 reloads
            n = 15 + 255 * k + 7 * (at % 5)
            assert length_ext(n)[:-1] == b"\xff" * k
            out.append(case(f"edge literal extension of {k} x 255, token at {at}",
                            place((lits(n, k), 3, 9), "token", at, salt=k), TAIL))
        for at in [11] + EDGE_TOKENS:
            n = 4 + 15 + 255 * k + 11 * (at % 5)
            out.append(case(f"edge match extension of {k} x 255 at {at}, overlapped",
                            place((lits(8, k), 7, n), "match_ext", at, salt=k), TAIL))
            if k <= 2:  # the same with the source apart (the literals before it are as long as the match)
                seq = (lits(n, k), n, n)
                first = layout([seq])[0].match_ext + 4
                out.append(case(f"edge match extension of {k} x 255 at {first + at}, apart",
                                place(seq, "match_ext", first + at, salt=k), TAIL))
    # an offset of two different non-zero bytes, split across a reload: at (63, 64) and, with a token at 64 so
    # that the second window starts there, at (127, 128); 300 bytes are produced first so that 0x0105 is valid
    start = [(lits(16, 5), 16, 300)]
    for lo_at, before in ((63, start), (127, start + lead(64 - layout(start)[-1].token, 9))):
        for off in (0x0105, 0x0033):
            out.append(case(f"edge offset {off:#06x} at ({lo_at}, {lo_at + 1})",
                            place((lits(3, off), off, 20), "offset", lo_at, before, salt=off & 255), TAIL))
    return out


WATERMARK_KINDS = ["ends_at_W", "ends_at_W_plus_1", "starts_at_W_minus_1", "in_previous_sequence"]


def _chain(kind: str, n: int, nlit: int, alternate: bool, seed: int):
    """A head sequence (24 literals and a match, after which W = 24) and n more with ``nlit`` literals each.
    The match of each of those is placed by ``kind`` relative to W, the watermark (``alternate``: every second
    one, the others in_previous_sequence, so that W keeps moving).  W follows the rule of the kernel's header
    comment: a match whose source reaches past W waits for the wave's stores, and W becomes the output
    position at which that match starts.  Returns (sequences, [(kind, source start, source end, W before)])."""
    rng = Lcg(seed)
    seqs: List[Seq] = [(lits(24, seed, FILL), 9, 6)]
    placed = []
    W = 24                             # the head's match reads [15, 21) with W = 0: it waits at op = 24
    op, prev_start, pm_start, pm_len = 30, 0, 24, 6
    for j in range(1, n + 1):
        lit = lits(nlit, seed + j, FILL)
        at = op + nlit                 # where this match's output starts
        k = kind if not alternate or j % 2 else "in_previous_sequence"
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
        else:                          # copies_previous_match (overlapped where it is longer than what is there)
            m = 4 + rng.below(13)
            s = pm_start + rng.below(pm_len)
        off = at - s
        span = min(m, off)
        placed.append((k, s, s + span, W))
        seqs.append((lit, off, m))
        if s + span > W:
            W = at
        prev_start, pm_start, pm_len, op = op, at, m, at + m
    return seqs, placed


@functools.lru_cache(maxsize=None)
def watermark_chains():
    """[(what, sequences, placements)] of the watermark family: every kind, alone and alternating, in chains
    of 2..40 sequences with 0..3 literals each; then the chains in which every match copies the output of the
    match before it."""
    out = []
    for ki, kind in enumerate(WATERMARK_KINDS + ["copies_previous_match"]):
        for alternate in (False, True):
            if alternate and kind in ("in_previous_sequence", "copies_previous_match"):
                continue
            for n in range(2, 41):
                for nlit in range(4):
                    what = f"watermark {kind}{' alternating' if alternate else ''} chain={n} literals={nlit}"
                    out.append((what, *_chain(kind, n, nlit, alternate, 1000 * ki + 500 * alternate + 4 * n + nlit)))
    return out


@functools.lru_cache(maxsize=None)
def watermark() -> List[Case]:
    return [case(what, seqs, lits(12, len(seqs), FILL)) for what, seqs, _ in watermark_chains()]


@functools.lru_cache(maxsize=None)
def output_size() -> List[Case]:
    """Per store path a block offered one byte too few, the exact size and one too many; the two blocks that
    end in a match and an empty last run keep the decode contract but not the end rules.  Then the smallest
    blocks, and an offset that reaches the output's first byte, or one before it."""
    out = []
    paths = [
        ("window literals last", [(lits(20, 1), 5, 8)], TAIL, True),
        ("wide-copy literals last", [(lits(20, 2), 5, 8)], lits(300, 3), True),
        ("wide-copy match, then 12 literals", [(lits(310, 4), 305, 300)], TAIL, True),
        ("overlapped match, then 12 literals", [(lits(10, 5), 3, 100)], TAIL, True),
        ("wide-copy match last", [(lits(310, 6), 305, 300)], b"", False),
        ("overlapped match last", [(lits(10, 7), 3, 100)], b"", False),
    ]
    for what, seqs, tail, rules in paths:
        block, full = build(seqs, tail, end_rules=rules), expand(seqs, tail)
        # what is stored before the check that refuses a size one short: everything but the last store
        before = expand(seqs) if tail else expand(seqs[:-1]) + seqs[-1][0]
        out.append(Case(f"size {what}, one short", block, len(full) - 1, before, False, rules))
        out.append(Case(f"size {what}, exact", block, len(full), full, True, rules))
        out.append(Case(f"size {what}, one long", block, len(full) + 1, full, False, rules))
    short = [(lits(9, 8), 9, 4), (lits(30, 9), 2, 4)]  # one short at the second sequence's literals
    out.append(Case("size literals of a middle sequence, short by its match", build(short, b"", False),
                    len(expand(short)) - 5, expand(short[:1]), False, False))
    out.append(Case("size in_n = 0, out_n = 0", b"", 0, b"", False, True))
    out.append(Case("size in_n = 0, out_n = 5", b"", 5, b"", False, True))
    out.append(Case("size lone 0x00 token, out_n = 0", b"\x00", 0, b"", True, True))
    out.append(Case("size lone 0x00 token, out_n = 1", b"\x00", 1, b"", False, True))
    for n in (1, 7, 70):
        first = lits(n, n)
        out.append(case(f"size offset = op = {n}", [(first, n, 9)], TAIL))
        bad = build([(first, n + 1, 9)], TAIL)
        out.append(Case(f"size offset = op + 1 = {n + 1}", bad, n + 9 + 12, first, False, True))
    return out


def batch_shape() -> List[Case]:
    """Nine mixed blocks, sent as batches of several sizes."""
    by_what = {c.what: c for c in output_size()}
    return [
        case("batch overlap", [(lits(7, 1), 7, 300)], TAIL),
        case("batch apart", [(lits(515, 2), 513, 513)], TAIL),
        by_what["size lone 0x00 token, out_n = 0"],
        case("batch literals only", [], lits(515, 3)),
        watermark()[155],
        by_what["size offset = op + 1 = 8"],
        case("batch one byte", [], b"\x42"),
        watermark()[-1],
        by_what["size overlapped match last, one short"],
    ]


DECODE_FAMILIES = {"overlap": overlap, "apart": apart, "literals": literals, "window_edges": window_edges,
                   "watermark": watermark, "output_size": output_size, "batch_shape": batch_shape}

SENTENCE = b"Pack my box with five dozen liquor jugs, then weigh the archive once more. "
PLANT_LENGTHS = [4 + 64 * k + d for k in (0, 1, 2, 5) for d in (-1, 0, 1)]


def encoder_inputs(chunk: int, step: int) -> List[Tuple[str, bytes]]:
    """[(name, input)] aimed at the encoder's search (``chunk`` and ``step`` are its two constants):
    period-p patterns (many positions of a step share a table slot), every length 0..80, a planted repeat of
    4 + 64k + d bytes ended by a differing byte, by the chunk's end and by the last 5 literals, and a long
    match that skips whole steps with another repeat right behind it."""
    out = []
    for p in range(1, 71):
        out.append((f"period_{p}", (lits(p, p) * (3 * step // p + 8))[:3 * step + 7]))
    for n in range(81):
        out.append((f"sentence_{n}", (SENTENCE * 2)[:n]))
        out.append((f"period3_{n}", (b"xyz" * 27)[:n]))
    for m in PLANT_LENGTHS:
        rng = Lcg(m)
        piece, a, gap, end = rng.noise(m + 40), rng.noise(step + 6), rng.noise(step + 6), rng.noise(20)
        other = bytes([piece[m] ^ 0x55 or 1])
        out.append((f"plant_{m}_differing_byte", a + piece + gap + piece[:m] + other + end))
        out.append((f"plant_{m}_last_literals", a + piece + gap + piece[:m + 5]))
        # zeros up to the repeat: one long match, whose steps are skipped whole, so the piece's table entries last
        zeros = bytes(chunk - m - len(a) - len(piece))
        out.append((f"plant_{m}_chunk_end", a + piece + zeros + piece + end))
    rng = Lcg(99)
    a, b, gap = rng.noise(40), rng.noise(3 * step + 9), rng.noise(step)
    out.append(("skip_steps_then_repeat", a + b + gap + b + a + rng.noise(20)))
    out.append(("skip_steps_zeros_then_repeat", a + bytes(5 * step + 3) + a + rng.noise(20)))
    return out
