"""An independent reader of the LZ4 block format in pure Python, for the tests only.

Written from the format's description (a block is a series of sequences: token, literal-length bytes,
literals, 2-byte little-endian offset, match-length bytes; the last sequence ends after its literals): it
shares no code with the kernels (dwarfs_amd/csrc/lz4_kernels.hip) or with the host restatement
(dwarfs_amd/csrc/lz4_host.cpp) and imports neither.  It plays the role tests/flac_ref.py plays for FLAC.

``walk`` parses a block into its sequences without producing bytes, ``decode`` produces them, and
``check_end_rules`` states the three rules LZ4_decompress_safe holds an encoder to.
"""

from __future__ import annotations

from typing import List, NamedTuple, Optional


class Lz4Error(ValueError):
    """The block breaks the format, or does not produce the stated size."""


class Sequence(NamedTuple):
    literals: int          # literal bytes of the sequence
    literal_at: int        # where they start in the block
    offset: Optional[int]  # None: the last sequence, which has no match
    match: int             # match bytes (0 for the last sequence)
    out_at: int            # output position of the sequence's first literal


def _length(block: bytes, at: int, nibble: int):
    """A nibble's value with its extension bytes: (value, position behind them)."""
    value = nibble
    if nibble == 15:
        while True:
            if at >= len(block):
                raise Lz4Error("length byte past the end of the block")
            byte = block[at]
            at += 1
            value += byte
            if byte != 255:
                break
    return value, at


def walk(block: bytes) -> List[Sequence]:
    """The sequences of a block; raises Lz4Error where the block cannot be parsed.  Offsets are checked for 0
    only: whether they reach before the output's start is for ``decode``, which knows what was produced."""
    block = bytes(block)
    seqs: List[Sequence] = []
    at = produced = 0
    while True:
        if at >= len(block):
            raise Lz4Error("token past the end of the block")
        token = block[at]
        literals, at = _length(block, at + 1, token >> 4)
        if literals > len(block) - at:
            raise Lz4Error("literals past the end of the block")
        literal_at = at
        at += literals
        if at == len(block):
            seqs.append(Sequence(literals, literal_at, None, 0, produced))
            return seqs
        if len(block) - at < 2:
            raise Lz4Error("offset past the end of the block")
        offset = block[at] | block[at + 1] << 8
        if offset == 0:
            raise Lz4Error("offset 0")
        match, at = _length(block, at + 2, token & 15)
        match += 4
        seqs.append(Sequence(literals, literal_at, offset, match, produced))
        produced += literals + match


def decode(block: bytes, size: int) -> bytes:
    """The ``size`` bytes the block stands for; Lz4Error if it is malformed, would produce more, or produces
    fewer."""
    block = bytes(block)
    out = bytearray()
    for s in walk_lenient(block):
        if isinstance(s, Lz4Error):
            raise s
        if len(out) + s.literals > size:
            raise Lz4Error("literals past the stated size")
        out += block[s.literal_at:s.literal_at + s.literals]
        if s.offset is None:
            break
        if s.offset > len(out):
            raise Lz4Error("offset before the start of the output")
        if len(out) + s.match > size:
            raise Lz4Error("match past the stated size")
        if s.offset >= s.match:
            out += out[len(out) - s.offset:len(out) - s.offset + s.match]
        else:  # the match overlaps its destination: a pattern of `offset` bytes repeated
            pattern = bytes(out[len(out) - s.offset:])
            out += (pattern * (s.match // s.offset + 1))[:s.match]
    if len(out) != size:
        raise Lz4Error(f"the block produced {len(out)} bytes, not {size}")
    return bytes(out)


def walk_lenient(block: bytes):
    """``walk`` sequence by sequence, in decoding order: a parse error is yielded where the parse reaches it,
    so that ``decode`` reports the first thing that goes wrong in a block with more than one fault."""
    at = produced = 0
    while True:
        try:
            if at >= len(block):
                raise Lz4Error("token past the end of the block")
            token = block[at]
            literals, at = _length(block, at + 1, token >> 4)
            if literals > len(block) - at:
                raise Lz4Error("literals past the end of the block")
        except Lz4Error as e:
            yield e
            return
        literal_at = at
        at += literals
        if at == len(block):
            yield Sequence(literals, literal_at, None, 0, produced)
            return
        if len(block) - at < 2:
            yield Lz4Error("offset past the end of the block")
            return
        offset = block[at] | block[at + 1] << 8
        try:
            if offset == 0:
                raise Lz4Error("offset 0")
            match, at = _length(block, at + 2, token & 15)
        except Lz4Error as e:
            yield e
            return
        yield Sequence(literals, literal_at, offset, match + 4, produced)
        produced += literals + match + 4


def check_end_rules(block: bytes, size: int) -> None:
    """The rules an encoder keeps because LZ4_decompress_safe enforces them: the last 5 bytes of the output
    are literals, the last match starts at least 12 bytes before the end, and so an input below 13 bytes is
    one literal run.  AssertionError names the rule that is broken."""
    seqs = walk(block)
    last = seqs[-1]
    assert last.offset is None
    assert last.out_at + last.literals == size, "the sequences do not add up to the stated size"
    matches = [s for s in seqs if s.offset is not None]
    if size < 13:
        assert not matches, "an input below 13 bytes must be one literal run"
    if matches:
        assert last.literals >= 5, f"the last {last.literals} bytes are literals, fewer than 5"
        start = matches[-1].out_at + matches[-1].literals
        assert start + 12 <= size, f"the last match starts {size - start} bytes before the end, fewer than 12"
    for s in matches:
        assert 1 <= s.offset <= 65535 and s.offset <= s.out_at + s.literals
