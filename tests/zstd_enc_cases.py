"""The Zstandard encoder's inputs, shared by the CPU and the GPU tests: every input of the LZ4 encoder's tests
(the match search is the same), then inputs aimed at the entropy stage, built from seeds with make_lz4_kat's
generators.  The aimed inputs are at most 2 * chunk + 1 bytes, but for the two sizes around 65792 that the 4-byte
Frame_Content_Size needs and the one that reaches the largest offset.  Where a count (literals, sequences) has to be hit exactly, the input is tuned against
the host encoder's own frame, which ``sections`` parses."""

import functools
from typing import List, NamedTuple, Optional

import lz4_cases as LC
import zstd_ref as R
from dwarfs_amd import zstd as Z

K = LC.K
CHUNK = 32768


class Section(NamedTuple):
    """What the headers of one block say."""
    block: int                  # 0 Raw, 2 Compressed
    literals: Optional[int]     # 0 Raw, 1 RLE, 2 Compressed
    size_format: Optional[int]  # the header's Size_Format bits (Raw and RLE: 0 and 2 are the 1-byte header)
    header_bytes: Optional[int]
    regenerated: Optional[int]
    streams: Optional[int]
    weights: Optional[str]      # "direct" or "fse"
    sequences: Optional[int]
    count_bytes: Optional[int]


def sections(frame: bytes) -> List[Section]:
    out = []
    for kind, size, at, _ in R.block_headers(frame):
        if kind != 2:
            out.append(Section(kind, *[None] * 8))
            continue
        b = frame[at:at + size]
        lk, sf = b[0] & 3, b[0] >> 2 & 3
        weights = None
        if lk < 2:
            hb = 2 if sf == 1 else 3 if sf == 3 else 1
            v = int.from_bytes(b[:hb], "little")
            regen, streams = v >> (3 if hb == 1 else 4), 0
            held = regen if lk == 0 else 1
        else:
            hb, nb = (3, 10) if sf < 2 else (sf + 2, 4 + 5 * sf)
            v = int.from_bytes(b[:hb], "little") >> 4
            regen, held, streams = v & ((1 << nb) - 1), v >> nb, 1 if sf == 0 else 4
            weights = "direct" if b[hb] >= 128 else "fse"
        q = b[hb + held:]
        if q[0] < 128:
            nseq, cb = q[0], 1
        else:
            assert q[0] < 255
            nseq, cb = ((q[0] - 128) << 8) + q[1], 2
        out.append(Section(kind, lk, sf, hb, regen, streams, weights, nseq, cb))
    return out


def skewed(seed: int, n: int, mask: int = 255) -> bytes:
    """Bytes over the whole range (or below mask + 1) with unequal frequencies: the AND of two uniform draws."""
    a, b = K.rnd(seed, n), K.rnd(seed + 1000, n)
    return bytes(x & y & mask for x, y in zip(a, b))


def _tuned(make, measure, target: int, start: int) -> bytes:
    """make(k) for the k at which measure(sections of its frame) == target, found from `start` by correction."""
    k = start
    for _ in range(40):
        data = make(k)
        got = measure(sections(Z.host_encode(data)[0]))
        if got == target:
            return data
        k += target - got
    raise AssertionError(f"no input with a count of {target}")


def _literals_input(target: int, raw: bool) -> bytes:
    """A second chunk with exactly `target` literals (a first chunk of zeros before it, since no match starts in
    a block's first search step): k unmatched bytes (skewed, or uniform for Raw literals), then 64 random bytes
    41 times, which match from their second copy on, one search step behind the first (below 200 literals:
    zeros, which match the first chunk's).  A byte more is a literal more, but for what the search finds inside
    the k bytes, which the correction makes up for."""
    seed = 4000 + target + (500 if raw else 0)
    draw = K.rnd if raw else skewed
    piece = K.rnd(seed + 2000, 64)
    tail, first = (bytes(3000), target - 5) if target < 200 else (piece * 41, target - 69)
    return _tuned(lambda k: bytes(CHUNK) + draw(seed, max(k, 0)) + tail, lambda s: s[1].regenerated, target, first)


def _sequences_input(target: int) -> bytes:
    """`abcd` again and again, each time behind one byte that differs: a 4-byte match per 5 bytes."""
    tail = K.rnd(4300, 16)
    make = lambda k: b"".join(b"abcd" + bytes([i * 7 % 251]) for i in range(k)) + tail  # noqa: E731
    return _tuned(make, lambda s: s[0].sequences, target, target + 16)


@functools.lru_cache(maxsize=None)
def inputs():
    """[(name, input)]"""
    out = list(LC.encoder_inputs())
    out.append(("below_16_3000", K.rnd(4001, 3000, 16)))            # a small alphabet: direct weights
    out.append(("below_128_text", skewed(4002, 6000, 127)))         # text-like bytes below 128
    out.append(("skewed_full_range", skewed(4003, 20000)))          # FSE-compressed weights
    out.append(("two_symbols", K.rnd(4004, 5000, 2)))
    out.append(("one_byte_200", b"\x41" * 200))                     # RLE literals
    out.append(("random_5000", K.rnd(4005, 5000)))                  # Raw literals, then a Raw block
    out.append(("no_sequences_compressible", skewed(4006, 2500)))   # no match, Huffman literals win
    # every byte equally often and no match: all code lengths 8, 255 equal weights, which neither description states
    out.append(("permutations_512", b"".join(bytes(sorted(range(256), key=lambda v, s=s: K.rnd(4100 + s, 256, 256)[v] * 256 + v))
                                             for s in range(2))))
    for t in (31, 32, 1023, 1024, 4095, 4096, 16383, 16384):
        out.append((f"literals_{t}", _literals_input(t, False)))
    for t in (31, 32, 4095, 4096):
        out.append((f"raw_literals_{t}", _literals_input(t, True)))
    for t in (127, 128):
        out.append((f"sequences_{t}", _sequences_input(t)))
    out.append(("abcd_chunk", b"".join(b"abcd" + bytes([i * 7 % 251]) for i in range(CHUNK // 5)) + K.rnd(4301, 3)))
    # The largest offset the search can give is 65532: a chunk's table starts with the positions of the chunk
    # before it, and a match starts at least 4 bytes before its chunk's end.  Its offset value 65535 is the
    # largest of offset code 15; code 16 (offsets from 65533) cannot occur, and LZ4's offset_65535 finds no match.
    piece = K.rnd(4400, 32)
    out.append(("offset_65532", piece + bytes(65532 - 32) + piece + K.rnd(4401, 16)))
    for period in (1, 2, 3):  # a match one search step behind the block's start, at the offset of the period
        out.append((f"period_{period}", (b"xyz"[:period] * 200)[:200 + period]))
    out.append(("long_literals_long_match", K.rnd(4007, 20000) + bytes(12000)))
    for n in (255, 256, 65791, 65792):  # around the Frame_Content_Size widths (0 and 1: empty, single_byte)
        out.append((f"size_{n}", K.input_bytes({"kind": "sentence", "length": n})))
    return out
