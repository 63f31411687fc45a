"""The inputs of the Zstandard encoder's options tests (per-block table modes, repeat offsets), shared by the CPU
and the GPU tests: every input of tests/zstd_enc_cases.py, then families aimed at the two options.  The match
search is the LZ4 encoder's, so an input can only invite a sequence; what the search made of it is read back from
the frame with ``blocks`` and asserted in tests/test_zstd_encode_adaptive_host.py."""

import functools
import struct
from typing import List, NamedTuple, Tuple

import zstd_enc_cases as EC
import zstd_ref as R

K = EC.K
CHUNK = EC.CHUNK
OPTIONS = (1, 2, 3)
LOG_STEP = 64  # own_table_log: 5 up to this many sequences (and up to 16 codes seen), 6 above


class Block(NamedTuple):
    """A Compressed block's sequences section as the reader sees it (a Raw block: kind 0 and nothing else)."""
    kind: int
    modes: int                              # the modes byte; None without sequences
    sequences: List[Tuple[int, int, int]]   # (literal length, match length, offset value)
    tables: tuple                           # per table (LL, OF, ML): (accuracy log, {code: probability}) as described


def blocks(frame: bytes) -> List[Block]:
    out, st = [], R.State()
    for kind, size, at, _ in R.block_headers(frame):
        if kind != 2:
            out.append(Block(kind, None, [], ()))
            continue
        body = frame[at:at + size]
        _, used, _ = R.literals_section(body, st, None)
        sec = body[used:]
        seqs = R.sequences_section(sec, st, None)
        modes, tables = None, ()
        if seqs:
            p = 1 if sec[0] < 128 else 2
            modes, p = sec[p], p + 1
            tables = []
            for k, (_, _, max_log, max_symbol) in enumerate(R.TABLES):
                mode = modes >> (6 - 2 * k) & 3
                if mode == 1:
                    tables.append((0, {sec[p]: 1}))
                    p += 1
                elif mode == 2:
                    freq, log, n = R.fse_read_description(sec[p:], max_log, max_symbol)
                    tables.append((log, {s: f for s, f in enumerate(freq) if f}))
                    p += n
                else:
                    tables.append(None)
            tables = tuple(tables)
        out.append(Block(kind, modes, seqs, tables))
    return out


def records(seed: int, count: int, stride: int = 32) -> bytes:
    """Fixed-stride records: `stride` - 4 bytes that stay, then a 4-byte field that changes: a match at the
    stride per record, literals between them (R1 runs)."""
    base = K.rnd(seed, stride - 4)
    return b"".join(base + struct.pack("<I", (i + 1) * 2654435761 & 0xFFFFFFFF) for i in range(count))


def interleaved(seed: int, count: int, a: int, b: int, piece: int, gap: int) -> bytes:
    """Pieces of `piece` bytes copied in turn from `a` and from `b` bytes back, `gap` fresh bytes between them:
    the offsets alternate (R2; gap 0: without literals)."""
    out = bytearray(K.rnd(seed, max(a, b) + 64))
    fresh = K.rnd(seed + 1, count * gap + 1)
    for i in range(count):
        src = len(out) - (a if i % 2 == 0 else b)
        out += out[src:src + piece]
        out += fresh[i * gap:(i + 1) * gap]
    return bytes(out) + K.rnd(seed + 2, 16)


def rotating(seed: int, count: int, offsets, piece: int) -> bytes:
    """Pieces of `piece` bytes copied from three offsets of one offset code in rotation, one fresh byte between:
    invites offsets that seldom equal one of the two before them, in few offset and match-length codes."""
    out = bytearray(K.rnd(seed, max(offsets) + 64))
    fresh = K.rnd(seed + 1, count)
    for i in range(count):
        src = len(out) - offsets[i % len(offsets)]
        out += out[src:src + piece]
        out.append(fresh[i])
    return bytes(out) + K.rnd(seed + 2, 16)


def dominant(seed: int, common: int, rare: int) -> bytes:
    """`common` matches of 4 bytes (abcd behind a byte that differs), then `rare` pieces matched once each at
    lengths 5, 6, ...: one dominant match-length code and many seen once (the normalisation gives back)."""
    pieces = [K.rnd(seed + 10 + j, 5 + j) for j in range(rare)]
    head = b"".join(p + bytes([200 + j]) for j, p in enumerate(pieces))
    body = b"".join(b"abcd" + bytes([i * 7 % 199]) for i in range(common))
    tail = b"".join(p + bytes([100 + j]) for j, p in enumerate(pieces))
    return head + body + tail + K.rnd(seed + 1, 16)


def wide(seed: int) -> bytes:
    """Literal runs and match lengths across the code ranges: a dictionary of random bytes, then runs of fresh
    bytes of many lengths, each behind a piece of the dictionary of many lengths."""
    dic = K.rnd(seed, 6000)
    lls = list(range(0, 18)) + [19, 21, 23, 27, 31, 39, 47, 63, 100, 200, 400, 800, 1600, 3200]
    mls = list(range(4, 36)) + [36, 38, 40, 42, 46, 50, 58, 66, 82, 98, 130, 200, 300, 600, 1200, 2400, 4800]
    out, at = bytearray(dic), 0
    for j in range(2 * max(len(lls), len(mls))):
        ll, ml = lls[j % len(lls)], mls[j % len(mls)]
        out += K.rnd(seed + 1 + j, ll)
        at = (at + 97) % (len(dic) - ml)
        out += dic[at:at + ml]
    return bytes(out) + K.rnd(seed + 100, 16)


def same_offset_across_chunks(seed: int) -> bytes:
    """Two chunks: the first one's last match and the second one's first match both lie 100 bytes behind their
    source.  The second chunk's first sequence must state its offset in full."""
    p, q = K.rnd(seed, 40), K.rnd(seed + 1, 40)
    first = bytes(CHUNK - 400) + K.rnd(seed + 2, 100) + p + K.rnd(seed + 3, 60) + p + K.rnd(seed + 4, 160)
    return first + K.rnd(seed + 5, 70) + q + K.rnd(seed + 6, 60) + q + K.rnd(seed + 7, 100) + bytes(3000)


@functools.lru_cache(maxsize=None)
def inputs():
    """[(name, input)]"""
    out = list(EC.inputs())
    out.append(("records_600", records(5001, 600)))
    out.append(("records_two_chunks", records(5002, 1100)))            # the stride goes on across the chunk's end
    out.append(("interleaved_literals", interleaved(5003, 300, 96, 160, 24, 3)))
    out.append(("interleaved_no_literals", interleaved(5004, 300, 96, 160, 24, 0)))
    out.append(("interleaved_mixed", interleaved(5005, 150, 72, 200, 16, 1) + interleaved(5006, 150, 72, 200, 16, 0)))
    out.append(("rotating_one_code", rotating(5007, 200, (40, 48, 56), 8)))
    for t in (1, 2, 3, LOG_STEP, LOG_STEP + 1):
        out.append((f"adaptive_sequences_{t}", EC._sequences_input(t)))
    out.append(("dominant_50_14", dominant(5008, 50, 14)))
    out.append(("wide_alphabets", wide(5009)))
    around = records(5011, CHUNK // 32 + 1)
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        out.append((f"records_{n}", around[:n]))
    out.append(("same_offset_across_chunks", same_offset_across_chunks(5020)))
    out.append(("random_two_chunks", K.rnd(5010, 40000)))              # Raw blocks under every option
    return out
