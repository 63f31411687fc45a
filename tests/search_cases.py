"""The inputs of the search-word tests (the deeper match search of the LZ4 and Zstandard encoders), shared by the
CPU and the GPU tests, and a restatement of the search's definition in plain Python.

``inputs()`` is every input of tests/zstd_enc_adaptive_cases.py (which holds tests/lz4_cases.py's encoder inputs),
then the constructed families below.  A constructed input is laid out position by position (``Layout``): pieces
at stated positions in a filler that holds no 4-byte word twice, so what a search can find at a position follows
from the input alone.  ``AIMS`` says per constructed input which position is aimed at and what each search word
must make of it; tests/test_search_host.py reads the answers from ``restate``.

``restate(data, search)`` is written from the definition's text (top of dwarfs_amd/csrc/lz4_host.cpp), not from the
C++: chunks, the table's start, steps, buckets of the ``depth`` highest positions, scores capped at ``CAP``, the
nearest of equal scores, the LAZY choice, the cut of a length.  It returns [(position, length, offset)].
"""

import functools
import struct

import numpy as np

import zstd_enc_adaptive_cases as AC

K = AC.K
CHUNK, STEP, HASH_BITS, CAP, LAZY = 32768, 64, 12, 64, 0x100
DEPTHS = (1, 2, 4, 8)
WORDS = tuple(d | lazy for lazy in (0, LAZY) for d in DEPTHS)  # the eight words; 0 is the one-candidate search


def hash4(word: int) -> int:
    return (word * 2654435761 & 0xFFFFFFFF) >> (32 - HASH_BITS)


def _words_and_hashes(data: bytes):
    a = np.frombuffer(data, np.uint8).astype(np.uint64)
    w = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
    h = (w * 2654435761 & 0xFFFFFFFF) >> (32 - HASH_BITS)
    return w.tolist(), h.tolist()


def _prefix(data: bytes, c: int, p: int, start: int, lim: int) -> int:
    """The common prefix of data[c:] and data[p:], known to be at least `start`, cut at `lim`."""
    k = start
    while k + 64 <= lim and data[c + k:c + k + 64] == data[p + k:p + k + 64]:
        k += 64
    while k < lim and data[c + k] == data[p + k]:
        k += 1
    return k


def restate(data: bytes, search: int, scores=None):
    """The sequences of `data` under the search word.  `scores`, a dict, receives {position: (best candidate,
    score)} for every position that was looked at and has a best."""
    n = len(data)
    if n < 13:
        return []
    depth, lazy = (search & ~LAZY) or 1, bool(search & LAZY)  # (0: one candidate, never lazy)
    word, hsh = _words_and_hashes(data)
    last_start, out = n - 12, []
    for cs in range(0, n, CHUNK):
        ce = min(cs + CHUNK, n)
        lim_end = min(ce, n - 5)
        tab = [[] for _ in range(1 << HASH_BITS)]  # per hash value the positions inserted, in order
        for q in range(max(cs - CHUNK, 0), cs):
            if q + 4 <= n:
                tab[hsh[q]].append(q)
        cursor = cs
        for ss in range(cs, ce, STEP):
            se = min(ss + STEP, ce)
            if cursor >= se:
                continue
            best = {}
            for p in range(max(cursor, ss), se):  # (no position before the cursor is ever taken or compared)
                if p > last_start or p + 4 > lim_end:
                    continue
                top = (0, 0)  # (score, candidate): the highest score, of equal scores the highest position
                for c in tab[hsh[p]][-depth:]:
                    if word[c] == word[p] and p - c <= 65535:
                        top = max(top, (_prefix(data, c, p, 4, min(lim_end - p, CAP)), c))
                if top[0]:
                    best[p] = top
                    if scores is not None:
                        scores[p] = (top[1], top[0])
            for p in range(ss, se):
                if p + 4 <= n:
                    tab[hsh[p]].append(p)
            p = max(cursor, ss)
            while p < se:
                passed = lazy and p + 1 < se and p in best and p + 1 in best and best[p + 1][0] > best[p][0]
                if p not in best or passed:
                    p += 1
                    continue
                score, c = best[p]
                length = _prefix(data, c, p, score, lim_end - p)
                out.append((p, length, p - c))
                cursor = p = p + length
    return out


# ---------------------------------------------------------------------------
# constructed inputs
# ---------------------------------------------------------------------------
class Layout:
    """Pieces at stated positions; what lies between is filler in which every 4-byte word differs from every
    other and from the pieces' (bytes 128..255 counting in base 128 behind a 0x7f: the pieces use bytes below
    0x7f, and so does whatever ends a match).  No word that begins in the filler has the hash of a word given to
    ``keep_clear``: the buckets of the words aimed at hold pieces only."""

    def __init__(self):
        self.buf = bytearray()
        self.count = 0
        self.puts = 0
        self.avoid = set()

    def keep_clear(self, piece: bytes, words: int = 6):
        for i in range(min(words, len(piece) - 3)):
            self.avoid.add(hash4(struct.unpack_from("<I", piece, i)[0]))

    def _hit(self, data: bytes) -> bool:
        return any(hash4(struct.unpack_from("<I", data, i)[0]) in self.avoid for i in range(len(data) - 3))

    def fill_to(self, at: int):
        assert at >= len(self.buf), (at, len(self.buf))
        lead = 0x7F
        while len(self.buf) < at:
            self.count += 1
            c = self.count
            group = bytes([lead, 128 + c % 128, 128 + c // 128 % 128, 128 + c // 16384 % 128])
            if self._hit(bytes(self.buf[-3:]) + group):
                lead = 0xFF if lead == 0x7F else lead - 1  # (the word that ends in the lead byte may be the hit)
            else:
                self.buf += group
                lead = 0x7F
        del self.buf[at:]

    def put(self, at: int, piece: bytes) -> int:
        """The piece at `at`; the byte before it differs from the one before each of the 127 pieces put before,
        so no match of a repeated piece starts ahead of it."""
        self.fill_to(at)
        while at:
            self.buf[at - 1] = 0x80 + self.puts % 128
            self.puts += 1
            if not self._hit(bytes(self.buf[-3:]) + piece[:3]):
                break
        self.buf += piece
        return at

    def done(self, tail: int = 24) -> bytes:
        self.fill_to(len(self.buf) + tail)
        return bytes(self.buf)


def piece(seed: int, n: int) -> bytes:
    """n bytes below 0x78 with no 4-byte word twice: a counter in base 100 between two seed bytes.  (0x78 to
    0x7e end a match behind a piece: no piece holds them.)"""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += bytes([100 + seed % 20, i % 100, i // 100 % 100, 100 + (seed // 20) % 20])
        i += 1
    return bytes(out[:n])


def colliding(word: bytes, count: int, seed: int):
    """`count` 4-byte words (bytes below 0x7f) other than `word` with its hash4."""
    want, out, v = hash4(struct.unpack("<I", word)[0]), [], seed * 7919
    while len(out) < count:
        v += 1
        cand = bytes([v % 100, v // 100 % 100, v // 10000 % 100, 101 + seed % 20])
        if cand != word and hash4(struct.unpack("<I", cand)[0]) == want:
            out.append(cand)
    return out


AIMS = {}  # name: {"at": the position or positions aimed at, and what the family's test needs beside them}


def laid_out(make):
    return make(Layout())


def older_is_longer(lay: Layout, decoys: int, units: int = 6):
    """Per unit: a source of 40 bytes, then `decoys` later occurrences of its first 4 to 6 bytes, each in a step
    of its own, then the 40 bytes again: the source is the (decoys + 1)th newest entry of its bucket."""
    at, aims = 0, []
    for u in range(units):
        body = piece(10 * decoys + u, 40)
        lay.keep_clear(body)
        lay.put(at + 7, body)
        at += 128
        for d in range(decoys):
            keep = 4 + d % 3
            lay.put(at + 11, body[:keep] + bytes([0x78 + d % 7, 0x7E]))
            at += 128
        aims.append(lay.put(at + 13, body))
        at += 128
    return lay.done(), aims


def colliding_words(lay: Layout, units: int = 6):
    """Per unit: a source of 40 bytes, then three other words with the hash of its first word, then the 40 bytes:
    depth 4 is the first to keep the source in the bucket, and no collision is a match."""
    at, aims = 0, []
    for u in range(units):
        body = piece(300 + u, 40)
        lay.keep_clear(body)
        lay.put(at + 5, body)
        at += 128
        for w in colliding(body[:4], 3, u):
            lay.put(at + 9, w)
            at += 128
        aims.append(lay.put(at + 3, body))
        at += 128
    return lay.done(), aims


CLIMB_BASE = 12


def climb(lay: Layout, steps: int, lane: int):
    """A query q at a position p with p % 64 == `lane`; source j (j = 0 .. steps) holds q[j : 2 * j + 12] between
    bytes that end the match.  Position p + j scores 12 + j through source j, the newest holder of its 4 bytes,
    and 10 + j through source j - 1: every position up to p + steps scores one more than the one before it, and
    p + steps + 1 scores 11 + steps."""
    q = piece(400 + steps + lane, CLIMB_BASE + 2 * steps + 8)
    lay.keep_clear(q, steps + 3)
    at = 0
    for j in range(steps + 1):
        lay.put(at + 20, bytes([0x78 + j]) + q[j:2 * j + CLIMB_BASE] + bytes([0x7E]))
        at += 128
    p = lay.put(at + lane, q)
    return lay.done(), p


def cap_both(lay: Layout):
    """The query's position scores CAP through an 80-byte source; the next position scores CAP too, through a
    source that goes on for 100: the longer one must not make the search pass the first over."""
    q = piece(500, 120)
    lay.keep_clear(q)
    lay.put(20, bytes([0x78]) + q[:80] + bytes([0x7E]))
    lay.put(148, bytes([0x79]) + q[1:101] + bytes([0x7D]))
    p = lay.put(256 + 10, q)
    return lay.done(), p


def tie(lay: Layout, cut_at_cap: bool):
    """Two sources of the query's first bytes with equal scores: the nearer one wins.  `cut_at_cap`: the older
    source goes on for 100 bytes, the nearer one for 70, and both score CAP."""
    q = piece(510 + cut_at_cap, 120)
    far, near = (100, 70) if cut_at_cap else (20, 20)
    lay.keep_clear(q)
    lay.put(20, q[:far] + bytes([0x7E]))
    lay.put(276, q[:near] + bytes([0x7D]))
    p = lay.put(512 + 10, q)
    return lay.done(), p, near


def same_hash_steps(unit: bytes):
    """A run of one repeated unit (64 equal hashes, or two groups of 32, in a step), something else, then a short
    run again: its bucket holds the highest positions of the first run's last inserted step."""
    return unit * (400 // len(unit)) + piece(520, 100) + unit * (40 // len(unit)) + piece(521, 30)


def far_offsets():
    """Zeros, with words at 65532, 65535 and 65536 bytes before their second occurrence in the third chunk: the
    first lies at the window's start and is found by a match cut to 4 bytes at the chunk's end; the other two
    lie before the window."""
    buf = bytearray(3 * CHUNK + 16)
    for src, dst, w in ((CHUNK, 3 * CHUNK - 4, b"WXYZ"), (CHUNK - 103, 3 * CHUNK - 104, b"efgh"),
                        (CHUNK - 304, 3 * CHUNK - 304, b"ijkl")):
        buf[src:src + 4] = w
        buf[dst:dst + 4] = w
    # (CHUNK - 103 -> 3 * CHUNK - 104: 65535 apart; CHUNK - 304 -> 3 * CHUNK - 304: 65536 apart)
    return bytes(buf)


def ends_at_limit(lay: Layout):
    """The second copy of a piece runs to the input's end: its match is cut 5 bytes before it; two sources tie
    at the cut."""
    p = piece(530, 50)
    lay.keep_clear(p)
    lay.put(10, p)
    lay.put(138, p[:40] + bytes([0x7E]))
    lay.put(266, p[:30])
    return (bytes(lay.buf),)


def repeats(seed: int, n: int) -> bytes:
    """Copies of 4 to 40 bytes from random places of what is there, between runs of 1 to 3 bytes of 16 values:
    many candidates of many lengths per position."""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 16, 64, dtype=np.uint8).tobytes())
    while len(out) < n:
        if rng.integers(0, 4):
            src, length = int(rng.integers(0, len(out) - 4)), int(rng.integers(4, 41))
            out += out[src:src + length]
        else:
            out += rng.integers(0, 16, int(rng.integers(1, 4)), dtype=np.uint8).tobytes()
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def constructed():
    """[(name, input)]; fills AIMS."""
    out = []
    for depth in (2, 4, 8):  # the source is the depth-th newest entry: this depth is the first to find it
        data, aims = laid_out(lambda lay: older_is_longer(lay, depth - 1))
        out.append((f"older_is_longer_{depth}", data))
        AIMS[f"older_is_longer_{depth}"] = {"at": aims, "first_depth": depth}
    for depth in DEPTHS:  # `depth` newer entries: this depth must miss it
        data, aims = laid_out(lambda lay: older_is_longer(lay, depth))
        out.append((f"too_deep_for_{depth}", data))
        AIMS[f"too_deep_for_{depth}"] = {"at": aims, "missed_by": depth}
    data, aims = laid_out(colliding_words)
    out.append(("colliding_words", data))
    AIMS["colliding_words"] = {"at": aims, "first_depth": 4}
    out.append(("zeros_then_zeros", same_hash_steps(b"\0")))
    out.append(("period_2_then_period_2", same_hash_steps(b"ab")))
    for steps, lane, name in ((1, 10, "climb_1"), (3, 10, "climb_3"), (1, 63, "climb_into_next_step"),
                              (3, 61, "climb_to_step_end")):
        data, p = laid_out(lambda lay: climb(lay, steps, lane))
        out.append((name, data))
        AIMS[name] = {"at": p, "steps": steps, "lane": lane}
    data, p = laid_out(cap_both)
    out.append(("cap_both", data))
    AIMS["cap_both"] = {"at": p}
    for cut in (False, True):
        data, p, near = laid_out(lambda lay: tie(lay, cut))
        name = "tie_at_cap" if cut else "tie"
        out.append((name, data))
        AIMS[name] = {"at": p, "length": near, "offset": p - 276}
    out.append(("far_offsets", far_offsets()))
    out.append(("ends_at_limit", laid_out(ends_at_limit)[0]))
    big = repeats(540, 2 * CHUNK + 777)
    for n in (0, 1, 12, 13, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 777):
        out.append((f"repeats_{n}", big[:n]))
    return out


@functools.lru_cache(maxsize=None)
def inputs():
    """[(name, input)]: the existing lists, then the constructed inputs"""
    out = list(AC.inputs()) + constructed()
    assert len({name for name, _ in out}) == len(out)
    return out
