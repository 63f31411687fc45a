"""The incompressible categorizer's inputs, shared by the fixture's maker (tests/golden/make_incompressible_kat.py),
the CPU and the GPU tests, and a restatement of the reference's fragment rules in plain Python.

The data comes from the project's own generators: the sentence text and random bytes of make_lz4_kat, ``skewed`` of
tests/zstd_enc_cases.py, ``repeats`` of tests/search_cases.py.  The *asserted* families restate the reference's own
tests (test/incompressible_categorizer_test.cpp) with this data; every piece of them has, by the maker's check, a
libzstd level -1 ratio of at most 0.90 or at least 1.0 and the same verdict at 0.99 from libzstd and from this
project's encoder.  The ``borderline`` family is recorded with both verdicts and asserted against neither.
"""

import functools
from typing import List, NamedTuple

import search_cases as SC
import zstd_enc_cases as EC

K = EC.K
KIB = 1024


def text(n: int) -> bytes:
    return K.input_bytes({"kind": "sentence", "length": n})


def random_bytes(seed: int, n: int) -> bytes:
    return K.rnd(seed, n)


class Case(NamedTuple):
    name: str
    data: bytes
    block_size: int
    fragments: bool
    min_input_size: int
    asserted: bool  # an asserted family: its pieces obey the maker's condition


def _fragments_input() -> bytes:
    return (text(12 * KIB) + random_bytes(9101, 12 * KIB) + text(12 * KIB) + random_bytes(9102, 12 * KIB) +
            text(3 * KIB))


def far_repeat() -> bytes:
    """Random bytes whose only redundancy is a repeat at a distance above the encoder's 64 KiB window."""
    piece = random_bytes(9301, 40 * KIB)
    return piece + random_bytes(9302, 30 * KIB) + piece


@functools.lru_cache(maxsize=None)
def cases() -> List[Case]:
    out = [
        Case("random_10000", random_bytes(9001, 10000), 1 << 20, False, 256, True),
        Case("text_10000", text(10000), 1 << 20, False, 256, True),
        Case("categorize_fragments", _fragments_input(), 8 * KIB, True, 256, True),
        Case("min_input_size_999", random_bytes(9002, 999), 1 << 20, False, 1000, True),
        Case("min_input_size_10000", random_bytes(9003, 10000), 1 << 20, False, 1000, True),
        # (short copies between fresh bytes rather than the sentence, whose ratio of 0.01 leaves no room a tenth
        # below it; libzstd's negative levels store literals as they are, so bytes that only an entropy coder
        # shrinks are no asserted input)
        Case("max_ratio_text", SC.repeats(9006, 10000), 1 << 20, False, 256, True),
        Case("repeats_40000", SC.repeats(9005, 40000), 16 * KIB, True, 256, True),
        # not asserted against libzstd: bytes with little to gain, and a repeat that only a larger window sees
        Case("borderline_below_200", K.rnd(9201, 20000, 200), 8 * KIB, True, 256, False),
        Case("borderline_below_128", K.rnd(9202, 20000, 128), 8 * KIB, True, 256, False),
        Case("borderline_skewed_below_16", EC.skewed(9004, 20000, 15), 8 * KIB, True, 256, False),
        Case("borderline_far_repeat", far_repeat(), 1 << 20, False, 256, False),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


def pieces(case: Case) -> List[bytes]:
    return [case.data[o:o + case.block_size] for o in range(0, len(case.data), case.block_size)]


# ---------------------------------------------------------------------------
# the reference's rules, restated (src/writer/categorizer/incompressible_categorizer.cpp)
# ---------------------------------------------------------------------------
DEFAULT, INCOMPRESSIBLE = "<default>", "incompressible"


class ExtentModel:
    """``data_extent_fragments``: compress() per piece, add_fragment, get_fragments.  ``size_of(piece)`` is the
    compressed size."""

    def __init__(self, block_size, generate_fragments, max_ratio, size_of):
        self.block_size, self.generate, self.max_ratio, self.size_of = block_size, generate_fragments, max_ratio, size_of
        self.reset()

    def reset(self):
        self.total_in = self.total_out = self.blocks = self.hard = 0
        self.fragments = []

    def add_data(self, data: bytes):
        for o in range(0, len(data), self.block_size):
            piece = data[o:o + self.block_size]
            size = self.size_of(piece)
            self.total_in += len(piece)
            self.total_out += size
            self.blocks += 1
            verdict = float(size) >= self.max_ratio * float(len(piece))
            self.hard += verdict
            if self.generate:
                category = INCOMPRESSIBLE if verdict else DEFAULT
                if self.fragments and self.fragments[-1][0] == category:
                    self.fragments[-1] = (category, self.fragments[-1][1] + len(piece))
                else:
                    self.fragments.append((category, len(piece)))

    def get_fragments(self, force_single_default=True):
        if not self.fragments and self.total_in > 0:
            hard = self.blocks > 0 and float(self.total_out) >= self.max_ratio * float(self.total_in)
            if force_single_default or hard:
                self.fragments.append((INCOMPRESSIBLE if hard else DEFAULT, self.total_in))
        return list(self.fragments)


def model_file(parts, cfg, size_of, is_hole):
    """``incompressible_categorizer_::job``, the job's add_data / add_hole / result over a file's parts (neighbouring
    data already merged): (fragments or None, (incompressible_blocks, total_blocks, total_in, total_out))."""
    total = sum(p.size if is_hole(p) else len(p) for p in parts)
    if total < cfg.min_input_size:
        return None, None
    cur = ExtentModel(cfg.block_size, cfg.generate_fragments, cfg.max_ratio, size_of)
    frags, stats = [], [0, 0, 0, 0]

    def flush(force):
        frags.extend(cur.get_fragments(force))
        for i, v in enumerate((cur.hard, cur.blocks, cur.total_in, cur.total_out)):
            stats[i] += int(v)
        cur.reset()

    for p in parts:
        if is_hole(p):
            flush(True)
            frags.append((DEFAULT, p.size))
        else:
            cur.add_data(p)
    flush(bool(frags))
    return frags, tuple(stats)
