"""Shared inputs of the digest tests (plain Python and numpy; no GPU, no native code): the messages of
tests/golden/digest_kat.json regenerated from their seeds, their expected digests from digest_kat.bin, and the batch
shapes both the host and the device tests run -- so that the two see the same bytes at the same addresses modulo 16.
"""

import functools
import json
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_digest_kat as MK  # noqa: E402

NEW = tuple(MK.ALGORITHMS)  # the thirteen names computed by the digest kernels
OLD = ("xxh3-64", "xxh3-128", "sha512-256")
WIDTH = {name: nbytes for name, (_, nbytes) in MK.ALGORITHMS.items()}
FILL = 0xA5
GUARD = 64
LANE_SPREAD = 4096  # above this many files a wave holds more than one file (lane_waves)


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((GOLDEN / "digest_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def messages():
    """The messages' bytes, regenerated once: [(bytes, misalign)]."""
    return [(MK.message_bytes(i, n), mis) for i, (n, mis) in enumerate(kat()["messages"])]


@functools.lru_cache(maxsize=None)
def expected(name):
    """uint8 [nmessages, digest bytes] of one algorithm, read-only."""
    blob = np.frombuffer((GOLDEN / "digest_kat.bin").read_bytes(), np.uint8)
    n, at = len(kat()["messages"]), 0
    for a in kat()["algorithms"]:
        if a["name"] == name:
            rows = blob[at:at + n * a["bytes"]].reshape(n, a["bytes"])
            rows.flags.writeable = False
            return rows
        at += n * a["bytes"]
    raise KeyError(name)


def place(indices, spare=16):
    """The messages `indices` laid into one buffer whose address is a multiple of 16, message k starting at a
    16-byte boundary plus its misalignment: ``(buffer, offsets, sizes)``, with `spare` bytes behind the last one."""
    msgs = messages()
    offs, at = [], 0
    for i in indices:
        m, mis = msgs[i]
        at = (at + 15) // 16 * 16 + mis
        offs.append(at)
        at += len(m)
    raw = np.zeros(at + spare + 16, np.uint8)
    start = -raw.ctypes.data % 16
    buf = raw[start:start + at + spare]
    for o, i in zip(offs, indices):
        buf[o:o + len(msgs[i][0])] = np.frombuffer(msgs[i][0], np.uint8)
    return buf, np.array(offs, np.int64), np.array([len(msgs[i][0]) for i in indices], np.int64)


@functools.lru_cache(maxsize=None)
def batch_shapes():
    """name -> message indices.  `all`: every message of the fixture (the length sweep on 16-byte boundaries, the
    boundary lengths at every misalignment); batches of 1, 63, 64 and 65 files around the wave width, each with an
    empty file between others and a long one; `spread`: more files than the lane spread bound, so waves hold
    several files each, short messages repeated with the empty one among them."""
    n = len(kat()["messages"])
    sweep = 305
    shapes = {"all": list(range(n))}
    for k in (1, 63, 64, 65):
        pick = [(37 * j + 11) % n for j in range(k)]
        pick[0] = 304            # 65539 bytes
        if k > 2:
            pick[1], pick[2] = 0, sweep + 3  # the empty message on a boundary and off it
        shapes[f"n{k}"] = pick
    shapes["spread"] = [(7 * j) % 301 for j in range(LANE_SPREAD + 200)]
    return shapes


def guarded_out(n, width, module):
    """A pre-filled output of n rows with GUARD bytes behind the last row (numpy or torch module given)."""
    return module.full((n * width + GUARD,), FILL, dtype=module.uint8)


def select_mask(n):
    return np.array([0 if k % 3 == 1 else 1 for k in range(n)], np.uint8)


def check_rows(got_flat, want_rows, select=None, what=""):
    """got_flat: uint8 [n * width + GUARD] as numpy.  Selected rows equal the fixture, the others and the guard
    keep FILL."""
    n, width = want_rows.shape
    got = got_flat[:n * width].reshape(n, width)
    sel = np.ones(n, bool) if select is None else select.astype(bool)
    bad = np.nonzero((got != want_rows).any(axis=1) & sel)[0]
    assert len(bad) == 0, (what, "wrong digests at", bad[:8].tolist())
    assert (got[~sel] == FILL).all(), (what, "an unselected row was written")
    assert (got_flat[n * width:] == FILL).all(), (what, "the guard bytes behind the last row were written")
