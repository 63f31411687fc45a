"""The LZ4 fixture (tests/golden/lz4_kat.json) and the encoder's inputs, shared by the CPU and the GPU tests."""

import base64
import functools
import hashlib
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_lz4_kat as K  # noqa: E402

from dwarfs_amd import _native as N  # noqa: E402


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((GOLDEN / "lz4_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, input, LZ4_compress_default block, LZ4_compress_HC level 9 block)]"""
    out = []
    for c in kat()["cases"]:
        data = K.input_bytes(c["spec"])
        assert len(data) == c["size"] and hashlib.sha256(data).hexdigest() == c["sha256"], c["name"]
        blocks = [K.unpack_block(c[key], data) for key in ("default", "hc9")]
        assert [hashlib.sha256(b).hexdigest() for b in blocks] == [c["default_sha256"], c["hc9_sha256"]], c["name"]
        out.append((c["name"], data, *blocks))
    return out


@functools.lru_cache(maxsize=None)
def damaged():
    """[(what, block, n, liblz4's return value, liblz4's output or None)].  The block with an offset of 0 is
    listed with a return value of -1: liblz4 1.9.3 returns n for it, but copies its destination onto itself, so
    there are no bytes to agree with, and the decode contract names offset 0 as corrupt."""
    default = {name: d for name, _, d, _ in cases()}
    return [(d["what"], K.damaged_block(d, default), d["n"], -1 if d.get("offset_zero") else d["ret"],
             base64.b64decode(d["out"]) if "out" in d else None) for d in kat()["damaged"]]


@functools.lru_cache(maxsize=None)
def encoder_inputs():
    """[(name, input)]: every fixture input, then the cases laid out from the encoder's own constants: sizes
    around the chunk and the search step, and a repeat that crosses a chunk boundary."""
    chunk, step = N.lib().rpp_lz4_chunk_bytes(), N.lib().rpp_lz4_step_positions()
    out = [(name, data) for name, data, _, _ in cases()]
    for n in (step - 1, step, step + 1, 2 * step + 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk + 1,
              chunk + step - 1, chunk + step + 1):
        out.append((f"sentence_{n}", K.input_bytes({"kind": "sentence", "length": n})))
        out.append((f"below4_{n}", K.rnd(700 + n % 97, n, 4)))
    piece = K.rnd(800, 300)
    # the second copy of `piece` starts 150 bytes before the chunk boundary and ends 150 behind it
    # (zeros between: a table entry survives only until another position with its hash is inserted)
    out.append(("repeat_across_chunks", piece + bytes(chunk - 150 - 300) + piece + K.rnd(802, 50)))
    # ... and one whose source lies in the chunk before: the table starts with that chunk's positions
    out.append(("source_in_previous_chunk", bytes(chunk - 400) + piece + bytes(500) + piece + K.rnd(805, 50)))
    return out
