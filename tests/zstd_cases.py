"""The Zstandard fixture (tests/golden/zstd_kat.json), shared by the CPU and the GPU tests."""

import base64
import functools
import hashlib
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_zstd_kat as K  # noqa: E402


# (a window of 1 KiB, no content size) "abcd" as raw literals and a sequence count of 0 written in two bytes (0x80 0x00), then modes, three RLE symbols
# and a bitstream: libzstd 1.4.8 reads the tables and returns "abcd"; the decode contract refuses the frame
COUNT_0_IN_TWO_BYTES = bytes.fromhex("28b52ffd0000650000206162636480005404000101")


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((GOLDEN / "zstd_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, input, {"l1" | "l3" | "l19" | "windowed" | "checksum": frame})]; the frames' bytes come from
    zstd_kat.bin and from the inputs (make_zstd_kat.unpack_frame)"""
    out = []
    for c in kat()["cases"]:
        data = K.input_bytes(c["spec"])
        assert len(data) == c["size"] and hashlib.sha256(data).hexdigest() == c["sha256"], c["name"]
        frames = {}
        for key in K.FRAME_KEYS:
            if key in c:
                frames[key] = K.unpack_frame(c[key], data)
                assert hashlib.sha256(frames[key]).hexdigest() == c[key + "_sha256"], (c["name"], key)
        out.append((c["name"], data, frames))
    return out


@functools.lru_cache(maxsize=None)
def frames():
    """[(name/key, frame, input)]: every frame of every case"""
    return [(f"{name}/{key}", f, data) for name, data, fs in cases() for key, f in fs.items()]


@functools.lru_cache(maxsize=None)
def damaged():
    """[(what, frame, n, accepted, libzstd's output or None, stricter)]: ``accepted`` is True where
    ZSTD_decompress returned n; ``stricter`` names the RFC section of a rule libzstd does not enforce, and such
    a frame is refused here although libzstd accepts it."""
    l3 = {name: fs.get("l3") for name, _, fs in cases()}
    size = {name: len(data) for name, data, _ in cases()}
    out = [(K.damaged_what(d), K.damaged_frame(d, l3), size[d["base"]], d["ret"] == size[d["base"]],
            base64.b64decode(d["out"]) if "out" in d else None, d.get("stricter")) for d in kat()["damaged"]]
    # the frames written by hand come with libzstd's verdict too, and go through the same tests
    return out + [(d["what"], bytes.fromhex(d["frame"]), d["n"], d["ret"] == d["n"], base64.b64decode(d["out"]),
                   d.get("stricter")) for d in kat()["handmade"]]
