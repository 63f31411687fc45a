"""Writes tests/golden/lz4_kat.json: LZ4 blocks made by liblz4, and what liblz4 says about damaged ones.

    python tests/golden/make_lz4_kat.py

Runs on the development machine only: it loads ``liblz4.so.1`` with ctypes (there are no headers).  The tests
read the JSON and need no liblz4.

"version": LZ4_versionString().  "cases": per input its spec (``input_bytes`` makes the bytes from it: large
inputs come from seeds), its size and SHA-256, and the LZ4_compress_default and LZ4_compress_HC level 9 blocks
with their SHA-256 (``pack_block``: base64, long literal runs as references into the input).  "damaged": blocks
(``damaged_block``: base64, or a cut or a changed byte of a case's default block) with the capacity ``n`` they were offered, what
``LZ4_decompress_safe(block, n)`` returned, and its output (base64) where that was ``n``: every truncation of
two small blocks, single-byte changes of every token, offset byte and extension byte of two more, an offset of
0 (marked "offset_zero": liblz4 1.9.3 accepts it and returns n although the bytes it "decodes" are the
destination's own; the decoders here reject it), and an offset one past the produced output.
"""
import base64
import ctypes as C
import hashlib
import json
import sys
import zlib
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

SENTENCE = b"The quick brown fox jumps over the lazy dog while the archive grows by one more block. "


def rnd(seed, n, below=256) -> bytes:
    return np.random.default_rng(seed).integers(0, below, n, dtype=np.uint8).tobytes()


def input_bytes(spec) -> bytes:
    kind = spec["kind"]
    if kind == "hex":
        return bytes.fromhex(spec["hex"])
    if kind == "zeros":
        return bytes(spec["length"])
    if kind == "sentence":
        return (SENTENCE * (spec["length"] // len(SENTENCE) + 1))[:spec["length"]]
    if kind == "random":
        return rnd(spec["seed"], spec["length"], spec.get("below", 256))
    if kind == "literal_run":  # `run` bytes that cannot match, then 20 of them again, then 12 more
        a = rnd(spec["seed"], spec["run"])
        return a + a[:20] + rnd(spec["seed"] + 1, 12)
    if kind == "match_length":  # a piece of `match` bytes twice, 8 bytes between, 12 behind
        a = rnd(spec["seed"], spec["match"])
        return a + rnd(spec["seed"] + 1, 8) + a + rnd(spec["seed"] + 2, 12)
    if kind == "offset":  # a pattern of `offset` bytes, then its first `repeat` bytes cyclically, then 12 more
        a = rnd(spec["seed"], spec["offset"])
        rep = (a * (spec["repeat"] // len(a) + 1))[:spec["repeat"]]
        return a + rep + rnd(spec["seed"] + 1, 12)
    if kind == "sandwich":  # random, zeros, the same random
        a = rnd(spec["seed"], spec["edge"])
        return a + bytes(spec["zeros"]) + a
    if kind == "near_end":  # a piece of 32 bytes twice, 8 bytes between, `tail` bytes behind
        a = rnd(spec["seed"], 32)
        return a + rnd(spec["seed"] + 1, 8) + a + rnd(spec["seed"] + 2, spec["tail"])
    raise ValueError(kind)


def case_specs():
    specs = [
        ("empty", {"kind": "hex", "hex": ""}),
        ("single_byte", {"kind": "hex", "hex": "5a"}),
        ("literals_12", {"kind": "hex", "hex": b"abcdefghijkl".hex()}),
        ("same_byte_13", {"kind": "hex", "hex": "41" * 13}),
    ]
    specs += [(f"literal_run_{n}", {"kind": "literal_run", "seed": 100 + n, "run": n})
              for n in (14, 15, 16, 269, 270, 271)]
    specs += [(f"match_length_{n}", {"kind": "match_length", "seed": 200 + n, "match": n})
              for n in (18, 19, 20, 273, 274, 275)]
    specs += [(f"offset_{n}", {"kind": "offset", "seed": 300 + n, "offset": n, "repeat": 64})
              for n in (1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 65535)]
    specs += [
        ("offset_65536", {"kind": "offset", "seed": 400, "offset": 65536, "repeat": 64}),
        ("zeros_65536", {"kind": "zeros", "length": 65536}),
        ("zeros_70000", {"kind": "zeros", "length": 70000}),
        ("sentence_18000", {"kind": "sentence", "length": 18000}),
        ("random_below_4", {"kind": "random", "seed": 500, "length": 20000, "below": 4}),
        ("random_4096", {"kind": "random", "seed": 501, "length": 4096}),
        ("sandwich", {"kind": "sandwich", "seed": 502, "edge": 300, "zeros": 70000}),
    ]
    specs += [(f"near_end_{t}", {"kind": "near_end", "seed": 600 + t, "tail": t}) for t in (0, 4, 5, 6, 11, 12, 13)]
    return specs


def b64(b: bytes) -> str:
    return base64.b64encode(b).decode()


def text(b: bytes):
    """Bytes as JSON: base64, or {"z": base64 of zlib} where that is shorter."""
    z = zlib.compress(b, 9)
    return {"z": b64(z)} if len(z) + 16 < len(b) else b64(b)


def untext(t) -> bytes:
    return zlib.decompress(base64.b64decode(t["z"])) if isinstance(t, dict) else base64.b64decode(t)


def pack_block(block: bytes, data: bytes, sequences) -> list:
    """A valid block as a list of parts: ``text`` values, and [start, length] for a literal run of 48 bytes or
    more, which is data[start : start + length] (a literal at output position p is the input's byte p).  Keeps
    the blocks of inputs that hardly compress out of the file; ``unpack_block`` puts them back."""
    parts, done = [], 0
    for q in sequences:
        if q.literals >= 48:
            assert block[q.literal_at:q.literal_at + q.literals] == data[q.out_at:q.out_at + q.literals]
            parts += [text(block[done:q.literal_at]), [q.out_at, q.literals]]
            done = q.literal_at + q.literals
    if done < len(block) or not parts:
        parts.append(text(block[done:]))
    return parts


def unpack_block(parts, data: bytes) -> bytes:
    return b"".join(data[p[0]:p[0] + p[1]] if isinstance(p, list) else untext(p) for p in parts)


def damaged_block(rec, default_blocks) -> bytes:
    """The block of a "damaged" record: written out, or a case's LZ4_compress_default block cut to "cut" bytes
    or with the byte at "at" set to "byte"."""
    if "block" in rec:
        return base64.b64decode(rec["block"])
    s = default_blocks[rec["base"]]
    return s[:rec["cut"]] if "cut" in rec else s[:rec["at"]] + bytes([rec["byte"]]) + s[rec["at"] + 1:]


def main():
    sys.path.insert(0, str(HERE.parent))
    import lz4_ref

    L = C.CDLL("liblz4.so.1")
    L.LZ4_versionString.restype = C.c_char_p
    L.LZ4_compressBound.argtypes = [C.c_int]
    L.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]

    def compress(data, level):
        cap = L.LZ4_compressBound(len(data))
        buf = C.create_string_buffer(cap)
        n = (L.LZ4_compress_default(data, buf, len(data), cap) if level is None else
             L.LZ4_compress_HC(data, buf, len(data), cap, level))
        assert n > 0
        return buf.raw[:n]

    def decompress(block, n):
        buf = C.create_string_buffer(max(n, 1))
        r = L.LZ4_decompress_safe(block, buf, len(block), n)
        return r, buf.raw[:max(r, 0)]

    cases, streams = [], {}
    for name, spec in case_specs():
        data = input_bytes(spec)
        d, h = compress(data, None), compress(data, 9)
        for s in (d, h):
            assert decompress(s, len(data)) == (len(data), data)
        streams[name] = (data, d)
        case = {"name": name, "spec": spec, "size": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        for key, s in (("default", d), ("hc9", h)):
            case[key] = pack_block(s, data, lz4_ref.walk(s))
            case[key + "_sha256"] = hashlib.sha256(s).hexdigest()
            assert unpack_block(case[key], data) == s
        cases.append(case)

    damaged = []

    def add(what, how, n, offset_zero=False):
        block = damaged_block(how, {k: v[1] for k, v in streams.items()})
        r, out = decompress(block, n)
        rec = dict({"what": what}, **how, n=n, ret=r)
        if offset_zero:
            # liblz4 1.9.3 does not reject offset 0: it copies the destination onto itself and returns n, so its
            # "output" is whatever the buffer held.  Recorded as it is; this project's decoders reject the block.
            rec["offset_zero"] = True
        elif r == n:
            rec["out"] = b64(out)
        damaged.append(rec)

    for name in ("same_byte_13", "literal_run_16"):
        data, s = streams[name]
        for cut in range(len(s)):
            add(f"{name} cut to {cut}", {"base": name, "cut": cut}, len(data))
    for name in ("literal_run_270", "match_length_274"):
        data, s = streams[name]
        spots = set()
        for q in lz4_ref.walk(s):
            lit_ext = (q.literals - 15) // 255 + 1 if q.literals >= 15 else 0
            token_at = q.literal_at - 1 - lit_ext
            spots.update(range(token_at, q.literal_at))  # the token and the literal length's bytes
            if q.offset is not None:
                at = q.literal_at + q.literals
                ext = (q.match - 4 - 15) // 255 + 1 if q.match - 4 >= 15 else 0
                spots.update(range(at, at + 2 + ext))  # the offset and the match length's bytes
        for at in sorted(spots):
            for v in sorted({s[at] ^ 0x01, s[at] ^ 0x10, s[at] ^ 0x80, 0x00, 0xFF} - {s[at]}):
                add(f"{name} byte {at} = {v:#04x}", {"base": name, "at": at, "byte": v}, len(data))
    # 4 literals, then a match of 8 at offset 0 / at offset 5 (one past the 4 bytes produced), then 5 literals
    for off in (0, 5, 4):
        block = bytes([0x44]) + b"abcd" + bytes([off, 0]) + bytes([0x50]) + b"vwxyz"
        add(f"offset {off} behind 4 literals", {"block": b64(block)}, 17, offset_zero=off == 0)

    out = {"version": L.LZ4_versionString().decode(), "cases": cases, "damaged": damaged}
    lines = [json.dumps(r, separators=(",", ":")) for r in cases + damaged]  # one record per line
    (HERE / "lz4_kat.json").write_text(
        '{"version":%s,\n"cases":[\n%s\n],\n"damaged":[\n%s\n]}\n' %
        (json.dumps(out["version"]), ",\n".join(lines[:len(cases)]), ",\n".join(lines[len(cases):])))
    print(f"{len(cases)} cases, {len(damaged)} damaged blocks, liblz4 {out['version']}")


if __name__ == "__main__":
    main()
