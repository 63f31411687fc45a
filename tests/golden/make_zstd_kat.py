"""Writes tests/golden/zstd_kat.json: Zstandard frames made by libzstd, and what libzstd says about damaged ones.

    python tests/golden/make_zstd_kat.py

Runs on the development machine only: it loads ``libzstd.so.1`` with ctypes (there are no headers).  The tests
read the JSON and need no libzstd.

"version": ZSTD_versionString().  "cases": per input its spec (``input_bytes`` makes the bytes from it: large
inputs come from seeds), its size and SHA-256, and its frames: ``ZSTD_compress`` at levels 1, 3 and 19 ("l1",
"l3", "l19"; only "l19" for the inputs tried for coverage alone) and, for some, ``ZSTD_compress2`` with
parameters ("windowed": windowLog 17, so the frame has a Window_Descriptor; "checksum": the checksum flag), each
with its SHA-256.  A frame is a list of parts (``pack_frame``): pieces of the binary file zstd_kat.bin written
beside the JSON, and, for Raw blocks and raw literal runs of 48 bytes or more, references into the input.
"damaged": a case's "l3" frame cut to "cut" bytes or with the byte at "at" set to "byte", offered the input's
size as capacity: what ``ZSTD_decompress`` returned ("ret": the size, or the error's name) and its output
(base64) where it returned that size: every truncation of two small frames, and single-byte changes of every
frame-header, block-header, literals-header and sequences-header byte of two more, and two changes inside a
sequence bitstream (``IN_BITSTREAM``).  "handmade": frames written by hand (``HANDMADE``) with libzstd's verdict
and output, for what no single-byte change reaches.  A record with "stricter" is
one that libzstd accepts and this project's decoders refuse, with the RFC 8878 section that states the rule; the
generator asserts that they stay below 5 % of the records.  "coverage": how often tests/zstd_ref.py reaches each
feature of the format over all the cases' frames; "not_reached": the features libzstd wrote for none of them.
"""
import base64
import ctypes as C
import hashlib
import json
import sys
from collections import Counter
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

SENTENCE = b"The quick brown fox jumps over the lazy dog while the archive grows by one more block. "
FRAME_KEYS = ("l1", "l3", "l19", "windowed", "checksum")


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
    if kind == "sandwich":  # random, other random, the first again
        a = rnd(spec["seed"], spec["edge"])
        return a + rnd(spec["seed"] + 1, spec["middle"]) + a
    if kind == "prefixes":  # sentence prefixes of 5..79 bytes, each followed by its length byte
        lens = np.random.default_rng(spec["seed"]).integers(5, 80, spec["count"])
        return b"".join(SENTENCE[:n] + bytes([n]) for n in lens)[:spec.get("cut")]  # (cut: so many bytes of them)
    if kind == "marked_copies":  # random bytes, then pieces of them again with `mark` between the pieces
        a = rnd(spec["seed"], spec["length"])
        rng = np.random.default_rng(spec["seed"] + 1)
        out = [a]
        for _ in range(spec["count"]):
            at = int(rng.integers(0, len(a) - spec["piece"]))
            out.append(a[at:at + spec["piece"]] + bytes.fromhex(spec["mark"]))
        return b"".join(out)
    if kind == "alternating":  # pieces of two kinds in turn: pulls matches from two or three recent offsets
        rng = np.random.default_rng(spec["seed"])
        a = [rnd(spec["seed"] + 1 + k, spec["piece"]) for k in range(3)]
        out = []
        for _ in range(spec["count"]):
            k = int(rng.integers(0, 3))
            cut = int(rng.integers(8, spec["piece"]))
            out.append(a[k][:cut] + rnd(int(rng.integers(1 << 30)), int(rng.integers(0, 3))))
        return b"".join(out)
    raise ValueError(kind)


def case_specs():
    return [
        ("empty", {"kind": "hex", "hex": ""}),
        ("single_byte", {"kind": "hex", "hex": "5a"}),
        ("zeros_300000", {"kind": "zeros", "length": 300000}),
        ("sentence_300000", {"kind": "sentence", "length": 300000}),
        ("below4_300000", {"kind": "random", "seed": 500, "length": 300000, "below": 4}),
        ("below64_20000", {"kind": "random", "seed": 501, "length": 20000, "below": 64}),
        ("sandwich", {"kind": "sandwich", "seed": 502, "edge": 5000, "middle": 400000}),
        ("prefixes_8000", {"kind": "prefixes", "seed": 503, "count": 8000}),
        # small frames, which the damaged list is made from
        ("sentence_400", {"kind": "sentence", "length": 400}),
        ("below4_700", {"kind": "random", "seed": 504, "length": 700, "below": 4}),
        ("prefixes_60", {"kind": "prefixes", "seed": 505, "count": 60}),
        ("below16_1500", {"kind": "random", "seed": 506, "length": 1500, "below": 16}),
        # tried for the features the inputs above do not reach
        ("marked_copies_20", {"kind": "marked_copies", "seed": 507, "length": 131072, "count": 20, "piece": 3000,
                              "mark": "7a"}),
        ("marked_copies_200", {"kind": "marked_copies", "seed": 508, "length": 131072, "count": 200, "piece": 600,
                               "mark": "7a"}),
        ("marked_copies_5000", {"kind": "marked_copies", "seed": 512, "length": 131072, "count": 5000, "piece": 24,
                                "mark": "7a"}),
        ("alternating", {"kind": "alternating", "seed": 509, "piece": 40, "count": 3000}),
        # a first block of 128 KiB and a short last one that leans on it: at level 19 the last block takes Repeat
        # for all three tables and 1-stream Treeless literals (the first), RLE for the literal lengths (the second)
        ("prefixes_cut_137572", {"kind": "prefixes", "seed": 530, "count": 8000, "cut": 137572}),
        ("prefixes_cut_131572", {"kind": "prefixes", "seed": 531, "count": 8000, "cut": 131572}),
        ("below256_2000", {"kind": "random", "seed": 511, "length": 2000}),
    ]


WINDOWED = ("sentence_300000",)
CHECKSUM = ("sentence_400", "below64_20000")
# the inputs tried for coverage hardly shrink below level 19: only that frame of theirs is kept
LEVEL_19_ONLY = ("marked_copies_20", "marked_copies_200", "marked_copies_5000", "alternating", "prefixes_cut_137572",
                 "prefixes_cut_131572")
# single-byte changes inside a sequence bitstream (base, at, byte) that libzstd accepts: bits left over, and a last
# sequence that reads past the stream's start
IN_BITSTREAM = (("below4_700", 79, 1), ("below4_700", 84, 5))
# frames written by hand (what, hex, content size), with a Window_Descriptor of 1 KiB and no content size: all three tables in RLE mode with a bitstream of the end mark
# alone ("abcd", then 4 literals and a match of 4 at repeat offset 1); and a Raw block "abcd", then a sequence
# without literals whose offset value 3 means repeat offset 1 minus 1, which is 0 at the start of a frame
HANDMADE = (
    ("RLE tables, end mark alone", "28b52ffd00005d00002061626364015404000101", 8),
    ("offset 0 through the repeat rule", "28b52ffd0000200000616263643d00000001540001" "0103", 8),
)
TRUNCATED = ("sentence_400", "below4_700")
CHANGED = ("prefixes_60", "below16_1500")


def b64(b: bytes) -> str:
    return base64.b64encode(b).decode()


_bin = None  # the bytes of zstd_kat.bin: what the frames hold besides pieces of their inputs


def text(b: bytes):
    """Bytes as JSON: {"bin": [start, length]}, a piece of zstd_kat.bin (appended to it here)."""
    global _bin
    if _bin is None:
        _bin = bytearray()
    _bin += b
    return {"bin": [len(_bin) - len(b), len(b)]}


def untext(t) -> bytes:
    global _bin
    if _bin is None:
        _bin = bytearray((HERE / "zstd_kat.bin").read_bytes())
    return bytes(_bin[t["bin"][0]:t["bin"][0] + t["bin"][1]])


def pack_frame(frame: bytes, data: bytes, spans) -> list:
    """A valid frame as a list of parts: ``text`` values (pieces of zstd_kat.bin), and [start, length] for a Raw
    block or a raw literal run of 48 bytes or more, which is data[start : start + length].  Keeps the frames of
    inputs that hardly compress out of the files; ``unpack_frame`` puts them back."""
    parts, done = [], 0
    for at, out_at, n in spans:
        if n >= 48:
            assert frame[at:at + n] == data[out_at:out_at + n]
            parts += [text(frame[done:at]), [out_at, n]]
            done = at + n
    if done < len(frame) or not parts:
        parts.append(text(frame[done:]))
    return parts


def unpack_frame(parts, data: bytes) -> bytes:
    return b"".join(data[p[0]:p[0] + p[1]] if isinstance(p, list) else untext(p) for p in parts)


def damaged_what(rec) -> str:
    return f"{rec['base']} cut to {rec['cut']}" if "cut" in rec else f"{rec['base']} byte {rec['at']} = {rec['byte']:#04x}"


def damaged_frame(rec, l3_frames) -> bytes:
    """The frame of a "damaged" record: a case's "l3" frame cut to "cut" bytes or with the byte at "at" set to
    "byte"."""
    s = l3_frames[rec["base"]]
    return s[:rec["cut"]] if "cut" in rec else s[:rec["at"]] + bytes([rec["byte"]]) + s[rec["at"] + 1:]


def main():
    sys.path.insert(0, str(HERE.parent))
    import zstd_ref as R

    L = C.CDLL("libzstd.so.1")
    L.ZSTD_versionString.restype = C.c_char_p
    L.ZSTD_getErrorName.restype = C.c_char_p
    L.ZSTD_getErrorName.argtypes = [C.c_size_t]
    L.ZSTD_isError.argtypes = [C.c_size_t]
    L.ZSTD_compressBound.restype = C.c_size_t
    L.ZSTD_compressBound.argtypes = [C.c_size_t]
    L.ZSTD_compress.restype = C.c_size_t
    L.ZSTD_compress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    L.ZSTD_decompress.restype = C.c_size_t
    L.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.ZSTD_createCCtx.restype = C.c_void_p
    L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    L.ZSTD_CCtx_setParameter.restype = C.c_size_t
    L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ZSTD_compress2.restype = C.c_size_t
    L.ZSTD_compress2.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    ZSTD_c_compressionLevel, ZSTD_c_windowLog, ZSTD_c_checksumFlag = 100, 101, 201  # (zstd.h's enum values)

    def compress(data, level):
        cap = L.ZSTD_compressBound(len(data))
        buf = C.create_string_buffer(cap)
        n = L.ZSTD_compress(buf, cap, data, len(data), level)
        assert not L.ZSTD_isError(n)
        return buf.raw[:n]

    def compress2(data, params):
        cctx = L.ZSTD_createCCtx()
        for k, v in params:
            assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, k, v))
        cap = L.ZSTD_compressBound(len(data))
        buf = C.create_string_buffer(cap)
        n = L.ZSTD_compress2(cctx, buf, cap, data, len(data))
        assert not L.ZSTD_isError(n)
        L.ZSTD_freeCCtx(cctx)
        return buf.raw[:n]

    def decompress(frame, n):
        buf = C.create_string_buffer(max(n, 1))
        r = L.ZSTD_decompress(buf, n, frame, len(frame))
        if L.ZSTD_isError(r):
            return L.ZSTD_getErrorName(r).decode(), b""
        return int(r), buf.raw[:r]

    cases, l3, inputs = [], {}, {}
    coverage = Counter()
    for name, spec in case_specs():
        data = input_bytes(spec)
        frames = {"l1": compress(data, 1), "l3": compress(data, 3), "l19": compress(data, 19)}
        if name in LEVEL_19_ONLY:
            frames = {"l19": frames["l19"]}
        if name in WINDOWED:
            frames["windowed"] = compress2(data, [(ZSTD_c_compressionLevel, 3), (ZSTD_c_windowLog, 17)])
            assert not R.frame_info(frames["windowed"]).single_segment
        if name in CHECKSUM:
            frames["checksum"] = compress2(data, [(ZSTD_c_compressionLevel, 3), (ZSTD_c_checksumFlag, 1)])
            assert R.frame_info(frames["checksum"]).checksum
        l3[name], inputs[name] = frames.get("l3"), data
        case = {"name": name, "spec": spec, "size": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        for key, s in frames.items():
            assert decompress(s, len(data)) == (len(data), data)
            trace = {}
            assert R.decode(s, coverage, trace=trace) == data, (name, key)
            case[key] = pack_frame(s, data, trace["spans"])
            case[key + "_sha256"] = hashlib.sha256(s).hexdigest()
            assert unpack_frame(case[key], data) == s
        cases.append(case)
        print(name, {k: len(v) for k, v in frames.items()}, file=sys.stderr)

    # what was seen on the development machine with libzstd 1.4.8: each must stay reached
    for key in R.FEATURES:
        assert key in NOT_REACHED or coverage[key] > 0, key
    not_reached = [k for k in R.FEATURES if coverage[k] == 0]

    damaged = []

    def add(what, how):
        frame, n = damaged_frame(how, l3), len(inputs[how["base"]])
        r, out = decompress(frame, n)
        rec = dict(how, ret=r)  # (offered n = the input's size; ``damaged_what`` names the record)
        if r == n:
            rec["out"] = b64(out)
        try:
            ours = R.decode(frame, size=n)
        except R.ZstdError as e:
            ours = None
            if r == n:
                rec["stricter"] = STRICTER[str(e)]  # (a KeyError here is a disagreement that needs looking at)
        else:
            assert r == n and ours == out, (what, r)
        damaged.append(rec)

    for name in TRUNCATED:
        for cut in range(len(l3[name])):
            add(f"{name} cut to {cut}", {"base": name, "cut": cut})
    for name in CHANGED:
        s, trace = l3[name], {}
        R.decode(s, trace=trace)
        for at in sorted(trace["spots"]):
            for v in sorted({s[at] ^ 0x01, s[at] ^ 0x10, s[at] ^ 0x80, 0x00, 0xFF} - {s[at]}):
                add(f"{name} byte {at} = {v:#04x}", {"base": name, "at": at, "byte": v})
    for base, at, byte in IN_BITSTREAM:
        add(f"{base} byte {at} = {byte:#04x}", {"base": base, "at": at, "byte": byte})
        assert "stricter" in damaged[-1], (base, at, byte)
    handmade = []
    for what, hexed, n in HANDMADE:
        frame = bytes.fromhex(hexed)
        r, out = decompress(frame, n)
        assert r == n, (what, r)  # libzstd accepts them all
        rec = {"what": what, "frame": hexed, "n": n, "ret": r, "out": b64(out)}
        try:
            assert R.decode(frame, size=n) == out, what
        except R.ZstdError as e:
            rec["stricter"] = STRICTER[str(e)]
        handmade.append(rec)
    assert [("stricter" in h) for h in handmade] == [False, True]
    stricter = sum(1 for d in damaged + handmade if "stricter" in d)
    assert 20 * stricter <= len(damaged), (stricter, len(damaged))

    cov = {k: coverage[k] for k in R.FEATURES}
    lines = [json.dumps(r, separators=(",", ":")) for r in cases + damaged + handmade]  # one record per line
    (HERE / "zstd_kat.json").write_text(
        '{"version":%s,\n"coverage":%s,\n"not_reached":%s,\n"cases":[\n%s\n],\n"damaged":[\n%s\n],\n"handmade":[\n%s\n]}\n' %
        (json.dumps(L.ZSTD_versionString().decode()), json.dumps(cov, separators=(",", ":")),
         json.dumps(not_reached), ",\n".join(lines[:len(cases)]), ",\n".join(lines[len(cases):len(cases) + len(damaged)]), ",\n".join(lines[len(cases) + len(damaged):])))
    (HERE / "zstd_kat.bin").write_bytes(bytes(_bin))
    print(f"{len(cases)} cases, {len(damaged)} damaged frames ({stricter} stricter), "
          f"libzstd {L.ZSTD_versionString().decode()}; not reached: {not_reached}")


# the features libzstd 1.4.8 wrote for none of the inputs tried; every other feature must stay reached.  An 8-byte
# content size needs 4 GiB and a 3-byte sequence count 32512 sequences in one block; RLE literals in the 1-byte
# format need 7..31 equal literals behind a block that left a Huffman table (below 7 they are stored raw); an RLE
# offset table needs every offset of a block in one power-of-two range.  The HANDMADE frame has all three tables
# in RLE mode.
NOT_REACHED = ("literals:rle:0", "of:rle", "seqcount:3byte", "fcs_bytes:8")

# the reader's refusals of frames that libzstd 1.4.8 accepts, and where RFC 8878 states the rule
STRICTER = {
    "offset 0 through the repeat rule": "3.1.1.5",
    "sequence bits left over": "3.1.1.3.2.1.1",
    "sequence bits overrun": "3.1.1.3.2.1.1",
    "reserved mode bits": "3.1.1.3.2.1",
}


if __name__ == "__main__":
    main()
