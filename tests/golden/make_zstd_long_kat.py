"""Writes tests/golden/zstd_long_kat.json: what libzstd says about the frames that this project's Zstandard encoder
writes with its `long` word (long = 1: matches against anything earlier in the same block).

    python tests/golden/make_zstd_long_kat.py

Runs on the development machine only: it loads ``libzstd.so.1`` with ctypes (there are no headers) and needs the
built library.  The tests read the JSON and need neither.

"version": ZSTD_versionString().  "pairs": the (options, search) pairs.  "cases": per input of
tests/zstd_long_cases.py (its own families, then the 116 inherited ones, then the 1.5 MiB input under the one pair
(3, 0)) its name, size and SHA-256; under "options,search" the size and SHA-256 of ``rpp_zstd_host_encode_long``'s
long = 1 frame, what ``ZSTD_decompress`` returned for it ("decompressed": the input's size, and the bytes were
compared with the input here) and "growth", the frame's size minus the long = 0 frame's; and "zstd_1" and
"zstd_1_long", libzstd level 1's size without and with its own long-distance matcher (window: the block).  Growth and
libzstd's sizes are recorded, not asserted.
"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

ZSTD_c_compressionLevel, ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching = 100, 101, 160


def main():
    import zstd_long_cases as LC
    from dwarfs_amd import zstd

    Z = C.CDLL("libzstd.so.1")
    Z.ZSTD_versionString.restype = C.c_char_p
    Z.ZSTD_decompress.restype = C.c_size_t
    Z.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    Z.ZSTD_isError.argtypes = [C.c_size_t]
    Z.ZSTD_compressBound.restype = C.c_size_t
    Z.ZSTD_compressBound.argtypes = [C.c_size_t]
    Z.ZSTD_createCCtx.restype = C.c_void_p
    Z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    Z.ZSTD_CCtx_setParameter.restype = C.c_size_t
    Z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    Z.ZSTD_compress2.restype = C.c_size_t
    Z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]

    def level_1(data, long):
        ctx = Z.ZSTD_createCCtx()
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(ctx, ZSTD_c_compressionLevel, 1))
        if long:  # zstd.cpp:404-406: the matcher on, the window the block (libzstd's floor is 10)
            assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(ctx, ZSTD_c_enableLongDistanceMatching, 1))
            log = max(10, (max(len(data), 1) - 1).bit_length())
            assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(ctx, ZSTD_c_windowLog, log))
        cap = Z.ZSTD_compressBound(len(data))
        buf = C.create_string_buffer(cap)
        r = Z.ZSTD_compress2(ctx, buf, cap, data, len(data))
        Z.ZSTD_freeCCtx(ctx)
        assert not Z.ZSTD_isError(r)
        return int(r)

    def record(name, data, pairs):
        rec = {"name": name, "size": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        for options, search in pairs:
            frame, _ = zstd.host_encode(data, options, search, 1)
            buf = C.create_string_buffer(max(len(data), 1))
            r = Z.ZSTD_decompress(buf, len(data), frame, len(frame))
            assert not Z.ZSTD_isError(r) and r == len(data) and buf.raw[:len(data)] == data, (name, options, search)
            rec[f"{options},{search}"] = {"frame_size": len(frame), "frame_sha256": hashlib.sha256(frame).hexdigest(),
                                          "decompressed": int(r),
                                          "growth": len(frame) - len(zstd.host_encode(data, options, search, 0)[0])}
        rec["zstd_1"], rec["zstd_1_long"] = level_1(data, 0), level_1(data, 1)
        return rec

    cases = [record(name, data, LC.PAIRS) for name, data in LC.inputs()]
    cases.append(record("reach_20", LC.reach_20(), ((3, 0),)))
    lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)
    (HERE / "zstd_long_kat.json").write_text(
        '{"version":%s,\n"pairs":%s,\n"cases":[\n%s\n]}\n' %
        (json.dumps(Z.ZSTD_versionString().decode()), json.dumps([list(p) for p in LC.PAIRS]), lines))
    grew = sum(1 for c in cases for k, v in c.items() if isinstance(v, dict) and v["growth"] > 0)
    print(f"{len(cases)} cases, libzstd {Z.ZSTD_versionString().decode()}, {grew} frames grew")


if __name__ == "__main__":
    main()
