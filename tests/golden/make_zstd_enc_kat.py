"""Writes tests/golden/zstd_enc_kat.json: what libzstd says about the frames of this project's Zstandard encoder.

    python tests/golden/make_zstd_enc_kat.py

Runs on the development machine only: it loads ``libzstd.so.1`` and ``liblz4.so.1`` with ctypes (there are no
headers) and needs the built library.  The tests read the JSON and need neither.

"version": ZSTD_versionString().  "cases": per input of tests/zstd_enc_cases.py its name, size and SHA-256, the
size and SHA-256 of ``rpp_zstd_host_encode``'s frame, what ``ZSTD_decompress`` returned for it ("decompressed":
the input's size, and the bytes were compared with the input here), ``ZSTD_getFrameContentSize``, and for
comparison, not asserted anywhere, the sizes of this project's LZ4 block ("lz4") and of libzstd's level-1 frame
("zstd1") of the same input: with predefined tables an input of far offsets and short literal runs can come out
larger than its LZ4 block.
"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))


def main():
    import zstd_enc_cases as EC
    from dwarfs_amd import lz4, zstd

    Z = C.CDLL("libzstd.so.1")
    Z.ZSTD_versionString.restype = C.c_char_p
    Z.ZSTD_decompress.restype = C.c_size_t
    Z.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    Z.ZSTD_compress.restype = C.c_size_t
    Z.ZSTD_compress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    Z.ZSTD_compressBound.restype = C.c_size_t
    Z.ZSTD_compressBound.argtypes = [C.c_size_t]
    Z.ZSTD_isError.argtypes = [C.c_size_t]
    Z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    Z.ZSTD_getFrameContentSize.argtypes = [C.c_char_p, C.c_size_t]
    cases = []
    for name, data in EC.inputs():
        frame, _ = zstd.host_encode(data)
        buf = C.create_string_buffer(max(len(data), 1))
        r = Z.ZSTD_decompress(buf, len(data), frame, len(frame))
        assert not Z.ZSTD_isError(r) and r == len(data) and buf.raw[:len(data)] == data, name
        cap = Z.ZSTD_compressBound(len(data))
        out = C.create_string_buffer(cap)
        z1 = Z.ZSTD_compress(out, cap, data, len(data), 1)
        assert not Z.ZSTD_isError(z1), name
        cases.append({"name": name, "size": len(data), "sha256": hashlib.sha256(data).hexdigest(),
                      "frame_size": len(frame), "frame_sha256": hashlib.sha256(frame).hexdigest(),
                      "decompressed": int(r), "content_size": int(Z.ZSTD_getFrameContentSize(frame, len(frame))),
                      "lz4": len(lz4.host_encode(data)[0]), "zstd1": int(z1)})
    lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)
    (HERE / "zstd_enc_kat.json").write_text('{"version":%s,\n"cases":[\n%s\n]}\n' %
                                            (json.dumps(Z.ZSTD_versionString().decode()), lines))
    print(f"{len(cases)} cases, libzstd {Z.ZSTD_versionString().decode()}")


if __name__ == "__main__":
    main()
