"""CPU tests of the LZ4 block codec (no GPU needed): the host restatements of the two kernels against liblz4's
recorded blocks (tests/golden/lz4_kat.json), against an independent reader of the format (tests/lz4_ref.py)
and, where liblz4.so.1 loads, against LZ4_decompress_safe itself; the framing, the factory and NONE sections."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lz4_cases as LC
import lz4_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import lz4 as Z
from dwarfs_amd import section as S

ROOT = Path(__file__).resolve().parent.parent
GUARD = 32


def guarded_host_decode(block: bytes, n: int):
    """rpp_lz4_host_decode into a buffer with guard bytes on both sides: (status, output, guards intact)."""
    src = np.frombuffer(bytes(block), np.uint8)
    buf = np.full(n + 2 * GUARD, 0xA5, np.uint8)
    st = N.lib().rpp_lz4_host_decode(src.ctypes.data_as(C.c_void_p), len(src),
                                     C.c_void_p(buf.ctypes.data + GUARD), n)
    return st, buf[GUARD:GUARD + n].tobytes(), bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + n:] == 0xA5).all())


def liblz4():
    try:
        L = C.CDLL("liblz4.so.1")
    except OSError:
        return None
    L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    return L


def test_fixture_records_the_library():
    assert LC.kat()["version"].startswith("1.")
    sizes = {name: (len(d), len(h)) for name, _, d, h in LC.cases()}
    # the sizes checked by hand against liblz4 1.9.3
    assert sizes["empty"] == (1, 1) and sizes["literals_12"] == (13, 13) and sizes["same_byte_13"] == (10, 10)
    assert sizes["zeros_65536"] == (267, 267) and sizes["zeros_70000"] == (285, 285)
    assert sizes["random_4096"] == (4114, 4114)


@pytest.mark.parametrize("which", ["default", "hc9"])
def test_decoders_read_liblz4_blocks(which):
    for name, data, d, h in LC.cases():
        block = d if which == "default" else h
        assert R.decode(block, len(data)) == data, name
        st, out, intact = guarded_host_decode(block, len(data))
        assert (st, intact) == (N.RPP_OK, True), name
        assert out == data, name


def test_damaged_blocks():
    assert len(LC.damaged()) > 100
    for what, block, n, ret, want in LC.damaged():
        st, out, intact = guarded_host_decode(block, n)
        assert intact, what
        try:
            ref = R.decode(block, n)
        except R.Lz4Error:
            ref = None
        if ret == n:
            assert st == N.RPP_OK and out == want and ref == want, what
        else:
            assert st in (N.RPP_OK, N.RPP_CORRUPT_INPUT), what
        assert (st == N.RPP_OK) == (ref is not None), what
        if what.startswith("offset 0 "):
            assert st == N.RPP_CORRUPT_INPUT, what
        if ref is not None:
            assert out == ref, what


def test_decode_rejects_what_the_contract_names():
    ok = bytes([0x44]) + b"abcd" + bytes([4, 0]) + bytes([0x50]) + b"vwxyz"  # 4 literals, match of 8, 5 literals
    assert Z.host_decode(ok, 17) == (N.RPP_OK, b"abcdabcdabcdvwxyz")
    assert Z.host_decode(ok, 16)[0] == N.RPP_CORRUPT_INPUT  # a copy would pass the stated size
    assert Z.host_decode(ok, 18)[0] == N.RPP_CORRUPT_INPUT  # the block ends before the stated size
    assert Z.host_decode(b"", 0)[0] == N.RPP_CORRUPT_INPUT  # no token at all
    assert Z.host_decode(b"\x00", 0) == (N.RPP_OK, b"")
    assert Z.host_decode(ok[:6], 17)[0] == N.RPP_CORRUPT_INPUT  # half an offset
    assert Z.host_decode(bytes([0xF0]), 15)[0] == N.RPP_CORRUPT_INPUT  # no extension byte


def test_host_encoder_on_every_input():
    L = liblz4()
    ratios = {}
    for name, data in LC.encoder_inputs():
        block, flag = Z.host_encode(data)
        n = len(data)
        assert R.decode(block, n) == data, name
        assert len(block) <= Z.bound(n), name
        assert flag == (4 + len(block) >= n), name
        R.check_end_rules(block, n)
        assert Z.host_decode(block, n) == (N.RPP_OK, data), name
        if L is not None:  # the real decoder, which enforces the end-of-block rules
            buf = C.create_string_buffer(max(n, 1))
            assert L.LZ4_decompress_safe(block, buf, len(block), n) == n, name
            assert buf.raw[:n] == data, name
        ratios[name] = len(block) / max(n, 1)
        assert Z.host_encode(data)[0] == block, name  # deterministic
    # a property of any LZ4 matcher on these (liblz4: 0.4 % and 0.7 %)
    for name in ("zeros_65536", "zeros_70000", "sentence_18000"):
        assert ratios[name] < 0.1, (name, ratios[name])


def test_encoder_finds_matches_across_chunks_but_no_offset_65536():
    by_name = dict(LC.encoder_inputs())
    chunk = N.lib().rpp_lz4_chunk_bytes()
    for name in ("repeat_across_chunks", "source_in_previous_chunk"):
        seqs = R.walk(Z.host_encode(by_name[name])[0])
        starts = [(s.out_at + s.literals, s.match, s.offset) for s in seqs if s.offset is not None]
        # the repeat is found on both sides of the boundary / from the chunk before
        assert sum(m for at, m, _ in starts if at < chunk) >= 100 or name != "repeat_across_chunks", starts
        assert sum(m for at, m, _ in starts if at >= chunk) >= 100, (name, starts)
    for s in R.walk(Z.host_encode(by_name["offset_65536"])[0]):
        assert s.offset is None or s.offset <= 65535


def test_bound_and_queries():
    L = N.lib()
    for n in (0, 1, 254, 255, 256, 65536, 1 << 30):
        assert L.rpp_lz4_bound(n) >= n + n // 255 + 16
    assert L.rpp_lz4_chunk_bytes() % L.rpp_lz4_step_positions() == 0
    big = np.zeros(16, np.uint8)
    n = C.c_uint64()
    assert L.rpp_lz4_host_encode(big.ctypes.data_as(C.c_void_p), 16, big.ctypes.data_as(C.c_void_p), 16, C.byref(n),
                                 None) == N.RPP_OUTPUT_TOO_SMALL
    assert L.rpp_lz4_host_encode(big.ctypes.data_as(C.c_void_p), (1 << 30) + 1, big.ctypes.data_as(C.c_void_p), 16,
                                 C.byref(n), None) == N.RPP_INVALID_ARGUMENT


def test_framing():
    assert Z.frame_header(0x01020304) == bytes([4, 3, 2, 1])
    assert Z.parse_frame(bytes([4, 3, 2, 1]) + b"rest") == (0x01020304, 4)
    for short in (b"", b"\x01", b"\x01\x02\x03"):
        buf = np.frombuffer(short + b"\0", np.uint8)
        assert N.lib().rpp_lz4_parse_frame(buf.ctypes.data_as(C.c_void_p), len(short), None) == N.RPP_TRUNCATED_INPUT
        with pytest.raises(RuntimeError, match="malformed LZ4 block header"):
            Z.Lz4BlockDecompressor(short)
    assert N.RPP_CORRUPT_INPUT == -8 and N.lib().rpp_abi_version() == 1


def test_factory_and_descriptions():
    c = block_codec.block_compressor("lz4", device="cpu")
    assert (c.type(), c.describe(), c.metadata_requirements()) == (3, "lz4", "")
    c = block_codec.block_compressor("lz4hc", device="cpu")
    assert (c.type(), c.describe()) == (4, "lz4hc [level=9]")
    for level in (0, 5, 12):
        c = block_codec.block_compressor(f"lz4hc:level={level}", device="cpu")
        assert (c.type(), c.describe(), c.level) == (4, f"lz4hc [level={level}]", level)
    assert block_codec.block_compressor("null").type() == 0
    assert block_codec.block_compressor("null").compress(b"abc") == b"abc"
    for spec, msg in (("lz4hc:level=13", "invalid option\\(s\\) for lz4hc: level=13"),
                      ("lz4hc:depth=3", "invalid option\\(s\\) for lz4hc: depth=3"),
                      ("lz4:level=3", "invalid option\\(s\\) for lz4: level=3"),
                      ("null:x=1", "invalid option\\(s\\) for null: x=1"),
                      ("zstd", "unknown compression: zstd"),
                      ("ricepp:level=3", "invalid option\\(s\\) for ricepp: level=3")):
        with pytest.raises(RuntimeError, match=msg):
            block_codec.block_compressor(spec)
    assert block_codec.block_compressor("ricepp:block_size=64").describe() == "ricepp [block_size=64]"


def test_ratio_rule_and_cpu_round_trip():
    comp = Z.Lz4BlockCompressor(device="cpu")
    by_name = dict(LC.encoder_inputs())
    with pytest.raises(Z.BadCompressionRatioError):
        comp.compress(by_name["random_4096"])
    for n in range(17):  # nothing this short shrinks by more than the 4-byte frame
        for data in (bytes(n), bytes(range(n))):
            block, flag = Z.host_encode(data)
            assert flag == (4 + len(block) >= n)
            if flag:
                with pytest.raises(Z.BadCompressionRatioError):
                    comp.compress(data)
            else:
                assert Z.decompress(comp.compress(data), "cpu") == data
    data = by_name["sentence_18000"]
    payload = comp.compress(data)
    assert payload[:4] == Z.frame_header(len(data)) and payload[4:] == Z.host_encode(data)[0]
    dec = Z.Lz4BlockDecompressor(payload, "cpu")
    assert dec.uncompressed_size() == len(data)
    target = bytearray()
    dec.start_decompression(target)
    assert dec.decompress_frame() and bytes(target) == data and not dec.decompress_frame()
    assert comp.compress_many([data, by_name["random_4096"]], keep_bad=True)[1] is None
    with pytest.raises(RuntimeError, match=r"^LZ4: decompression failed \(error: -8\)$"):
        Z.decompress(payload[:-3], "cpu")


def test_none_section_walks():
    """A NONE section as the writer stores a block that did not shrink: the v2 header, then the raw bytes."""
    import hashlib
    import struct

    data = dict(LC.encoder_inputs())["random_4096"]
    # section_header_v2 (include/dwarfs/fstypes.h:85-97); walk reads the layout, the checksums are the GPU's to verify
    image = (b"DWARFS" + bytes([2, 5]) + hashlib.sha512(data).digest()[:32] +
             struct.pack("<QIHHQ", 0, 7, S.SECTION_TYPE_BLOCK, Z.COMPRESSION_TYPE_NONE, len(data)) + data)
    secs, bad = S.walk(image)
    assert bad is None and len(secs) == 1
    at, h = secs[0]
    assert (at, h.type, h.compression, h.number, h.length) == (0, 0, 0, 7, len(data))
    assert image[at + S.HEADER_BYTES:at + S.HEADER_BYTES + h.length] == data


def test_cpp_host_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/lz4_test.cpp: the host functions alone in a program of their own, built with AddressSanitizer
    and UBSan, over the fixture's blocks and the damaged ones (exact-size heap buffers, so a byte read or
    written outside them is reported)."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_lz4.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "lz4_vectors.bin"
    with open(vec, "wb") as f:
        def rec(kind, n, expect, a, b=b""):
            f.write(np.array([kind, n, expect, len(a), len(b)], "<i8").tobytes() + a + b)
        for _, data, d, h in LC.cases():
            rec(0, len(data), 0, d, data)
            rec(0, len(data), 0, h, data)
        for _, block, n, ret, want in LC.damaged():
            rec(1, n, 1 if ret == n else 0, block, want or b"")
        for _, data in LC.encoder_inputs():
            rec(2, len(data), 0, data)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "lz4_test"), str(vec)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "lz4_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
