"""CPU tests of the Zstandard block decoder (no GPU needed): the host restatement of the kernels against libzstd's
recorded frames and its verdicts on damaged ones (tests/golden/zstd_kat.json) and against an independent reader
of the format (tests/zstd_ref.py); the frame header, the block count, the Python classes and their errors."""

import ctypes as C
import hashlib
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import zstd_cases as ZC
import zstd_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import zstd as Z

ROOT = Path(__file__).resolve().parent.parent
GUARD = 32


def guarded_host_decode(frame: bytes, n: int):
    """rpp_zstd_host_decode into a buffer with guard bytes on both sides: (status, output, guards intact)."""
    src = np.frombuffer(bytes(frame) + b"\0", np.uint8)
    buf = np.full(n + 2 * GUARD, 0xA5, np.uint8)
    st = N.lib().rpp_zstd_host_decode(src.ctypes.data_as(C.c_void_p), len(src) - 1,
                                      C.c_void_p(buf.ctypes.data + GUARD), n)
    return st, buf[GUARD:GUARD + n].tobytes(), bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + n:] == 0xA5).all())


def test_fixture_records_the_library_and_the_shapes_checked_by_hand():
    assert ZC.kat()["version"].startswith("1.")
    by_name = {name: (data, frames) for name, data, frames in ZC.cases()}
    kinds = lambda f: [k for k, *_ in R.block_headers(f)]  # noqa: E731
    for name in ("empty", "single_byte"):
        assert all(kinds(f) == [0] for f in by_name[name][1].values()), name
    assert kinds(by_name["zeros_300000"][1]["l3"]) == [2, 1, 1]
    assert kinds(by_name["sandwich"][1]["l3"])[:3] == [0, 0, 0]
    assert set(by_name["sentence_300000"][1]) == {"l1", "l3", "l19", "windowed"}
    assert not R.frame_info(by_name["sentence_300000"][1]["windowed"]).single_segment
    assert R.frame_info(by_name["sentence_400"][1]["checksum"]).checksum


def test_decoders_reproduce_every_case():
    for name, frame, data in ZC.frames():
        want = hashlib.sha256(data).hexdigest()
        assert hashlib.sha256(R.decode(frame)).hexdigest() == want, name
        st, out, intact = guarded_host_decode(frame, len(data))
        assert (st, intact) == (N.RPP_OK, True), name
        assert hashlib.sha256(out).hexdigest() == want, name


def test_frame_info_and_count_blocks_agree_with_the_reader():
    for name, frame, data in ZC.frames():
        want = R.frame_info(frame)
        got = Z.frame_info(frame)
        assert (got.header_bytes, got.content_size, got.window) == (want.header_bytes, want.content_size, want.window), name
        assert bool(got.flags & Z.FLAG_SINGLE_SEGMENT) == want.single_segment, name
        assert bool(got.flags & Z.FLAG_CHECKSUM) == want.checksum, name
        assert got.content_size == len(data), name
        assert Z.count_blocks(frame) == R.count_blocks(frame), name
    for what, frame, n, *_ in ZC.damaged():
        try:
            want = R.count_blocks(frame)
        except R.ZstdError:
            want = N.RPP_CORRUPT_INPUT
        assert Z.count_blocks(frame) == want, what


def test_damaged_frames():
    damaged = ZC.damaged()
    assert len(damaged) > 400
    # each of the three rules that libzstd does not enforce has a record, and the RLE tables an accepted one
    assert {d[5] for d in damaged if d[5]} == {"3.1.1.3.2.1", "3.1.1.3.2.1.1", "3.1.1.5"}
    assert any(d[0] == "RLE tables, end mark alone" and d[3] and not d[5] for d in damaged)
    stricter = [d for d in damaged if d[5]]
    assert 20 * len(stricter) <= len(damaged)
    for what, frame, n, accepted, want, rule in damaged:
        st, out, intact = guarded_host_decode(frame, n)
        assert intact, what
        try:
            ref = R.decode(frame, size=n)
        except R.ZstdError:
            ref = None
        if accepted and not rule:
            assert st == N.RPP_OK and out == want and ref == want, what
        else:  # libzstd returned an error, or the RFC states a rule that it does not enforce
            assert st == N.RPP_CORRUPT_INPUT and ref is None, what


def test_coverage_counts_match_a_recount():
    stats = Counter()
    for _, frame, _ in ZC.frames():
        R.decode(frame, stats)
    kat = ZC.kat()
    assert {k: stats[k] for k in R.FEATURES} == kat["coverage"]
    assert kat["not_reached"] == [k for k in R.FEATURES if stats[k] == 0]
    for k in ("block:raw", "block:rle", "block:compressed", "literals:compressed:0", "literals:compressed:3",
              "literals:treeless:2", "weights:direct", "weights:fse", "ll:fse", "of:predefined", "rep:3:ll0",
              "offset_beyond_128k", "frame:windowed", "frame:checksum", "literals:treeless:0", "ll:repeat", "of:repeat",
              "ml:repeat", "ll:rle"):
        assert stats[k] > 0, k


def test_decode_rejects_what_the_contract_names():
    by_name = {name: (data, frames) for name, data, frames in ZC.cases()}
    data, frames = by_name["sentence_400"]
    ok = frames["l3"]
    assert Z.host_decode(ok, len(data)) == (N.RPP_OK, data)
    assert Z.host_decode(ok, len(data) - 1)[0] == N.RPP_CORRUPT_INPUT  # not the stated size
    assert Z.host_decode(ok + b"\0", len(data))[0] == N.RPP_CORRUPT_INPUT  # a byte behind the frame
    assert Z.host_decode(ok + ok, len(data))[0] == N.RPP_CORRUPT_INPUT  # a second frame
    assert Z.host_decode(bytes.fromhex("502a4d1804000000") + b"abcd" + ok, len(data))[0] == N.RPP_CORRUPT_INPUT  # skippable
    checked = frames["checksum"]
    assert Z.host_decode(checked, len(data)) == (N.RPP_OK, data)
    assert Z.host_decode(checked[:-1], len(data))[0] == N.RPP_CORRUPT_INPUT  # 3 bytes of checksum
    flipped = checked[:-1] + bytes([checked[-1] ^ 0xFF])
    assert Z.host_decode(flipped, len(data)) == (N.RPP_OK, data)  # the checksum is skipped, not verified
    # a sequence count of 0 takes the single byte 0: written in two bytes it is refused by all three readers
    assert Z.host_decode(ZC.COUNT_0_IN_TWO_BYTES, 4)[0] == N.RPP_CORRUPT_INPUT
    with pytest.raises(R.ZstdError, match="a count of 0 in two bytes"):
        R.decode(ZC.COUNT_0_IN_TWO_BYTES, size=4)
    plain = ZC.COUNT_0_IN_TWO_BYTES[:6] + bytes([0x35]) + ZC.COUNT_0_IN_TWO_BYTES[7:14] + b"\0"  # the count as one byte
    assert Z.host_decode(plain, 4) == (N.RPP_OK, b"abcd") and R.decode(plain, size=4) == b"abcd"
    # a Dictionary_ID of 0 is accepted, any other is refused: the field goes behind the descriptor byte
    assert ok[4] & 3 == 0
    for did, st in ((0, N.RPP_OK), (7, N.RPP_CORRUPT_INPUT)):
        frame = ok[:4] + bytes([ok[4] | 1]) + bytes([did]) + ok[5:]
        assert Z.host_decode(frame, len(data))[0] == st, did
    # a frame without Frame_Content_Size: a Window_Descriptor takes the field's place
    assert ok[4] == 0x20 | 0x40 and len(data) == 400  # single segment, a 2-byte content size of 400 - 256
    no_size = ok[:4] + bytes([0x00, 0x00]) + ok[7:]  # window 1 KiB
    assert Z.host_decode(no_size, len(data)) == (N.RPP_OK, data)
    with pytest.raises(RuntimeError, match="^ZSTD content size unknown$"):
        Z.ZstdBlockDecompressor(no_size, "cpu")


def test_decompressor_on_the_cpu_and_the_three_errors():
    by_name = {name: (data, frames) for name, data, frames in ZC.cases()}
    data, frames = by_name["prefixes_8000"]
    dec = Z.ZstdBlockDecompressor(frames["l19"], "cpu")
    assert (dec.type(), dec.uncompressed_size(), dec.metadata()) == (2, len(data), None)
    target = bytearray()
    with pytest.raises(RuntimeError, match="decompression not started"):
        dec.decompress_frame()
    dec.start_decompression(target)
    assert dec.decompress_frame() and bytes(target) == data and not dec.decompress_frame()
    small = [by_name[n] for n in ("sentence_400", "below4_700", "empty", "zeros_300000")]
    assert Z.decompress_many([Z.ZstdBlockDecompressor(f["l3"], "cpu") for _, f in small], "cpu") == [d for d, _ in small]
    assert Z.decompress(by_name["below64_20000"][1]["checksum"], "cpu") == by_name["below64_20000"][0]
    with pytest.raises(RuntimeError, match="^ZSTD content size error$"):
        Z.ZstdBlockDecompressor(b"\x28\xb5\x2f", "cpu")
    with pytest.raises(RuntimeError, match="^ZSTD content size error$"):
        Z.ZstdBlockDecompressor(b"\x00" + frames["l3"][1:], "cpu")
    with pytest.raises(RuntimeError, match=r"^failed to decompress frame \(zstd error: -8\)$"):
        Z.decompress(frames["l3"][:-3], "cpu")
    with pytest.raises(RuntimeError, match="unknown compression: zstd"):
        block_codec.block_compressor("zstd")  # there is no encoder


def test_abi_edges():
    L = N.lib()
    assert L.rpp_zstd_decode_batch(None, None, None, 0, None, None, None, None, 0, None, 0, None) == N.RPP_OK
    assert L.rpp_zstd_decode_workspace_bytes(3000, 4) > L.rpp_zstd_decode_workspace_bytes(0, 4) > 0
    assert L.rpp_zstd_frame_info(None, 0, None, None, None) == N.RPP_CORRUPT_INPUT
    assert L.rpp_zstd_count_blocks(None, 0) == N.RPP_CORRUPT_INPUT


def test_cpp_host_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/zstd_test.cpp: the host functions alone in a program of their own, built with AddressSanitizer
    and UBSan, over every fixture frame and every damaged one (exact-size heap buffers, so a byte read or
    written outside them is reported)."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_zstd.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "zstd_vectors.bin"
    with open(vec, "wb") as f:
        def rec(n, expect, a, b=b""):
            f.write(np.array([n, expect, len(a), len(b)], "<i8").tobytes() + a + b)
        for _, frame, data in ZC.frames():
            rec(len(data), 1, frame, data)
        for _, frame, n, accepted, want, rule in ZC.damaged():
            ok = accepted and not rule
            rec(n, 1 if ok else 0, frame, want if ok else b"")
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "zstd_test"), str(vec)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "zstd_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
