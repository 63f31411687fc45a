"""CPU tests of the Zstandard block encoder (no GPU needed): the host restatement of the kernels over the inputs
of tests/zstd_enc_cases.py.  Every frame is read by three readers: libzstd 1.4.8, whose verdict on these very bytes
tests/golden/zstd_enc_kat.json records under their SHA-256, the independent reader tests/zstd_ref.py, and this
project's rpp_zstd_host_decode.  Then what of the format the inputs reach, the Python layer, the ABI's edges, and
the host functions alone under AddressSanitizer and UBSan."""

import ctypes as C
import functools
import hashlib
import json
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import lz4_ref
import zstd_enc_cases as EC
import zstd_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import lz4
from dwarfs_amd import zstd as Z

ROOT = Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((ROOT / "tests" / "golden" / "zstd_enc_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def encoded():
    """[(name, input, frame, flag)], computed once"""
    return [(name, data, *Z.host_encode(data)) for name, data in EC.inputs()]


def test_every_input_three_readers():
    records = kat()["cases"]
    assert kat()["version"] == "1.4.8" and [r["name"] for r in records] == [c[0] for c in encoded()]
    for rec, (name, data, frame, _) in zip(records, encoded()):
        assert (rec["size"], rec["sha256"]) == (len(data), hashlib.sha256(data).hexdigest()), name
        # libzstd decoded the frame with this SHA-256 to the input, and read its content size
        assert (rec["frame_size"], rec["frame_sha256"]) == (len(frame), hashlib.sha256(frame).hexdigest()), name
        assert rec["decompressed"] == rec["content_size"] == len(data), name
        assert R.decode(frame) == data, name
        assert Z.host_decode(frame, len(data)) == (N.RPP_OK, data), name
        info = Z.frame_info(frame)
        assert info.content_size == len(data) and info.flags & Z.FLAG_SINGLE_SEGMENT, name
        assert not info.flags & Z.FLAG_CHECKSUM, name


def test_size_and_flag():
    for name, data, frame, flag in encoded():
        assert len(frame) <= Z.bound(len(data)), name
        assert flag == (len(frame) >= len(data)), name
        assert len(R.block_headers(frame)) == max(1, -(-len(data) // EC.CHUNK)), name  # one block per chunk


def huf_lengths(hist):
    """The code-length rule of zstd_enc_common.h's huf_lengths, restated."""
    total, full = sum(hist), 1 << 11
    lens = [0] * 256
    for s, c in enumerate(hist):
        if c:
            lens[s] = next(l for l in range(1, 12) if l == 11 or (c << l) >= total)
    k = lambda: sum(1 << (11 - l) for l in lens if l)  # noqa: E731
    while k() > full:
        for l in range(10, 0, -1):
            for s in range(256):
                if lens[s] == l and k() > full:
                    lens[s] = l + 1
    while k() < full:
        for l in range(2, 12):
            for s in range(256):
                if lens[s] == l and (1 << (11 - l)) <= full - k():
                    lens[s] = l - 1
    return lens


def test_format_reach():
    stats, seen = Counter(), {}
    for name, data, frame, _ in encoded():
        assert R.decode(frame, stats) == data
        seen[name] = EC.sections(frame)
    every = [s for secs in seen.values() for s in secs]
    for key in ("block:raw", "block:compressed",
                "literals:raw:0", "literals:raw:1", "literals:raw:3",        # the three Raw header widths
                "literals:rle:0", "literals:rle:1",
                "literals:compressed:0", "literals:compressed:2", "literals:compressed:3",
                "weights:direct", "weights:fse", "seqcount:zero", "seqcount:1byte", "seqcount:2byte",
                "ll:predefined", "of:predefined", "ml:predefined", "fcs_bytes:1", "fcs_bytes:2", "fcs_bytes:4"):
        assert stats[key] > 0, key
    # Size format 1 is four streams with both sizes below 1024, and up to 1023 literals go into one stream: the
    # definition leaves it no input.  The encoder must never write it.
    assert stats["literals:compressed:1"] == 0
    for key in R.FEATURES:  # nothing the format section rules out
        if key.startswith(("block:rle", "literals:treeless", "rep:", "frame:windowed", "frame:checksum", "fcs_bytes:8",
                           "seqcount:3byte")) or key.endswith((":rle", ":fse", ":repeat")) and key[:2] in ("ll", "of", "ml"):
            assert stats[key] == 0, key
    assert {s.streams for s in every if s.literals == 2} == {1, 4}
    assert {s.header_bytes for s in every if s.literals == 0} == {1, 2, 3}
    assert {s.header_bytes for s in every if s.literals == 2} == {3, 4, 5}
    assert {s.count_bytes for s in every if s.block == 2} == {1, 2}
    assert any(s.block == 2 and s.sequences == 0 and s.literals == 2 for s in every)  # wins through its literals
    # the counts around every boundary, in the second block of their input
    for t, sf, streams in ((1023, 0, 1), (1024, 2, 4), (4095, 2, 4), (4096, 2, 4), (16383, 2, 4), (16384, 3, 4)):
        s = seen[f"literals_{t}"][1]
        assert (s.literals, s.regenerated, s.size_format, s.streams) == (2, t, sf, streams), t
    for t, hb in ((31, 1), (32, 2), (4095, 2), (4096, 3)):
        s = seen[f"raw_literals_{t}"][1]
        assert (s.literals, s.regenerated, s.header_bytes) == (0, t, hb), t
    assert [seen[f"sequences_{t}"][0].sequences for t in (127, 128)] == [127, 128]
    assert [seen[f"sequences_{t}"][0].count_bytes for t in (127, 128)] == [1, 2]
    assert seen["abcd_chunk"][0].sequences > 200
    assert seen["one_byte_200"][0].literals == 1 and seen["two_symbols"][0].weights == "direct"
    # the fallback: every byte value equally often gives 8 bits each, so the 255 listed weights are all equal,
    # which the FSE form cannot state and the direct form cannot list; the literals are Raw (here: a Raw block)
    data = dict(EC.inputs())["permutations_512"]
    assert lz4_ref.walk(lz4.host_encode(data)[0])[0].offset is None  # no match: all 512 bytes are literals
    assert set(huf_lengths([data.count(bytes([v])) for v in range(256)])) == {8}
    assert seen["permutations_512"][0].block == 0
    # The largest offset code.  The search is the LZ4 encoder's, whose block states the offsets: a chunk's table
    # starts with the positions of the chunk before it and a match starts at least 4 bytes before its chunk's
    # end, so no offset is above 2 * chunk - 4 = 65532, whose value 65535 is the last of code 15: all 15 extra
    # bits set.  An offset code of 16 (offsets from 65533 on) cannot come out of this search.
    offsets = [q.offset for name, data in EC.inputs() for q in lz4_ref.walk(lz4.host_encode(data)[0]) if q.offset]
    assert max(offsets) == 2 * EC.CHUNK - 4 and (max(offsets) + 3).bit_length() - 1 == 15
    assert max(q.offset or 0 for q in lz4_ref.walk(lz4.host_encode(dict(EC.inputs())["offset_65532"])[0])) == 65532
    # offsets 1, 2 and 3 are written as the values 4 to 6, never as repeat codes (no "rep:" above), and LL codes
    # from 16 and ML codes from 32 on with extra bits come with the long runs and matches of the LZ4 inputs
    for period in (1, 2, 3):
        walked = lz4_ref.walk(lz4.host_encode(dict(EC.inputs())[f"period_{period}"])[0])
        assert [q.offset for q in walked if q.offset] == [period], period
    assert any(q.literals >= 16 for q in lz4_ref.walk(lz4.host_encode(dict(EC.inputs())["literal_run_269"])[0]))
    assert max(q.match or 0 for q in lz4_ref.walk(lz4.host_encode(dict(EC.inputs())["zeros_65536"])[0])) > 32000


def test_python_layer_on_the_cpu():
    by_name = dict(EC.inputs())
    comp = Z.ZstdBlockCompressor(device="cpu")
    assert (comp.type(), comp.describe(), comp.metadata_requirements()) == (2, "zstd [level=22]", "")
    assert comp.get_compression_constraints() == {} and comp.estimate_memory_usage(1000) == 1000
    assert comp.clone().describe() == comp.describe()
    for name in ("sentence_18000", "skewed_full_range", "zeros_70000", "source_in_previous_chunk"):
        frame = comp.compress(by_name[name])
        dec = Z.ZstdBlockDecompressor(frame, "cpu")
        target = bytearray()
        dec.start_decompression(target)
        assert dec.decompress_frame() and bytes(target) == by_name[name], name
    with pytest.raises(lz4.BadCompressionRatioError):
        comp.compress(by_name["random_5000"])
    many = comp.compress_many([by_name["sentence_18000"], by_name["random_5000"]], keep_bad=True)
    assert many[1] is None and Z.decompress(many[0], "cpu") == by_name["sentence_18000"]
    assert Z.block_compressor("zstd", "cpu").describe() == "zstd [level=22]"
    assert Z.block_compressor("zstd:level=3", "cpu").describe() == "zstd [level=3]"
    assert Z.block_compressor("zstd:level=-5", "cpu").describe() == "zstd [level=-5]"
    for spec, what in (("zstd:level=23", "level=23"), ("zstd:level=x", "level=x"), ("zstd:long=1", "long=1"),
                       ("zstd:level=3:window=9", "window=9")):
        with pytest.raises(RuntimeError, match=f"^invalid option\\(s\\) for zstd: {what}$"):
            Z.block_compressor(spec, "cpu")
    with pytest.raises(RuntimeError, match="unknown compression: zstd"):
        block_codec.block_compressor("zstd")  # the factory of block_codec is unchanged


def test_abi_edges():
    L = N.lib()
    assert L.rpp_zstd_encode_batch(None, None, None, 0, None, None, None, None, None, 0, None, 0, None) == N.RPP_OK
    assert L.rpp_zstd_encode_workspace_bytes(100000, 4) > L.rpp_zstd_encode_workspace_bytes(0, 4) > 0
    assert L.rpp_zstd_encode_workspace_bytes(100000, 4) > L.rpp_lz4_encode_workspace_bytes(100000, 4)
    assert [L.rpp_zstd_bound(n) for n in (0, 1, 32768, 32769)] == [12, 13, 32768 + 15, 32769 + 15]
    out = np.zeros(64, np.uint8)
    n, flag = C.c_uint64(), C.c_uint32()
    src = np.frombuffer(b"abcdefgh", np.uint8)
    args = (src.ctypes.data_as(C.c_void_p), 8, out.ctypes.data_as(C.c_void_p))
    assert L.rpp_zstd_host_encode(*args, L.rpp_zstd_bound(8) - 1, C.byref(n), C.byref(flag)) == N.RPP_OUTPUT_TOO_SMALL
    assert L.rpp_zstd_host_encode(*args, L.rpp_zstd_bound(8), C.byref(n), None) == N.RPP_OK and n.value == 17
    assert L.rpp_zstd_host_encode(None, 0, out.ctypes.data_as(C.c_void_p), 12, C.byref(n), C.byref(flag)) == N.RPP_OK
    assert out[:n.value].tobytes() == bytes.fromhex("28b52ffd2000010000") and flag.value == 1
    assert L.rpp_zstd_host_encode(None, 8, out.ctypes.data_as(C.c_void_p), 64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
    assert L.rpp_zstd_host_encode(*args[:2], None, 64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
    assert L.rpp_zstd_host_encode(*args, 64, None, None) == N.RPP_INVALID_ARGUMENT


def test_cpp_host_encoder_under_asan_ubsan(tmp_path):
    """tests/cpp/zstd_encode_test.cpp: host encode, then host decode, of every input in a program of its own,
    built with AddressSanitizer and UBSan, with exact-size heap buffers."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_zstd_encode.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "zstd_encode_vectors.bin"
    with open(vec, "wb") as f:
        for _, data, frame, _ in encoded():
            f.write(np.array([len(data), len(frame)], "<i8").tobytes() + data)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "zstd_encode_test"), str(vec)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "zstd_encode_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
