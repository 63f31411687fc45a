"""CPU tests of the Zstandard encoder's `long` word (no GPU needed): the host restatement over the inputs of
tests/zstd_long_cases.py.  The matcher is restated in plain Python there and compared sequence by sequence; every
long = 1 frame is read by libzstd 1.4.8, whose verdict tests/golden/zstd_long_kat.json records under the frame's
SHA-256, by the independent reader tests/zstd_ref.py and by rpp_zstd_host_decode; long = 0 is the old entry point's
bytes; then the sizes, the format reach, the categorizer, the Python layer, and the host functions alone under
AddressSanitizer and UBSan."""

import ctypes as C
import functools
import hashlib
import json
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import incompressible_cases as IC
import zstd_enc_adaptive_cases as AC
import zstd_long_cases as LC
import zstd_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import categorize as CZ
from dwarfs_amd import lz4
from dwarfs_amd import zstd as Z

ROOT = Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((ROOT / "tests" / "golden" / "zstd_long_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def encoded(options, search, long):
    """[(name, input, frame, flag)], computed once per word triple"""
    return [(name, data, *Z.host_encode(data, options, search, long)) for name, data in LC.inputs()]


def rows(data, search, long):
    return [tuple(r) for r in Z.host_sequences(data, search, long).tolist()]


def test_the_inputs():
    names = [name for name, _ in LC.inputs()]
    assert len(set(names)) == len(names) and len(AC.inputs()) == 116 and names[-116:] == [n for n, _ in AC.inputs()]
    assert [r["name"] for r in kat()["cases"]] == names + ["reach_20"] and kat()["version"] == "1.4.8"
    assert [tuple(p) for p in kat()["pairs"]] == list(LC.PAIRS)


@pytest.mark.parametrize("search", (0, 8 | lz4.SEARCH_LAZY))
def test_index_find_and_merge_sequence_by_sequence(search):
    """The plain-Python matcher and merge of zstd_long_cases.py against the host code's list, and the list against
    the sequences that the independent reader finds in the frame."""
    stats, far_offsets = Counter(), 0
    for name, data in LC.inputs():
        shorts, longs = rows(data, search, 0), LC.find_long(data)
        want = LC.merge(shorts, longs, stats)
        assert rows(data, search, 1) == want, name
        assert all(a + m <= b for (a, m, _), (b, _, _) in zip(want, want[1:])), name  # in order, none overlaps
        assert all(m >= 4 and p // LC.CHUNK == (p + m - 1) // LC.CHUNK and 0 < off <= p for p, m, off in want), name
        assert all(m >= LC.MIN_MATCH for _, m, _ in longs), name
        far_offsets += sum(off > 65535 for _, _, off in want)
        frame = Z.host_encode(data, 0, search, 1)[0]  # (options 0: every offset is written in full)
        blocks, got = AC.blocks(frame), []
        for c, b in enumerate(blocks):
            at = c * LC.CHUNK
            for ll, ml, ov in b.sequences:
                got.append((at + ll, ml, ov - 3))
                at += ll + ml
        in_frames = [s for s in want if blocks[s[0] // LC.CHUNK].kind == 2]  # (a Raw block states none)
        assert got == in_frames, name
    assert stats["head"] and stats["tail"] and stats["headtail"] and stats["gone"] and far_offsets > 20


def test_first_occurrence_and_chunk_ends():
    by_name = dict(LC.own_inputs())
    longs = LC.find_long(by_name["three_copies"])
    second = [m for m in longs if 160000 <= m[0] < 180000]
    third = [m for m in longs if m[0] >= 250000]
    assert second and third and all(off == 90000 for _, _, off in second) and all(off == 180000 for _, _, off in third)
    cut = LC.find_long(by_name["chunk_end_4000"])  # cut at the chunk's end and picked up again behind it
    assert cut == [(3 * LC.CHUNK - 2000, 2000, 3 * LC.CHUNK - 7000), (3 * LC.CHUNK, 2000, 3 * LC.CHUNK - 7000)]
    assert LC.find_long(by_name["chunk_end_40_100"]) == [(3 * LC.CHUNK, 100, 3 * LC.CHUNK - 40 - 77)]
    assert LC.find_long(by_name["partial_63_from_1003"]) == []
    for name in ("partial_64_from_1003", "partial_64_from_993", "partial_64_from_1024"):
        assert LC.find_long(by_name[name]) == [(120011, 64, 120011 - int(name.rsplit("_", 1)[1]))], name
    assert LC.find_long(by_name["partial_95_from_1003"]) == [(120011, 95, 120011 - 1003)]
    both = LC.merge(rows(by_name["both_sides"], 0, 0), LC.find_long(by_name["both_sides"]))
    assert [(96302, 20, 300), (96322, 70, 96322 - 3200), (96392, 10, 300)] == [s for s in both if s[0] >= 96302]
    for name in ("zeros_100000", "period_7"):  # the first chunk's source overlaps its target; all point at the start
        longs = LC.find_long(by_name[name])
        assert longs[0][2] < longs[0][1] and len(longs) == 4 and all(p - off < 7 * LC.GRID for p, _, off in longs), name


@pytest.mark.parametrize("options,search", LC.PAIRS)
def test_long_0_is_the_old_entry_point(options, search):
    for name, data, frame, flag in encoded(options, search, 0):
        assert (frame, flag) == Z.host_encode(data, options, search), name


@pytest.mark.parametrize("options,search", LC.PAIRS)
def test_every_frame_three_readers(options, search):
    for rec, (name, data, frame, flag) in zip(kat()["cases"], encoded(options, search, 1)):
        assert (rec["name"], rec["size"], rec["sha256"]) == (name, len(data), hashlib.sha256(data).hexdigest())
        got = rec[f"{options},{search}"]
        assert (got["frame_size"], got["frame_sha256"]) == (len(frame), hashlib.sha256(frame).hexdigest()), name
        assert got["decompressed"] == len(data), name  # libzstd decoded these very bytes to the input
        assert got["growth"] == len(frame) - len(Z.host_encode(data, options, search)[0]), name
        assert R.decode(frame) == data, name
        assert Z.host_decode(frame, len(data)) == (N.RPP_OK, data), name
        assert len(frame) <= Z.bound(len(data)) and flag == (len(frame) >= len(data)), name
        assert len(R.block_headers(frame)) == max(1, -(-len(data) // LC.CHUNK)), name  # one block per chunk


@pytest.mark.parametrize("options,search", LC.PAIRS)
def test_far_copies_shrink(options, search):
    """R + R: the first half is Raw (n / 2 and 3 bytes per chunk), the second one long match per chunk (81920 is a
    multiple of the grid, so the copy's first window is indexed): under n / 2 + n / 16.  Without the word the
    copy lies beyond the window and the frame is no smaller than the input."""
    short = {c[0]: c for c in encoded(options, search, 0)}
    for name, data, frame, flag in encoded(options, search, 1):
        if name not in LC.FAR:
            continue
        assert len(frame) < len(short[name][2]), name
        if name == "far_rr":
            n = len(data)
            assert len(frame) < n // 2 + n // 16 and not flag
            assert len(short[name][2]) >= n and short[name][3]


def test_format_reach():
    most = 0
    for name, data, frame, _ in encoded(0, 0, 1):
        for b in AC.blocks(frame):
            most = max([most] + [ov.bit_length() - 1 for _, _, ov in b.sequences])
    assert most >= 17
    data = LC.reach_20()  # 1.5 MiB: host only here, once on the GPU
    frame, flag = Z.host_encode(data, 3, 0, 1)
    rec = kat()["cases"][-1]
    assert (rec["name"], rec["sha256"]) == ("reach_20", hashlib.sha256(data).hexdigest())
    assert (rec["3,0"]["frame_size"], rec["3,0"]["frame_sha256"]) == (len(frame), hashlib.sha256(frame).hexdigest())
    assert rec["3,0"]["decompressed"] == len(data) and not flag
    assert R.decode(frame) == data and Z.host_decode(frame, len(data)) == (N.RPP_OK, data)
    last = [b for b in AC.blocks(frame) if b.sequences][-1]
    assert max(ov.bit_length() - 1 for _, _, ov in last.sequences) >= 20


def test_the_categorizer_sees_the_far_repeat():
    case = next(c for c in IC.cases() if c.name == "borderline_far_repeat")
    for long, category in ((0, "incompressible"), (1, "<default>")):
        cfg = CZ.IncompressibleConfig(min_input_size=case.min_input_size, block_size=case.block_size,
                                      generate_fragments=True, long=long)
        r = CZ.IncompressibleCategorizer(cfg, "cpu").categorize(case.data)
        assert r.fragments == [CZ.Fragment(category, len(case.data))], long
        scan = CZ.scan_pieces([case.data], cfg, "cpu")
        assert scan.sizes.tolist() == [len(Z.host_encode(case.data, 0, 0, long)[0])]
    with pytest.raises(ValueError):
        CZ.IncompressibleConfig(long=2)


def test_unknown_long_words_and_sizes():
    L = N.lib()
    src = np.frombuffer(b"abcdefgh", np.uint8)
    out = np.zeros(64, np.uint8)
    n = C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for long in (2, 3, 1 << 31):
        assert L.rpp_zstd_host_encode_long(p(src), 8, 0, 0, long, p(out), 64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            Z.ZstdBlockCompressor(device="cpu", long=long)
    assert L.rpp_zstd_host_encode_long(p(src), 8, 4, 0, 1, p(out), 64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
    assert L.rpp_zstd_host_encode_long(p(src), 8, 0, 3, 1, p(out), 64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
    # an over-size block is refused by its size alone (nothing is read); without the word 2^27 + 1 is no such size
    too_big = N.RPP_ZSTD_LONG_MAX_BLOCK + 1
    assert L.rpp_zstd_host_encode_long(p(src), too_big, 0, 0, 1, p(out), 64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
    assert L.rpp_zstd_host_encode_long(p(src), too_big, 0, 0, 0, p(out), 64, C.byref(n), None) == N.RPP_OUTPUT_TOO_SMALL
    for total, blocks in ((0, 1), (1 << 20, 3), (1 << 24, 1)):
        assert L.rpp_zstd_encode_workspace_bytes_long(total, blocks, 0) == L.rpp_zstd_encode_workspace_bytes(total, blocks)
        assert L.rpp_zstd_encode_workspace_bytes_long(total, blocks, 1) > L.rpp_zstd_encode_workspace_bytes(total, blocks)
        assert L.rpp_zstd_encode_workspace_bytes_long(total, blocks, 1) % 16 == 0


def test_python_layer_on_the_cpu():
    by_name = dict(LC.own_inputs())
    for spec, long in (("zstd", 0), ("zstd:long", 1), ("zstd:long=1", 1), ("zstd:long=0", 0),
                       ("zstd:level=3:long:depth=8:lazy=1", 1)):
        comp = Z.block_compressor_long(spec, "cpu")
        assert comp.long == long and comp.clone().long == long
        assert comp.describe() == ("zstd [level=%d, long]" if long else "zstd [level=%d]") % comp.level
        frame = comp.compress(by_name["far_gap_33"] if long else by_name["mixed_700"])
        want = Z.host_encode(by_name["far_gap_33"] if long else by_name["mixed_700"], 0, comp.search, long)[0]
        assert frame == want and Z.decompress(frame, "cpu") == (by_name["far_gap_33"] if long else by_name["mixed_700"])
    with pytest.raises(lz4.BadCompressionRatioError):
        Z.block_compressor("zstd", "cpu").compress(by_name["far_rr"])
    for spec in ("zstd:long", "zstd:long=1"):  # the factory without the option refuses it, as it always did
        with pytest.raises(RuntimeError, match="invalid option"):
            Z.block_compressor(spec, "cpu")
    for bad in ("zstd:long=2", "zstd:long=yes", "zstd:longer"):
        with pytest.raises(RuntimeError, match="invalid option"):
            Z.block_compressor_long(bad, "cpu")


def test_cpp_host_long_under_asan_ubsan(tmp_path):
    """tests/cpp/zstd_long_test.cpp: every size from 0 to 200 and the far-copy family through the host encoder with
    long = 1 and the host decoder, in a program of its own, built with AddressSanitizer and UBSan, with exact-size
    heap buffers."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_zstd_long.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "zstd_long_vectors.bin"
    with open(vec, "wb") as f:
        for i, (name, data, frame, _) in enumerate(encoded(3, 0, 1)):
            if name in LC.FAR or name in ("both_sides", "mixed_700", "three_copies", "period_7"):
                f.write(np.array([len(data), len(frame)], "<i8").tobytes() + data)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "zstd_long_test"), str(vec)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "zstd_long_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
