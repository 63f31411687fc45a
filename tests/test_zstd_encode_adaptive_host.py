"""CPU tests of the Zstandard encoder's options word (no GPU needed): the host restatement over the inputs of
tests/zstd_enc_adaptive_cases.py with options 1 (per-block table modes), 2 (repeat offsets) and 3 (both).  Every
frame is read by libzstd 1.4.8, whose verdict tests/golden/zstd_enc_adaptive_kat.json records under the frame's
SHA-256, by the independent reader tests/zstd_ref.py and by rpp_zstd_host_decode.  Then the rules themselves,
restated here and applied to what the reader finds in the frames, the format reach, the sizes, the Python layer,
and the host functions alone under AddressSanitizer and UBSan."""

import ctypes as C
import functools
import hashlib
import json
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import zstd_enc_adaptive_cases as AC
import zstd_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import lz4
from dwarfs_amd import zstd as Z

ROOT = Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((ROOT / "tests" / "golden" / "zstd_enc_adaptive_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def encoded(options):
    """[(name, input, frame, flag)], computed once per options word"""
    return [(name, data, *Z.host_encode(data, options)) for name, data in AC.inputs()]


@functools.lru_cache(maxsize=None)
def parsed(options):
    """{name: the blocks of its frame}"""
    return {name: AC.blocks(frame) for name, _, frame, _ in encoded(options)}


def test_options_0_is_the_old_entry_point():
    L = N.lib()
    for name, data, frame, flag in encoded(0):
        assert (frame, flag) == Z.host_encode(data), name
        src = np.frombuffer(data + b"\0", np.uint8)
        out = np.zeros(Z.bound(len(data)), np.uint8)
        n, f = C.c_uint64(), C.c_uint32()
        assert L.rpp_zstd_host_encode(src.ctypes.data_as(C.c_void_p), len(data), out.ctypes.data_as(C.c_void_p),
                                      len(out), C.byref(n), C.byref(f)) == N.RPP_OK
        assert out[:n.value].tobytes() == frame and bool(f.value) == flag, name


@pytest.mark.parametrize("options", AC.OPTIONS)
def test_every_input_three_readers(options):
    records = kat()["cases"]
    assert kat()["version"] == "1.4.8" and [r["name"] for r in records] == [c[0] for c in encoded(options)]
    for rec, (name, data, frame, flag) in zip(records, encoded(options)):
        assert (rec["size"], rec["sha256"]) == (len(data), hashlib.sha256(data).hexdigest()), name
        got = rec[str(options)]
        assert (got["frame_size"], got["frame_sha256"]) == (len(frame), hashlib.sha256(frame).hexdigest()), name
        assert got["decompressed"] == len(data), name  # libzstd decoded these very bytes to the input
        assert rec["size0"] == len(encoded(0)[records.index(rec)][2]), name
        assert R.decode(frame) == data, name
        assert Z.host_decode(frame, len(data)) == (N.RPP_OK, data), name
        assert len(frame) <= Z.bound(len(data)) and flag == (len(frame) >= len(data)), name
        assert len(R.block_headers(frame)) == max(1, -(-len(data) // AC.CHUNK)), name  # one block per chunk


def offset_value(off, off1, off2, ll, i):
    """The repeat-offset rule of zstd_enc_common.h, restated."""
    if i >= 1 and ll > 0 and off == off1:
        return 1
    if i >= 2 and off == off2 and off != off1:
        return 2 if ll > 0 else 1
    return off + 3


@pytest.mark.parametrize("options", (2, 3))
def test_the_repeat_rule_sequence_by_sequence(options):
    """The options-0 frame states every offset in full; from those the rule gives the value of every sequence."""
    first_in_full = 0
    for name, _, _, _ in encoded(0):
        plain, got = parsed(0)[name], parsed(options)[name]
        if [b.kind for b in plain] != [b.kind for b in got]:
            continue  # (a chunk that is Compressed only with the options has no options-0 sequences to go by)
        for bp, bg in zip(plain, got):
            offs = [ov - 3 for _, _, ov in bp.sequences]
            assert all(o >= 1 for o in offs), name
            want = [(ll, ml, offset_value(off, offs[i - 1] if i else 0, offs[i - 2] if i > 1 else 0, ll, i))
                    for i, ((ll, ml, _), off) in enumerate(zip(bp.sequences, offs))]
            assert bg.sequences == want, name
            first_in_full += bool(want)
    assert first_in_full > 100
    # two chunks, the second one's first offset equal to the first one's last: written in full all the same
    first, second = parsed(options)["same_offset_across_chunks"]
    assert first.sequences[-1][2] == second.sequences[0][2] == 100 + 3


def own_table_log(count, seen):
    return 6 if count > 64 or seen > 16 else 5


def normalise(hist, log):
    """fse_normalise of zstd_enc_common.h, restated: ({code: probability}, whether it had to give back)."""
    size, total = 1 << log, sum(hist.values())
    freq = {s: max(1, c * size // total) for s, c in sorted(hist.items())}
    most = max(sorted(hist), key=lambda s: hist[s])  # (max keeps the first of equals: the smallest code)
    gave_back = sum(freq.values()) > size
    if sum(freq.values()) < size:
        freq[most] += size - sum(freq.values())
    while sum(freq.values()) > size:
        freq[max(sorted(freq), key=lambda s: freq[s])] -= 1
    return freq, gave_back


def codes_of(seqs):
    ll = [max(c for c in range(36) if R.LL_BASE[c] <= q[0]) for q in seqs]
    of = [q[2].bit_length() - 1 for q in seqs]
    ml = [max(c for c in range(53) if R.ML_BASE[c] <= q[1]) for q in seqs]
    return ll, of, ml


@pytest.mark.parametrize("options", (1, 3))
def test_the_table_rules_block_by_block(options):
    """RLE exactly where one code is seen; an FSE_Compressed table has the rule's accuracy log and the rule's
    normalised distribution of the block's own codes."""
    gave_back, logs = Counter(), Counter()
    for name, _, _, _ in encoded(options):
        for b in parsed(options)[name]:
            if not b.sequences:
                continue
            for k, codes in enumerate(codes_of(b.sequences)):
                hist, mode = Counter(codes), b.modes >> (6 - 2 * k) & 3
                assert mode in (0, 1, 2) and (mode == 1) == (len(hist) == 1), (name, k)
                if mode == 1:
                    assert b.tables[k] == (0, {codes[0]: 1}), (name, k)
                if mode == 2:
                    log = own_table_log(len(codes), len(hist))
                    freq, back = normalise(hist, log)
                    assert b.tables[k] == (log, freq), (name, k)
                    gave_back[name] += back
                    logs[log] += 1
    assert logs[5] > 0 and logs[6] > 0
    assert gave_back["dominant_50_14"] > 0
    # the counts on either side of the accuracy log's step, and 1, 2 and 3 sequences
    for t, log in ((AC.LOG_STEP, 5), (AC.LOG_STEP + 1, 6)):
        (b,) = parsed(options)[f"adaptive_sequences_{t}"]
        assert len(b.sequences) == t and b.modes >> 6 == 2 and b.tables[0][0] == log, t
    for t in (1, 2, 3):
        (b,) = parsed(options)[f"adaptive_sequences_{t}"]
        assert len(b.sequences) == t, t
    assert parsed(options)["adaptive_sequences_1"][0].modes == 0b01010100  # three RLE tables


def reach(options):
    stats = Counter()
    for _, data, frame, _ in encoded(options):
        assert R.decode(frame, stats) == data
    return stats


def test_format_reach():
    both, tables, repeat = reach(3), reach(1), reach(2)
    reached = sorted(k for k in R.FEATURES if both[k] and (k.startswith("rep:") or k[:3] in ("ll:", "of:", "ml:")))
    assert reached == sorted(["ll:predefined", "ll:rle", "ll:fse", "of:predefined", "of:rle", "of:fse",
                              "ml:predefined", "ml:rle", "ml:fse", "rep:1:ll", "rep:2:ll", "rep:1:ll0"])
    assert not any(v for k, v in tables.items() if k.startswith("rep:"))  # options 1: no offset value below 4
    assert all(ov >= 4 for bs in parsed(1).values() for b in bs for _, _, ov in b.sequences)
    assert all(b.modes in (None, 0) for bs in parsed(2).values() for b in bs)  # options 2: modes byte 0 only
    assert repeat["rep:1:ll"] and repeat["rep:2:ll"] and repeat["rep:1:ll0"]
    for stats in (both, tables, repeat):  # nothing the definition rules out
        for key in R.FEATURES:
            if key.startswith(("block:rle", "literals:treeless", "rep:3", "rep:2:ll0", "frame:windowed",
                               "frame:checksum")) or key.endswith(":repeat"):
                assert stats[key] == 0, key
    # Raw under every option; the literal runs and match lengths of wide_alphabets reach the high codes
    assert all(b.kind == 0 for o in (0, 1, 2, 3) for b in parsed(o)["random_two_chunks"])
    ll, _, ml = codes_of([q for b in parsed(3)["wide_alphabets"] for q in b.sequences])
    assert max(ll) >= 30 and max(ml) >= 47 and len(set(ll)) >= 25 and len(set(ml)) >= 40


def test_totals_against_options_0():
    old = json.loads((ROOT / "tests" / "golden" / "zstd_enc_kat.json").read_text())["cases"]
    base = len(old)
    assert [r["name"] for r in old] == [c[0] for c in encoded(3)[:base]]
    total0 = sum(r["frame_size"] for r in old)
    total3 = sum(len(c[2]) for c in encoded(3)[:base])
    assert total3 < total0
    assert kat()["totals"]["0"]["base"] == total0 and kat()["totals"]["3"]["base"] == total3


def test_unknown_option_bits():
    L = N.lib()
    out = np.zeros(64, np.uint8)
    n = C.c_uint64()
    src = np.frombuffer(b"abcdefgh", np.uint8)
    for options in (4, 8, 7, 1 << 31):
        assert L.rpp_zstd_host_encode_opt(src.ctypes.data_as(C.c_void_p), 8, options, out.ctypes.data_as(C.c_void_p),
                                          64, C.byref(n), None) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_zstd_encode_batch_opt(None, None, None, 0, options, None, None, None, None, None, 0, None, 0,
                                           None) == N.RPP_INVALID_ARGUMENT
        with pytest.raises(Exception):
            Z.host_encode(b"abcdefgh", options)
        with pytest.raises(ValueError):
            Z.ZstdBlockCompressor(device="cpu", options=options)
    assert L.rpp_zstd_encode_batch_opt(None, None, None, 0, 3, None, None, None, None, None, 0, None, 0, None) == N.RPP_OK
    assert (Z.ENC_TABLES, Z.ENC_REPEAT, Z.ENC_ADAPTIVE) == (1, 2, 3)
    assert (N.RPP_ZSTD_ENC_TABLES, N.RPP_ZSTD_ENC_REPEAT) == (1, 2)


def test_python_layer_on_the_cpu():
    by_name = dict(AC.inputs())
    for options in (0,) + AC.OPTIONS:
        comp = Z.ZstdBlockCompressor(device="cpu", options=options)
        assert comp.describe() == "zstd [level=22]" and comp.clone().options == options
        for name in ("records_600", "interleaved_mixed", "same_offset_across_chunks"):
            frame = comp.clone().compress(by_name[name])
            assert frame == Z.host_encode(by_name[name], options)[0], name
            assert Z.decompress(frame, "cpu") == by_name[name], name
        with pytest.raises(lz4.BadCompressionRatioError):
            comp.compress(by_name["random_two_chunks"])
        many = comp.compress_many([by_name["records_600"], by_name["random_two_chunks"], b""], keep_bad=True)
        assert many[1] is None and many[2] is None and many[0] == Z.host_encode(by_name["records_600"], options)[0]
    assert Z.ZstdBlockCompressor(device="cpu").options == 0 and Z.block_compressor("zstd", "cpu").options == 0


def test_cpp_host_encoder_with_options_under_asan_ubsan(tmp_path):
    """tests/cpp/zstd_encode_adaptive_test.cpp: host encode with each options word, then host decode, of every
    input in a program of its own, built with AddressSanitizer and UBSan, with exact-size heap buffers."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_zstd_encode_adaptive.sh")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "zstd_encode_adaptive_vectors.bin"
    with open(vec, "wb") as f:
        for i, (_, data, _, _) in enumerate(encoded(0)):
            sizes = [len(encoded(o)[i][2]) for o in (0, 1, 2, 3)]
            f.write(np.array([len(data)] + sizes, "<i8").tobytes() + data)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "zstd_encode_adaptive_test"), str(vec)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "zstd_encode_adaptive_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
