"""CPU tests of the constructed LZ4 blocks (tests/lz4_build.py; no GPU needed): the block writer itself, then
every block of every family through the independent reader (tests/lz4_ref.py), the host decoder with guard
bytes, and liblz4's LZ4_decompress_safe where liblz4.so.1 loads; the inputs aimed at the encoder through the
host encoder.  The expected bytes come from the sequence lists (``lz4_build.expand``).  The same families run
on the GPU in tests/test_gpu_lz4_constructed.py."""

import ctypes as C
import subprocess
from collections import Counter

import numpy as np
import pytest

import lz4_build as B
import lz4_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import lz4 as Z
from test_lz4_host import ROOT, guarded_host_decode, liblz4

# blocks per family: a change of a family shows here
FAMILY_SIZES = {"overlap": 6528, "apart": 120, "literals": 960, "window_edges": 78, "watermark": 1248,
                "output_size": 29, "batch_shape": 9}


def test_block_writer():
    assert B.length_ext(14) == b"" and B.length_ext(15) == b"\x00" and B.length_ext(269) == b"\xfe"
    assert B.length_ext(270) == b"\xff\x00" and B.length_ext(15 + 255 * 3 + 7) == b"\xff\xff\xff\x07"
    seqs, tail = [(b"abcd", 4, 8)], b"0123456789vwxyz"
    block = B.build(seqs, tail)
    assert block == bytes([0x44]) + b"abcd" + bytes([4, 0, 0xF0, 0]) + tail
    assert B.expand(seqs, tail) == b"abcdabcdabcd" + tail
    assert B.layout(seqs, tail) == [B.Fields(0, 1, 1, 5, 7, 7), B.Fields(7, 8, 9, -1, -1, 24)]
    with pytest.raises(AssertionError):
        B.build(seqs, b"vwxyz")  # the end rules are kept unless the caller says otherwise
    assert B.build(seqs, b"", end_rules=False)[-1] == 0
    with pytest.raises(ValueError):
        B.expand([(b"abcd", 5, 4)])
    for total in [0] + list(range(4, 700)):
        assert len(B.build(B.lead(total), b"", end_rules=False)) == total + 1  # (the last run's token)
    for field in ("token", "lit_ext", "literals", "offset", "match_ext"):
        for at in (40, 63, 64, 300):
            seq = (B.lits(20), 3, 30)
            placed = B.place(seq, field, at)
            assert getattr(B.layout(placed)[-2], field) == at and placed[-1] == seq
    assert len(set(B.lits(256, 3))) == 256 and B.FILL not in B.lits(600, 1, B.FILL)


@pytest.mark.parametrize("family", list(B.DECODE_FAMILIES))
def test_family_on_the_cpu_decoders(family):
    cases = B.DECODE_FAMILIES[family]()
    assert len(cases) == FAMILY_SIZES[family]
    assert len({c.what for c in cases}) == len(cases)
    L = liblz4()
    for c in cases:
        assert len(c.block) <= 72 * 1024 and c.out_n <= 72 * 1024, c.what
        try:
            ref = R.decode(c.block, c.out_n)
        except R.Lz4Error:
            ref = None
        assert (ref is not None) == c.ok, c.what
        if c.ok:
            assert ref == c.want and len(c.want) == c.out_n, c.what
        st, out, intact = guarded_host_decode(c.block, c.out_n)
        assert intact, c.what
        assert st == (N.RPP_OK if c.ok else N.RPP_CORRUPT_INPUT), c.what
        # a refused block leaves what the sequences before the refusal stored, and the fill behind it
        assert out == c.want + bytes([0xA5]) * (c.out_n - len(c.want)), c.what
        if L is not None and c.end_rules:  # (the comparison runs wherever liblz4.so.1 is installed)
            buf = C.create_string_buffer(max(c.out_n, 1))
            ret = L.LZ4_decompress_safe(c.block, buf, len(c.block), c.out_n)
            if c.ok:
                assert ret == c.out_n and buf.raw[:c.out_n] == c.want, c.what
            else:
                assert ret != c.out_n, c.what
    assert any(c.ok for c in cases)


def test_liblz4_is_compared_where_it_is_installed():
    """The families' comparison with LZ4_decompress_safe must not silently fall away on a machine that has
    the library: where `ldconfig` lists it, it has to load."""
    try:
        r = subprocess.run(["/sbin/ldconfig", "-p"], capture_output=True, text=True)
    except OSError:
        return
    if r.returncode == 0 and "liblz4.so.1" in r.stdout:
        assert liblz4() is not None


def test_families_reach_what_they_aim_at():
    """The counts that say the families visit the decode kernel's edges (the kernel's two rules as restated in
    lz4_build: the register window, the watermark)."""
    assert B.apart_alignments() == {(s, d) for s in range(4) for d in range(4)}
    # literals: stored from the window up to relative end 64, by the wide copy from 65 on
    ends = Counter()
    for c in B.literals():
        lit, rel, _ = B.window_trace(c.block)[-2]
        ends[rel + lit] += lit > 0
    assert all(ends[e] >= 4 for e in (62, 63, 64, 65, 66)) and ends[2] and ends[128], ends
    # window edges: the offset's low byte is read from lane 63, its high byte after a reload
    offs = [B.window_trace(c.block)[-2][2] for c in B.window_edges() if "edge offset" in c.what]
    assert offs == [63, 63, 63, 63]
    # watermark: every placement occurs, at the rule's equality edge without a wait and one byte on with one
    placed = Counter()
    for _, _, p in B.watermark_chains():
        for kind, s, e, W in p:
            placed[kind, (e > W) - (e < W), s < W] += 1
            assert {"ends_at_W": e == W, "ends_at_W_plus_1": e == W + 1, "starts_at_W_minus_1": s == W - 1 and e > W,
                    "in_previous_sequence": True, "copies_previous_match": True}[kind], (kind, s, e, W)
    assert placed["ends_at_W", 0, True] > 1000 and placed["ends_at_W_plus_1", 1, True] > 1000
    assert placed["starts_at_W_minus_1", 1, True] > 1000
    assert placed["in_previous_sequence", 1, False] > 1000 and placed["in_previous_sequence", -1, True] > 30
    assert placed["copies_previous_match", 1, False] > 1000
    assert sum(1 for what, _, _ in B.watermark_chains() if "copies_previous_match" in what) >= 64


@pytest.fixture(scope="module")
def encoder_inputs():
    return B.encoder_inputs(N.lib().rpp_lz4_chunk_bytes(), N.lib().rpp_lz4_step_positions())


def test_host_encoder_on_the_aimed_inputs(encoder_inputs):
    L = liblz4()
    chunk, step = N.lib().rpp_lz4_chunk_bytes(), N.lib().rpp_lz4_step_positions()
    assert len(encoder_inputs) == 70 + 2 * 81 + 3 * 12 + 2
    matches = {}
    for name, data in encoder_inputs:
        block, flag = Z.host_encode(data)
        n = len(data)
        assert R.decode(block, n) == data, name
        R.check_end_rules(block, n)
        assert flag == (4 + len(block) >= n), name
        assert len(block) <= Z.bound(n), name
        assert Z.host_decode(block, n) == (N.RPP_OK, data), name
        if L is not None:
            buf = C.create_string_buffer(max(n, 1))
            assert L.LZ4_decompress_safe(block, buf, len(block), n) == n, name
            assert buf.raw[:n] == data, name
        matches[name] = [(s.out_at + s.literals, s.match) for s in R.walk(block) if s.offset is not None]
    # the inputs reach what they aim at: the planted repeat is found with its length, however it is ended
    for m in B.PLANT_LENGTHS:
        if m >= 4:
            assert m in [ln for _, ln in matches[f"plant_{m}_differing_byte"]], m
            assert (chunk - m, m) in matches[f"plant_{m}_chunk_end"], m
        if m >= 7:  # (a match starts 12 bytes before the end at the latest)
            at, ln = matches[f"plant_{m}_last_literals"][-1]
            assert ln == m and at + ln == len(dict(encoder_inputs)[f"plant_{m}_last_literals"]) - 5, m
    for name in ("skip_steps_then_repeat", "skip_steps_zeros_then_repeat"):
        (at, ln), (at2, ln2) = matches[name][-2:]
        assert ln >= 3 * step and at2 == at + ln and ln2 == 40, (name, matches[name])  # the repeat right behind
    assert matches["period_1"] and matches["period_70"] and not matches["sentence_12"]


def test_cpp_host_functions_under_asan_ubsan_on_the_constructed_blocks(tmp_path, encoder_inputs):
    """tests/cpp/lz4_test.cpp (the host functions in a program of their own, built with AddressSanitizer and
    UBSan) over the constructed blocks: the small families whole, every 16th block of the two large ones."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_lz4.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "lz4_constructed.bin"
    with open(vec, "wb") as f:
        def rec(kind, n, expect, a, b=b""):
            f.write(np.array([kind, n, expect, len(a), len(b)], "<i8").tobytes() + a + b)
        for family, make in B.DECODE_FAMILIES.items():
            cases = make()
            for c in cases[::16] if len(cases) > 2000 else cases:
                if c.ok:
                    rec(0, c.out_n, 0, c.block, c.want)
                else:
                    rec(1, c.out_n, 0, c.block)
        for _, data in encoder_inputs:
            rec(2, len(data), 0, data)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "lz4_test"), str(vec)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "lz4_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
