"""CPU tests of the constructed Zstandard frames (tests/zstd_build.py; no GPU needed): the frame writer itself,
then every frame of every family through the independent reader (tests/zstd_ref.py), the host restatement with
guard bytes, libzstd 1.4.8's recorded verdict (tests/golden/zstd_built_kat.json) and libzstd itself where
libzstd.so.1 loads.  The expected bytes come from the builder's own executor of the sequence lists.  The same
families run on the GPU in tests/test_gpu_zstd_constructed.py."""

import json
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import zstd_build as B
import zstd_ref as R
from dwarfs_amd import _native as N
from test_zstd_host import ROOT, guarded_host_decode

sys.path.insert(0, str(ROOT / "tests" / "golden"))
import make_zstd_built_kat as K  # noqa: E402

# frames per family: a change of a family shows here
FAMILY_SIZES = {"overlap": 136, "apart": 84, "batches_of_64": 9, "watermark": 368, "repeat_offsets": 18, "chains": 52,
                "isolation": 13, "literals": 98, "sequences": 37, "window_and_size": 62}
# the frames that libzstd 1.4.8 accepts and the contract refuses, and the RFC 8878 section that refuses each
STRICTER_FRAMES = {
    "repeat_offsets initial history, code 3 without literals is offset 0": "3.1.1.5",
    "repeat_offsets repeat offset 1 minus 1 with repeat offset 1 = 1": "3.1.1.5",
    "sequences ll + ml one byte over the block maximum": "3.1.1.2.3",
    "window_and_size offset = window + 1": "3.1.1.1.2",
    "window_and_size Raw block of block maximum + 1": "3.1.1.2.3",
    "window_and_size RLE block of block maximum + 1": "3.1.1.2.3",
    "window_and_size a block's literals and match end at block maximum + 1": "3.1.1.2.3",
    "window_and_size a block's trailing literals end at block maximum + 1": "3.1.1.2.3",
}


@pytest.fixture(scope="module")
def kat():
    return json.loads((ROOT / "tests" / "golden" / "zstd_built_kat.json").read_text())


def test_frame_writer():
    assert B.backward([(5, 3), (0, 0), (1, 2)]) == bytes([0b1_101_01]) and B.backward([]) == b"\x01"
    assert B.backward([(0xAB, 8)]) == bytes([0xAB, 0x01])
    assert B.sequence_count(127) == b"\x7f" and B.sequence_count(128) == b"\x80\x80" and B.sequence_count(5, 2) == b"\x80\x05"
    assert B.sequence_count(0x7EFF) == b"\xfe\xff" and B.sequence_count(0x7F00) == b"\xff\x00\x00"
    assert B.literals_header(0, 0, 5) == b"\x28" and B.literals_header(1, 1, 5) == b"\x55\x00"
    assert B.literals_header(2, 0, 1023, 1023) == bytes([0xF2, 0xFF, 0xFF])
    assert B.window_descriptor(1024) == (0, 1024) and B.window_descriptor(1025) == (1, 1152)
    assert B.xxh64(b"") == 0xEF46DB3751D8E999  # (the published value for an empty input and seed 0)
    # descriptions go through the independent reader and come back as they were
    for norm, log in ((R.LL_DEFAULT), (R.OF_DEFAULT), (R.ML_DEFAULT), ([8, 6, 0, 0, 0, 0, 0, 0, 0, 0, 5, 4, 3, 2, 1, 1, -1, -1], 5),
                      ([0, 0, 0, 0, 31, 1], 5), ([1] * 20 + [0] * 7 + [492], 9), ([255, 0, -1], 8)):
        data, bits = B.fse_description(norm, log)
        assert len(data) == (bits + 7) // 8
        assert R.fse_read_description(data, 9, 52) == (list(norm), log, len(data)), norm
    with pytest.raises(B.BuildError):
        B.fse_description([3, 3], 5)
    # every tree description gives its weights back, and every symbol its code
    for weights, how in ((B.balanced_weights(range(5)), "direct"), (B.balanced_weights(range(5)), "fse"),
                         (B.unary_weights(B.DEEP), "direct"), (B.skewed_weights(list(range(40)), 4), "fse"),
                         (B.skewed_weights(list(range(41)), 4), "fse"), ([1, 1], "direct")):
        desc = B.tree_description(weights, how)
        got, used = R.huffman_weights(desc, None)
        assert (got, used) == (list(weights[:-1]), len(desc)), (weights, how)
        codes, text = B.huffman_codes(weights), bytes(s for s, w in enumerate(weights) if w) * 3
        assert R.huffman_stream(R.huffman_build(got), B.huffman_stream(codes, text), len(text)) == text
    # the smallest frame, byte by byte: a window of 1 KiB, a Raw block "ab", then a match of 3 at offset 2
    f = B.Frame().raw(b"ab").block([(b"c", 3, B.ov_of(2))], b"d")
    assert f.bytes() == bytes.fromhex("28b52ffd" "00" "00" "100000" "6162" "450000" "10" "6364" "01" "00" "014e08")
    assert R.decode(f.bytes(), size=7) == b"abcbcbd" == bytes(f.out)
    with pytest.raises(B.BuildError):
        B.Frame().raw(b"ab").block([(b"c", 3, B.ov_of(4))]).case("offset before the start, called valid")
    assert len(set(B.lits(256, 3))) == 256 and B.FILL not in B.lits(600, 1, B.FILL)


@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_family_on_the_cpu_decoders(family, kat):
    cases = B.FAMILIES[family]()
    assert len(cases) == FAMILY_SIZES[family]
    assert len({c.what for c in cases}) == len(cases)
    L = K.libzstd()
    recs = kat["families"][family]
    assert [r[0] for r in recs] == [c.what for c in cases]
    for c, rec in zip(cases, recs):
        assert c.what.startswith(family)
        try:
            ref = R.decode(c.frame, size=c.out_n)
        except R.ZstdError:
            ref = None
        assert (ref is not None) == c.ok, c.what
        assert len(c.want) == c.out_n if c.ok else len(c.want) <= c.out_n, c.what
        if c.ok:
            assert ref == c.want, c.what
        st, out, intact = guarded_host_decode(c.frame, c.out_n)
        assert intact, c.what
        assert st == (N.RPP_OK if c.ok else N.RPP_CORRUPT_INPUT), c.what
        assert out[:len(c.want)] == c.want, c.what  # (a refused frame: what the blocks before the failing one produce)
        try:
            assert R.count_blocks(c.frame) == c.blocks, c.what
        except R.ZstdError:  # (the headers cannot be walked: the caller's promise is one block)
            assert c.blocks == 1 and not c.ok, c.what
        # libzstd 1.4.8 as recorded
        assert rec[1] == K.digest(c.frame), c.what
        accepted = rec[2] == c.out_n
        if len(rec) > 4:  # the RFC states a rule that libzstd does not enforce
            assert accepted and not c.ok and rec[4] == STRICTER_FRAMES[c.what], c.what
        else:
            assert accepted == c.ok, c.what
        if accepted and c.ok:
            assert rec[3] == K.digest(c.want), c.what
        if L is not None:  # (and libzstd itself wherever libzstd.so.1 is installed)
            ret, zout = K.verdict(L, c.frame, c.out_n)
            assert ret == rec[2] and (K.digest(zout) if ret == c.out_n else "") == rec[3], c.what
    assert any(c.ok for c in cases)


def test_libzstd_is_compared_where_it_is_installed():
    try:
        r = subprocess.run(["/sbin/ldconfig", "-p"], capture_output=True, text=True)
    except OSError:
        return
    if r.returncode == 0 and "libzstd.so.1" in r.stdout:
        assert K.libzstd() is not None


def test_recorded_disagreements_are_the_rfcs_rules(kat):
    assert kat["version"] == "1.4.8"
    recs = [r for f in kat["families"].values() for r in f]
    stricter = [r for r in recs if len(r) > 4]
    assert 20 * len(stricter) <= len(recs) and len(recs) == sum(FAMILY_SIZES.values())
    assert {r[0]: r[4] for r in stricter} == STRICTER_FRAMES
    # the 0-literal last stream of four: libzstd accepts it, as the contract does
    zero = [r for r in kat["families"]["literals"] if "the last holds 0" in r[0]]
    assert len(zero) == 2 and all(r[3] and len(r) == 4 for r in zero)


def test_built_frames_reach_every_feature():
    """The accepted frames reach every feature of the format that the reader counts, the four that libzstd
    wrote for none of its frames included (the kat's "not_reached" stays: it is a statement about libzstd)."""
    stats = Counter()
    for c in B.all_cases():
        if c.ok:
            R.decode(c.frame, stats, size=c.out_n)
    assert [k for k in R.FEATURES if stats[k] == 0] == []
    assert all(stats[k] >= 2 for k in ("literals:rle:0", "of:rle", "seqcount:3byte", "fcs_bytes:8"))


def test_families_reach_what_they_aim_at():
    """The counts that say the families visit the kernels' edges."""
    # watermark: every placement occurs, at the rule's equality edge without a wait and one byte on with one
    placed = Counter()
    for _, _, p in B.watermark_chains():
        for kind, s, e, W in p:
            placed[kind, (e > W) - (e < W), s < W] += 1
            assert {"ends_at_W": e == W, "ends_at_W_plus_1": e == W + 1, "starts_at_W_minus_1": s == W - 1 and e > W,
                    "in_own_literals": s >= W}.get(kind, True), (kind, s, e, W)
    assert placed["ends_at_W", 0, True] > 500 and placed["ends_at_W_plus_1", 1, True] > 500
    assert placed["starts_at_W_minus_1", 1, True] > 500 and placed["in_own_literals", 1, False] > 200
    assert placed["in_previous_sequence", 1, False] > 500 and placed["copies_previous_match", 1, False] > 300
    # literals: both refill paths (a stream below 8 bytes is read byte-wise), and four streams of unequal bytes
    f = B.Frame()
    f.compressed(b"A" * 300 + b"L" * 300 + b"A" * 300 + b"K" * 300, lit=dict(kind="compressed", weights=B.unary_weights(B.DEEP), sf=2))
    assert f.stream_bytes == [38, 413, 38, 413]
    f.compressed(b"L" * 10 + b"K" * 10 + b"L" * 10 + b"A" * 7, lit=dict(kind="treeless", sf=1))
    assert f.stream_bytes == [14, 14, 14, 1]
    # sequences: the widest one asks for 16 + 15 + 16 extra bits (offset, match length, literal length) behind
    # the three first states, and the state updates behind it (LL, ML, OF) read 9 + 9 + 8 bits: 73 bits in a row
    wide = B.wide_frame()
    assert [n for _, n in wide.reads[:9]] == [9, 8, 9, 16, 15, 16, 9, 9, 8]
    assert wide.case("widest") == next(c for c in B.sequences() if "widest" in c.what)._replace(what="widest")
    assert len(wide.out) == 100 + B.BLOCK_MAX
    # chains: every supplier's description differs, so a table from the wrong block cannot read the same codes
    assert len({tuple(B._fse3(v)[k][1]) for v in range(20) for k in range(3)}) >= 40


def test_cpp_host_functions_under_asan_ubsan_on_the_built_frames(tmp_path):
    """tests/cpp/zstd_test.cpp (the host functions in a program of their own, built with AddressSanitizer and
    UBSan) over all the built frames."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_zstd.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "zstd_built.bin"
    with open(vec, "wb") as f:
        for make in B.FAMILIES.values():
            for c in make():
                f.write(np.array([c.out_n, int(c.ok), len(c.frame), len(c.want) if c.ok else 0], "<i8").tobytes() +
                    c.frame + (c.want if c.ok else b""))
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "zstd_test"), str(vec)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "zstd_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
