"""CPU tests of the segmenter's match search (no GPU needed): the C ABI's host-side entry points, and the host
restatement (rpp_segment_host_hashes / _index / _scan / _extend: a rolling update and a sequential index build)
against tests/golden/segment_kat.json -- the Python model's answers from prefix sums and per-window content."""

import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from dwarfs_amd import _native as N
from dwarfs_amd import segmenter as S
from dwarfs_amd.codec import UnsupportedConfiguration

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_segment_kat as K  # noqa: E402

NEW_SYMBOLS = ("rpp_segment_check_config", "rpp_segment_tile_frames", "rpp_segment_positions", "rpp_segment_index_slots",
               "rpp_segment_hash_workspace_bytes", "rpp_segment_hash_batch", "rpp_segment_scan_workspace_bytes",
               "rpp_segment_scan_batch", "rpp_segment_index_workspace_bytes", "rpp_segment_index_batch",
               "rpp_segment_extend_batch", "rpp_segment_host_hashes", "rpp_segment_host_index", "rpp_segment_host_scan",
               "rpp_segment_host_extend")


def Cfg(c) -> S.SegmenterConfig:
    return S.SegmenterConfig(c["window_bits"], c["increment_shift"], c["granularity"], c["filter_bits"])


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "segment_kat.json").read_text())


def test_kat_file_is_current(kat):
    """The committed file is what the model writes (the model's own assertions run here too)."""
    assert json.loads(json.dumps(K.build())) == kat
    assert (GOLDEN / "segment_kat.json").stat().st_size < 400 * 1024


def test_symbols_and_sizes():
    L = N.lib()
    for name in NEW_SYMBOLS:
        assert name in N.EXPORTED_SYMBOLS and hasattr(L, name)
    assert C.sizeof(N.RppSegmentConfig) == 24 and C.sizeof(N.RppSegmentScanResult) == 16
    assert S.HIT_DTYPE.itemsize == 8 and S.CANDIDATE_DTYPE.itemsize == 40 and S.MATCH_DTYPE.itemsize == 12
    T = S.tile_frames()
    assert T >= 256 and T & (T - 1) == 0
    cfg = S.SegmenterConfig(4, 1, 3, 1024)
    assert (cfg.window_frames, cfg.window_bytes, cfg.step_frames, cfg.filter_words) == (16, 48, 8, 16)
    assert [cfg.positions(f) for f in (0, 15, 16, 17, 2**32 - 1, 2**32)] == [0, 0, 1, 2, 2**32 - 16, 0]
    assert [cfg.slots(f) for f in (15, 16, 23, 24, 100)] == [0, 1, 1, 2, 11]
    assert S.SegmenterConfig(2, 5, 1, 64).step_frames == 1 and S.SegmenterConfig(2, 5, 1, 64).slots(10) == 7
    assert L.rpp_segment_scan_workspace_bytes(3, 10**6) > L.rpp_segment_hash_workspace_bytes(3, 10**6) > 0


@pytest.mark.parametrize("bad", [dict(window_bits=0), dict(window_bits=21), dict(granularity=0), dict(granularity=65),
                                 dict(filter_bits=0), dict(filter_bits=32), dict(filter_bits=96),
                                 dict(filter_bits=(1 << 16) + 64), dict(filter_bits=1 << 33), dict(window_bits=2**32)])
def test_unsupported_config(bad):
    """Every entry point refuses the config before it touches any pointer."""
    cfg = S.SegmenterConfig(**{**dict(window_bits=4, increment_shift=1, granularity=1, filter_bits=1024), **bad})
    with pytest.raises(UnsupportedConfiguration):
        cfg.native()
    with pytest.raises(UnsupportedConfiguration):
        S.host_hashes(bytes(100), cfg)
    if max(bad.values()) >= 2**32 and "filter_bits" not in bad:
        return
    L = N.lib()
    c = N.RppSegmentConfig(cfg.window_bits, cfg.increment_shift, cfg.granularity, 0, cfg.filter_bits)
    null = C.c_void_p(0)
    U = N.RPP_UNSUPPORTED_CONFIG
    assert L.rpp_segment_check_config(C.byref(c)) == U
    assert L.rpp_segment_check_config(None) == U
    assert L.rpp_segment_positions(C.byref(c), 1000) == 0 and L.rpp_segment_index_slots(C.byref(c), 1000) == 0
    assert L.rpp_segment_hash_batch(C.byref(c), null, null, null, 1, 100, null, 0, null, null, null, 0, null) == U
    assert L.rpp_segment_scan_batch(C.byref(c), null, null, null, 1, 100, null, null, 0, null, null, null, 0, null) == U
    assert L.rpp_segment_index_batch(C.byref(c), null, null, null, 1, 100, null, null, null, 0, null, null, null, null,
                                     null, 0, null) == U
    assert L.rpp_segment_extend_batch(C.byref(c), null, null, null, 1, null, null) == U
    assert L.rpp_segment_host_hashes(C.byref(c), null, 100, null) == U
    assert L.rpp_segment_host_index(C.byref(c), null, 100, null, null, null, null, null) == U
    assert L.rpp_segment_host_scan(C.byref(c), null, 100, null, null, 0, null) == U
    assert L.rpp_segment_host_extend(C.byref(c), null, null, null, 1, null) == U


def test_argument_checks_without_gpu():
    L = N.lib()
    c = S.SegmenterConfig(4, 1, 1, 1024).native()
    null = C.c_void_p(0)
    I = N.RPP_INVALID_ARGUMENT
    assert L.rpp_segment_hash_batch(C.byref(c), null, null, null, 0, 0, null, 0, null, null, null, 0, null) == N.RPP_OK
    assert L.rpp_segment_index_batch(C.byref(c), null, null, null, 0, 0, null, null, null, 0, null, null, null, null, null,
                                     0, null) == N.RPP_OK
    assert L.rpp_segment_extend_batch(C.byref(c), null, null, null, 0, null, null) == N.RPP_OK
    assert L.rpp_segment_hash_batch(C.byref(c), null, null, null, 1, 100, null, 0, null, null, null, 0, null) == I
    assert L.rpp_segment_scan_batch(C.byref(c), null, null, null, 1, 100, null, null, 0, null, null, null, 0, null) == I
    assert L.rpp_segment_extend_batch(C.byref(c), null, null, null, 1, null, null) == I
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    need = L.rpp_segment_scan_workspace_bytes(1, 100)
    assert L.rpp_segment_scan_batch(C.byref(c), p, p, p, 1, 100, p, p, 4, null, p, p, need - 1, null) == I
    # an extent of 2^32 frames is an error on the host too, and nothing is read
    assert L.rpp_segment_host_hashes(C.byref(c), p, 2**32, p) == I
    count = C.c_uint64(7)
    assert L.rpp_segment_host_scan(C.byref(c), p, 2**32, p, p, 0, C.cast(C.byref(count), C.c_void_p)) == I
    assert L.rpp_segment_host_index(C.byref(c), p, 2**32, p, p, p, p, p) == I
    # shorter than the window: OK and nothing written
    assert L.rpp_segment_host_hashes(C.byref(c), null, 15, null) == N.RPP_OK
    assert S.host_hashes(bytes(15), S.SegmenterConfig(4, 1, 1, 1024)).size == 0


def test_host_hashes_equal_kat(kat):
    for e in kat["hashes"]:
        h = S.host_hashes(K.message_bytes(e["message"]), Cfg(e["config"]))
        assert h.size == e["count"] and K.digest(h) == e["sha256"], (e["config"], e["message"])
        assert h[:4].tolist() == e["first"] and h[-1:].tolist() == e["last"]


@pytest.mark.parametrize("bits,g", [(4, 1), (12, 1), (12, 6)])
def test_closed_form_all_byte_values(bits, g):
    """A window of L equal bytes v: a = v L, b = v L (L + 1) / 2, both mod 2^16 (at (12, 6) both wrap many times);
    the rolled values after it agree with the first."""
    cfg = S.SegmenterConfig(bits, 1, g, 1024)
    L = cfg.window_bytes
    for v in range(256):
        want = ((v * L) & 0xFFFF) | (((v * L * (L + 1) // 2) & 0xFFFF) << 16)
        assert S.host_hashes(bytes([v]) * (L + 2 * g), cfg).tolist() == [want] * 3, v


def test_host_index_equals_kat(kat):
    for e in kat["index"]:
        cfg = Cfg(e["config"])
        r = S.host_index(K.message_bytes(e["message"]), cfg)
        assert (r.hash.tolist(), r.offset.tolist(), r.entered.tolist()) == (e["hash"], e["offset"], e["entered"]), \
            (e["config"], e["message"])
        assert r.block_filter.tobytes().hex() == e["block_filter"] == r.global_filter.tobytes().hex()
        assert len(e["hash"]) == cfg.slots(e["message"]["length"] // cfg.granularity)


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_first_repeating_window_rule(shift):
    """zeros, random bytes, zeros, then 0x5A bytes: the first all-zero window and the first all-0x5A window of the
    block are entered, the later ones are not; every other window is; only entered hashes reach the filters."""
    cfg = S.SegmenterConfig(4, shift, 1, 1 << 14)
    W, step = cfg.window_frames, cfg.step_frames
    rng = np.random.default_rng(31)
    q = 4 * W + 3
    block = bytes(q) + rng.integers(1, 256, q, dtype=np.uint8).tobytes() + bytes(q) + b"\x5a" * q
    r = S.host_index(block, cfg)
    assert r.offset.tolist() == list(range(0, len(block) - W + 1, step))
    seen, want = set(), []
    for o in r.offset.tolist():
        w = block[o:o + W]
        rep = len(set(w)) == 1
        want.append(0 if rep and w[0] in seen else 1)
        if rep:
            seen.add(w[0])
    assert r.entered.tolist() == want and seen == {0, 0x5A}
    zero = [i for i, o in enumerate(r.offset.tolist()) if block[o:o + W] == bytes(W)]
    assert len(zero) >= 6 and r.entered[zero].tolist() == [1] + [0] * (len(zero) - 1)
    assert any(o > 2 * q for o in r.offset[zero].tolist())  # (zero windows of the second run are among them)
    model = [0] * cfg.filter_words
    for h, e in zip(r.hash.tolist(), r.entered.tolist()):
        if e:
            K.filter_set(model, h)
    assert r.block_filter.tolist() == model
    # a second block into the same global filter: its first all-zero window is entered again (the rule is per block)
    r2 = S.host_index(bytes(2 * W), cfg, r.global_filter)
    assert r2.entered.tolist()[0] == 1 and sum(r2.entered.tolist()) == 1
    assert (r.global_filter == (r.block_filter | r2.block_filter)).all()


def test_host_scan_equals_kat(kat):
    for e in kat["scan"]:
        cfg = Cfg(e["config"])
        block, extent, plants = K.planted(e["config"], e["seed"])
        filt = S.host_index(block, cfg).block_filter
        assert filt.tobytes().hex() == e["block_filter"]
        pos, hashes, count = S.host_scan(extent, filt, cfg)
        assert count == len(e["hits"]) and [[int(p), int(h)] for p, h in zip(pos, hashes)] == e["hits"]
        # a capacity one below the count: the full count, a correct prefix
        p2, h2, c2 = S.host_scan(extent, filt, cfg, capacity=count - 1)
        assert c2 == count and np.array_equal(p2, pos[:-1]) and np.array_equal(h2, hashes[:-1])
        assert S.host_scan(extent, np.zeros(cfg.filter_words, np.uint64), cfg)[2] == 0
        full = S.host_scan(extent, np.full(cfg.filter_words, 2**64 - 1, np.uint64), cfg)
        assert np.array_equal(full[1], S.host_hashes(extent, cfg)) and full[2] == cfg.positions(len(extent) // cfg.granularity)


def test_host_extend_equals_kat(kat):
    for e in kat["extend"]:
        cfg = Cfg(e["config"])
        ext, block, cands = K.extend_case(e["config"], e["seed"])
        assert [list(c) for c in cands] == e["candidates"]
        cd = np.concatenate([S.candidates([c[0]], c[1], 0, 0, c[2], c[3], c[4]) for c in cands])
        got = S.host_extend(ext, block, cd, cfg)
        assert [[int(m["off"]), int(m["pos"]), int(m["size"])] for m in got] == e["matches"]
    # candidates that do not fit are no match and nothing of them is read
    cfg = S.SegmenterConfig(4, 1, 1, 1024)
    bad = np.concatenate([S.candidates([0], 1, 0, 0, 0, 16, 16), S.candidates([1], 0, 0, 0, 0, 16, 16),
                          S.candidates([0], 0, 0, 0, 1, 16, 16)])
    got = S.host_extend(bytes(16), bytes(16), bad, cfg)
    assert got["size"].tolist() == [0, 0, 0] and got["pos"].tolist() == [0, 1, 0] and got["off"].tolist() == [1, 0, 0]
