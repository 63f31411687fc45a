"""GPU tests of the segmenter's match search (rpp_segment_hash_batch ... rpp_segment_extend_batch and their Python /
C++ layers).  Every comparison is for equality: with the host restatement (a rolling update and a sequential
index build, not the kernels' formulation) and with tests/golden/segment_kat.json (the Python model)."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from dwarfs_amd import _native as N
from dwarfs_amd import segmenter as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_segment_kat as K  # noqa: E402

DEV = "cuda"


def C(c) -> S.SegmenterConfig:
    return S.SegmenterConfig(c["window_bits"], c["increment_shift"], c["granularity"], c["filter_bits"])


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "segment_kat.json").read_text())


def _dev(b: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b) + b"\x3c" * 16, np.uint8).copy()).to(DEV)


def _fill(kind: str, n: int, i: int, rng) -> bytes:
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "zero":
        return bytes(n)
    pair = b"\xa5\x3c" if i % 2 == 0 else b"\x11\xee"
    return (pair * (n // 2 + 1))[:n]


def _u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


# ---- hashes ----

@pytest.mark.parametrize("data_kind", ["random", "zero", "period2"])
@pytest.mark.parametrize("g", [1, 2, 3, 4, 5, 6])
def test_hashes_at_every_misalignment(g, data_kind):
    """Extents of W - 1 (no output), W, W + 1, T - 1, T, T + 1 and 2T + 3 frames, each starting at every byte
    offset modulo 16, back to back in one batch behind filler bytes."""
    cfg = S.SegmenterConfig(4, 1, g, 1024)
    W, T = cfg.window_frames, S.tile_frames()
    rng = np.random.default_rng(21)
    frames = [W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 3]
    exts, starts, at = [], [], 0
    for a in range(16):
        at = (at + 15) // 16 * 16 + a
        for f in frames:
            exts.append(_fill(data_kind, f * g, len(exts), rng))
            starts.append(at)
            at += f * g
    blob = bytearray(b"\xc3" * (at + 16))
    for o, e in zip(starts, exts):
        blob[o:o + len(e)] = e
    assert {(o % 16, len(e) // g) for o, e in zip(starts, exts)} == {(a, f) for a in range(16) for f in frames}
    hashes, hs = S.window_hashes(_dev(bytes(blob)), starts, [len(e) // g for e in exts], cfg)
    got = hashes.cpu().numpy().view(np.uint32)
    assert hs[-1] == got.size == sum(max(0, len(e) // g - W + 1) for e in exts)
    want = {}  # (the host hashes of equal extents are computed once)
    for b, e in enumerate(exts):
        if e not in want:
            want[e] = S.host_hashes(e, cfg)
        assert np.array_equal(got[hs[b]:hs[b + 1]], want[e]), (b, starts[b] % 16, len(e) // g)
    assert hs[1] == hs[0]  # W - 1 frames: no position


def test_hashes_equal_kat(kat):
    """Every KAT message of each config in one batch, against the model's recorded digests."""
    by_cfg = {}
    for e in kat["hashes"]:
        by_cfg.setdefault(json.dumps(e["config"], sort_keys=True), []).append(e)
    for entries in by_cfg.values():
        cfg = C(entries[0]["config"])
        g = cfg.granularity
        msgs = [K.message_bytes(e["message"]) for e in entries]
        starts, at = [], 3
        for m in msgs:
            starts.append(at)
            at += len(m)
        blob = b"\xc3" * 3 + b"".join(msgs)
        hashes, hs = S.window_hashes(_dev(blob), starts, [len(m) // g for m in msgs], cfg)
        got = hashes.cpu().numpy().view(np.uint32)
        for b, e in enumerate(entries):
            h = got[hs[b]:hs[b + 1]]
            assert h.size == e["count"] and K.digest(h) == e["sha256"], e["message"]
            assert h[:4].tolist() == e["first"] and h[-1:].tolist() == e["last"]


def test_hashes_all_ff_wide_window():
    """window_bits 12, g = 6, all 0xFF: both halves wrap 2^16 many times; the closed form holds at every position."""
    cfg = S.SegmenterConfig(12, 1, 6, 1024)
    L = cfg.window_bytes
    n = cfg.window_frames + S.tile_frames() + 9
    data = b"\xff" * (n * 6)
    hashes, hs = S.window_hashes(_dev(b"\x00" * 5 + data), [5], [n], cfg)
    got = hashes.cpu().numpy().view(np.uint32)
    want = ((255 * L) & 0xFFFF) | (((255 * L * (L + 1) // 2) & 0xFFFF) << 16)
    assert got.size == n - cfg.window_frames + 1 and (got == want).all()
    assert np.array_equal(got, S.host_hashes(data, cfg))


def test_variable_granularity_and_errors():
    """g = 7 and 64 take the variable path; an extent of 2^32 frames is an error and nothing is read."""
    rng = np.random.default_rng(22)
    for g in (7, 64):
        cfg = S.SegmenterConfig(3, 0, g, 64)
        data = rng.integers(0, 256, 300 * g + 5, dtype=np.uint8).tobytes()
        hashes, _ = S.window_hashes(_dev(data), [5], [300], cfg)
        assert np.array_equal(hashes.cpu().numpy().view(np.uint32), S.host_hashes(data[5:], cfg))
    cfg = S.SegmenterConfig(4, 1, 1, 1024)
    with pytest.raises(ValueError):
        S.window_hashes(_dev(bytes(64)), [0], [2**32], cfg)
    # through the C ABI: the sizes are read on the device, the status comes back from there
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    sz = torch.full((1,), 2**32, dtype=torch.int64, device=DEV)
    out = S.DeviceHits.new(1, 64, 8, DEV)
    filt = torch.full((cfg.filter_words,), -1, dtype=torch.int64, device=DEV)
    S.scan_into(out, _dev(bytes(64)), off, sz, filt, cfg)
    assert out.status() == N.RPP_INVALID_ARGUMENT and out.count() == 0


# ---- index ----

def _index_blocks(rng, cfg):
    W, g, step = cfg.window_frames, cfg.granularity, cfg.step_frames
    q = 4 * W + 3
    zrz = bytes(q * g) + rng.integers(0, 256, q * g, dtype=np.uint8).tobytes() + bytes(q * g) + b"\x5a" * (q * g)
    return [rng.integers(0, 256, (W - 1) * g, dtype=np.uint8).tobytes(),
            rng.integers(0, 256, W * g, dtype=np.uint8).tobytes(),
            rng.integers(0, 256, (5 * W + step // 2 + 1) * g, dtype=np.uint8).tobytes(),
            rng.integers(0, 256, (300 * W + 7) * g, dtype=np.uint8).tobytes(),  # more slots than one workgroup's waves
            zrz, bytes((3 * W + 1) * g)]


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_index_equals_host(shift, g):
    cfg = S.SegmenterConfig(4, shift, g, 4096)
    blocks = _index_blocks(np.random.default_rng(23), cfg)
    offs, at = [], 1
    for b in blocks:
        offs.append(at)
        at += len(b) + 3
    blob = bytearray(b"\xc3" * (at + 16))
    for o, b in zip(offs, blocks):
        blob[o:o + len(b)] = b
    idx = S.BlockIndex.build(_dev(bytes(blob)), offs, [len(b) // g for b in blocks], cfg)
    gf = np.zeros(cfg.filter_words, np.uint64)
    block_or = np.zeros(cfg.filter_words, np.uint64)
    filters = _u64(idx.block_filters)
    for b, blk in enumerate(blocks):
        want = S.host_index(blk, cfg, gf)
        h, o, e = idx.slots(b)
        assert np.array_equal(h, want.hash) and np.array_equal(o, want.offset) and np.array_equal(e, want.entered), b
        assert filters[b].tobytes() == want.block_filter.tobytes(), b
        block_or |= filters[b]
    assert idx.slots(0)[0].size == 0 and idx.slots(1)[0].size == 1
    assert _u64(idx.global_filter).tobytes() == gf.tobytes() == block_or.tobytes()
    # zeros / random / zeros / 0x5A: one all-zero window and one all-0x5A window are entered
    h, o, e = idx.slots(4)
    L = cfg.window_bytes
    rep = [blocks[4][int(x) * g:int(x) * g + L] for x in o]
    zero_slots = [i for i, w in enumerate(rep) if w == bytes(L)]
    a5_slots = [i for i, w in enumerate(rep) if w == b"\x5a" * L]
    assert len(zero_slots) > 2 and len(a5_slots) > 1
    assert [int(e[i]) for i in zero_slots] == [1] + [0] * (len(zero_slots) - 1)
    assert [int(e[i]) for i in a5_slots] == [1] + [0] * (len(a5_slots) - 1)
    # two calls into one global filter
    shared = torch.zeros(cfg.filter_words, dtype=torch.int64, device=DEV)
    one = S.BlockIndex.build(_dev(blocks[2]), [0], [len(blocks[2]) // g], cfg, shared)
    two = S.BlockIndex.build(_dev(blocks[3]), [0], [len(blocks[3]) // g], cfg, shared)
    assert _u64(shared).tobytes() == (_u64(one.block_filters)[0] | _u64(two.block_filters)[0]).tobytes()


def test_index_equals_kat(kat):
    for e in kat["index"]:
        cfg = C(e["config"])
        blk = K.message_bytes(e["message"])
        idx = S.BlockIndex.build(_dev(b"\xc3" + blk), [1], [len(blk) // cfg.granularity], cfg)
        h, o, en = idx.slots(0)
        assert (h.tolist(), o.tolist(), en.tolist()) == (e["hash"], e["offset"], e["entered"]), e["message"]
        assert _u64(idx.block_filters)[0].tobytes().hex() == e["block_filter"]


# ---- scan ----

@pytest.fixture(scope="module")
def planted_case():
    cfg = S.SegmenterConfig(6, 1, 2, 4096)
    block, extent, plants = K.planted({"window_bits": 6, "increment_shift": 1, "granularity": 2, "filter_bits": 4096})
    return cfg, block, extent, plants


def test_scan_planted(planted_case, kat):
    cfg, block, extent, plants = planted_case
    g, W = cfg.granularity, cfg.window_frames
    n = len(extent) // g
    idx = S.BlockIndex.build(_dev(block), [0], [len(block) // g], cfg)
    filt = idx.block_filters[0].contiguous()
    d_ext = _dev(b"\xc3" * 7 + extent)
    pos, hashes, count = S.scan(d_ext, 7, n, filt, cfg)
    hp, hh, hc = S.host_scan(extent, _u64(filt), cfg)
    assert count == hc == pos.size and np.array_equal(pos, hp) and np.array_equal(hashes, hh)
    assert (np.diff(pos.astype(np.int64)) > 0).all()
    want = [e for e in kat["scan"] if e["config"]["window_bits"] == 6][0]
    assert [[int(p), int(h)] for p, h in zip(pos, hashes)] == want["hits"] and plants == [tuple(p) for p in want["plants"]]
    _, off, entered = idx.slots(0)
    hit = set(pos.tolist())
    planted_hits = 0
    for p, o, frames in plants:
        for so, e in zip(off.tolist(), entered.tolist()):
            if e and o <= so and so + W <= o + frames:
                assert p + (so - o) in hit
                planted_hits += 1
    assert planted_hits >= 10
    # a capacity one below the count: overflow status, the full count, a correct prefix
    out = S.DeviceHits.new(1, n, count - 1, DEV)
    d_off = torch.tensor([7], dtype=torch.int64, device=DEV)
    d_sz = torch.tensor([n], dtype=torch.int64, device=DEV)
    out.hits.fill_(-1)
    S.scan_into(out, d_ext, d_off, d_sz, filt, cfg)
    assert out.status() == N.RPP_OUTPUT_TOO_SMALL and out.count() == count
    h = out.host()
    assert np.array_equal(h["pos"], pos[:-1]) and np.array_equal(h["hash"], hashes[:-1])
    assert out.hit_start.cpu().tolist() == [0, count]
    p2, h2, c2 = S.scan(d_ext, 7, n, filt, cfg, capacity=count - 1)
    assert c2 == count and np.array_equal(p2, pos[:-1]) and np.array_equal(h2, hashes[:-1])
    # an empty filter: no hit; a full one: every position
    empty = torch.zeros(cfg.filter_words, dtype=torch.int64, device=DEV)
    assert S.scan(d_ext, 7, n, empty, cfg)[2] == 0
    full = torch.full((cfg.filter_words,), -1, dtype=torch.int64, device=DEV)
    p3, h3, c3 = S.scan(d_ext, 7, n, full, cfg)
    assert c3 == n - W + 1 and np.array_equal(p3, np.arange(c3)) and np.array_equal(h3, S.host_hashes(extent, cfg))


def test_scan_batch_of_extents(planted_case):
    """Three extents in one call (one shorter than the window): the hit ranges per extent equal the host's."""
    cfg, block, extent, _ = planted_case
    g = cfg.granularity
    filt_host = S.host_index(block, cfg).block_filter
    filt = torch.from_numpy(filt_host.view(np.int64).copy()).to(DEV)
    exts = [extent, extent[:10 * g], extent[33 * g:]]
    offs = [0, len(extent) + 1, len(extent) + 1 + 10 * g + 2]
    blob = bytearray(offs[2] + len(exts[2]))
    for o, e in zip(offs, exts):
        blob[o:o + len(e)] = e
    sizes = [len(e) // g for e in exts]
    out = S.DeviceHits.new(3, sum(sizes), 4096, DEV)
    S.scan_into(out, _dev(bytes(blob)), torch.tensor(offs, dtype=torch.int64, device=DEV),
                torch.tensor(sizes, dtype=torch.int64, device=DEV), filt, cfg)
    assert out.status() == N.RPP_OK
    hs = out.hit_start.cpu().tolist()
    h = out.host()
    for b, e in enumerate(exts):
        p, hh, c = S.host_scan(e, filt_host, cfg)
        assert hs[b + 1] - hs[b] == c
        assert np.array_equal(h["pos"][hs[b]:hs[b + 1]], p) and np.array_equal(h["hash"][hs[b]:hs[b + 1]], hh)
    assert hs[-1] == out.count() and hs[1] == hs[2]


def test_scan_lone_large_extent():
    """One extent of 4 MiB + 5 bytes alone in its call, run twice: byte-identical output equal to the host's."""
    cfg = S.SegmenterConfig(12, 1, 1, 1 << 16)
    rng = np.random.default_rng(25)
    n = 4 * 2**20 + 5
    extent = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    block = rng.integers(0, 256, 2**20, dtype=np.uint8).tobytes()
    extent[1234567:1234567 + 300000] = block[50001:350001]
    extent = bytes(extent)
    idx = S.BlockIndex.build(_dev(block), [0], [len(block)], cfg)
    d_ext = _dev(b"\xc3" * 3 + extent)
    runs = [S.scan(d_ext, 3, n, idx.global_filter, cfg) for _ in range(2)]
    assert runs[0][2] == runs[1][2]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    hp, hh, hc = S.host_scan(extent, _u64(idx.global_filter), cfg)
    assert runs[0][2] == hc and np.array_equal(runs[0][0], hp) and np.array_equal(runs[0][1], hh)
    assert hc >= 300000 // cfg.step_frames - 3


def test_scan_graph_capture(planted_case):
    """One scan call captured in a graph on a side stream and replayed twice."""
    cfg, block, extent, _ = planted_case
    g = cfg.granularity
    n = len(extent) // g
    filt_host = S.host_index(block, cfg).block_filter
    filt = torch.from_numpy(filt_host.view(np.int64).copy()).to(DEV)
    d_ext = _dev(extent)
    d_off = torch.tensor([0], dtype=torch.int64, device=DEV)
    d_sz = torch.tensor([n], dtype=torch.int64, device=DEV)
    out = S.DeviceHits.new(1, n, 4096, DEV)
    S.scan_into(out, d_ext, d_off, d_sz, filt, cfg)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            S.scan_into(out, d_ext, d_off, d_sz, filt, cfg)
    hp, hh, hc = S.host_scan(extent, filt_host, cfg)
    results = []
    for _ in range(2):
        out.hits.fill_(-1)
        out.result.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        results.append((out.count(), out.status(), out.host().tobytes()))
    assert results[0] == results[1] and results[0][0] == hc and results[0][1] == N.RPP_OK
    h = out.host()
    assert np.array_equal(h["pos"], hp) and np.array_equal(h["hash"], hh)


# ---- extend ----

def test_extend_equals_host_and_kat(kat):
    for e in kat["extend"]:
        cfg = C(e["config"])
        ext, block, cands = K.extend_case(e["config"])
        assert [list(c) for c in cands] == e["candidates"]
        for lead in (0, 5):  # (the device copies start at different alignments)
            cd = np.concatenate([S.candidates([c[0]], c[1], lead, 3, c[2], c[3], c[4]) for c in cands])
            got = S.extend(_dev(b"\xc3" * lead + ext), _dev(b"\x3c" * 3 + block), cd, cfg)
            assert [[int(m["off"]), int(m["pos"]), int(m["size"])] for m in got] == e["matches"]
            cd0 = np.concatenate([S.candidates([c[0]], c[1], 0, 0, c[2], c[3], c[4]) for c in cands])
            assert got.tobytes() == S.host_extend(ext, block, cd0, cfg).tobytes()
    # what the cases were built to reach
    m = kat["extend"][1]["matches"]  # g = 3
    W, bframes = 16, 12 * 16 + 5
    assert m[0] == [0, 2 * W, bframes]                    # the block's start and end
    assert m[1] == [3 * W - 2, 5 * W - 2, 2 * W + 4]      # begin and end
    assert m[2] == [4 * W + 3, 20 * W + 1, 4 * W]         # a mismatch inside the neighbouring frame on each side
    assert m[3][2] == 0 and m[4][2] == W and m[5] == [0, 36 * W + 1, 2 * W]


def test_extend_hash_collision_and_long_runs():
    """Two windows with equal hashes and different bytes give size 0; a match of 1 MiB is extended over many steps
    of the wave, with the mismatch at every distance modulo 16 around a step boundary."""
    cfg = S.SegmenterConfig(4, 1, 1, 1024)
    a = bytes([1, 2, 1] + [7] * 13)
    b = bytes([2, 0, 2] + [7] * 13)  # the same sum, the same weighted sum
    assert a != b and S.host_hashes(a, cfg).tolist() == S.host_hashes(b, cfg).tolist()
    got = S.extend(_dev(a), _dev(b), S.candidates([0], 0, 0, 0, 0, 16, 16), cfg)
    assert (int(got[0]["off"]), int(got[0]["pos"]), int(got[0]["size"])) == (0, 0, 0)
    rng = np.random.default_rng(26)
    n = 2**20
    block = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cands, exts = [], []
    for k, cut in enumerate([1000, 1024, 1025, 1039, 1040, 2048 + 15, 5000, n // 2]):
        ext = bytearray(block)
        mid = n // 2
        if mid - 16 - cut - 1 >= 0:
            ext[mid - 16 - cut - 1] ^= 0x80   # the prefix stops after `cut` bytes
        if mid + cut < n:
            ext[mid + cut] ^= 0x80            # the suffix stops after `cut` bytes
        exts.append(bytes(ext))
        cands.append(S.candidates([mid - 16], mid - 16, k * n, 0, 0, n, n))
    cd = np.concatenate(cands)
    got = S.extend(_dev(b"".join(exts)), _dev(block), cd, cfg)
    for k, cut in enumerate([1000, 1024, 1025, 1039, 1040, 2048 + 15, 5000, n // 2]):
        pre = min(cut, n // 2 - 16)
        suf = min(cut, n // 2)
        assert (int(got[k]["off"]), int(got[k]["pos"]), int(got[k]["size"])) == (n // 2 - 16 - pre, n // 2 - 16 - pre,
                                                                                16 + pre + suf), (k, cut)
    assert got.tobytes() == S.host_extend(b"".join(exts), block, cd, cfg).tobytes()


# ---- the joined search, the C++ facade ----

def test_find_candidates(planted_case):
    cfg, block, extent, plants = planted_case
    other = np.random.default_rng(27).integers(0, 256, 777 * cfg.granularity, dtype=np.uint8).tobytes()
    rows = S.find_candidates(extent, [other, block], cfg)
    assert sorted(map(tuple, rows.tolist())) == sorted((p, 1, o, f) for p, o, f in plants)


def test_cpp_segment(planted_case, tmp_path):
    """tests/cpp/segment_test: ricepp_amd::segment_index / segment_scan on the planted case, given as files of
    the block and the extent and a table of the expected hits."""
    exe = ROOT / "tests" / "cpp" / "build" / "segment_test"
    if not exe.exists():
        subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_segment.sh")], check=True)
    cfg, block, extent, plants = planted_case
    (tmp_path / "block.bin").write_bytes(block)
    (tmp_path / "extent.bin").write_bytes(extent)
    r = subprocess.run([str(exe), str(tmp_path / "block.bin"), str(tmp_path / "extent.bin"), str(cfg.window_bits),
                        str(cfg.increment_shift), str(cfg.granularity), str(cfg.filter_bits)] +
                       [f"{p}:{o}:{f}" for p, o, f in plants], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "segment_test: OK" in r.stdout
