"""GPU tests of the incompressible categorizer's kernels.  Everything the batch call writes (sizes, verdicts, totals,
fragment rows, counts, statuses) is compared bit for bit with the host restatement (``device="cpu"``, which
tests/test_incompressible_host.py pins to the Zstandard host encoder and to libzstd's recorded verdicts), in buffers
filled with 0xFF that have guard words behind them; sizes are also compared with ``encode_batch``'s frame sizes
for the same pieces.  The shapes are the smallest at which the two new kernels can go wrong: the chunk-loop carry of
``classify`` (64 and 65 chunks), the tile carry of ``fragments`` (63, 64, 65, 128, 129 pieces), runs that cross a
tile, empty extents, and the ``>=`` edge of the ratio."""

import functools

import numpy as np
import pytest
import torch

import incompressible_cases as IC
from dwarfs_amd import categorize as CZ
from dwarfs_amd import zstd as Z
from dwarfs_amd.lz4 import SEARCH_LAZY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIB, MIB = 1024, 1 << 20
GUARD = 4  # elements (rows) behind every array


def buffers(npieces, nextents, xp):
    """The six result arrays, filled with 0xFF, GUARD elements longer than the call needs."""
    shapes = ((npieces + GUARD, np.int64), (npieces + GUARD, np.int32), ((nextents + GUARD, CZ.TOTALS), np.int64),
              ((npieces + GUARD, 2), np.int64), (nextents + GUARD, np.int32), (npieces + GUARD, np.int32))
    if xp is np:
        return tuple(np.full(s, -1, d) for s, d in shapes)
    return tuple(torch.full(s if isinstance(s, tuple) else (s,), -1, dtype=getattr(torch, np.dtype(d).name), device=DEV)
                 for s, d in shapes)


@functools.lru_cache(maxsize=None)
def host(extents: tuple, cfg):
    flat, offs, szs, base = laid_out(extents, cfg)
    return tuple(a.copy() for a in CZ.host_scan(flat, offs, szs, base, cfg, buffers(len(szs), len(extents), np)))


def laid_out(extents, cfg):
    offs, szs, base = CZ.cut([len(x) for x in extents], cfg.block_size)
    flat = np.frombuffer(b"".join(extents) + bytes(16), np.uint8)
    return flat, offs, szs, base


def check(extents, cfg, with_encoder=True):
    """The batch call against the host call, every byte of every buffer; the arrays of the device's results."""
    extents = tuple(extents)
    flat, offs, szs, base = laid_out(extents, cfg)
    d_in = torch.from_numpy(flat.copy()).to(DEV)
    got = CZ.scan_batch(d_in, offs, szs, base, cfg, buffers(len(szs), len(extents), torch))
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in got)
    want = host(extents, cfg)
    for name, g, w in zip(("sizes", "verdicts", "totals", "frag_rows", "frag_count", "status"), got, want):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8].tolist())
    n, e = len(szs), len(extents)
    assert not got[5][:n].any()
    for a, used in zip(got, (n, n, e, n, e, n)):  # the guards (the host call leaves them too: said again)
        assert (a[used:] == -1).all()
    if not cfg.generate_fragments:
        assert (got[3] == -1).all() and not got[4][:e].any()
    if with_encoder and n:
        enc = Z.encode_batch(d_in, offs.astype(np.int64), szs.astype(np.int64).tolist(), options=cfg.options,
                             search=cfg.search)
        torch.cuda.synchronize()
        assert enc.sizes.cpu().numpy().tolist() == got[0][:n].tolist()
    return got


# ---------------------------------------------------------------------------
# classify
# ---------------------------------------------------------------------------
CLASSIFY_SIZES = (1, 255, 32 * KIB - 1, 32 * KIB, 32 * KIB + 1, 2 * MIB, 2 * MIB + 1)


@functools.lru_cache(maxsize=None)
def classify_extents():
    """An empty extent (no piece), then random and text of every size: each extent one piece at a 4 MiB block."""
    big_r, big_t = IC.random_bytes(9501, 2 * MIB + 1), IC.text(2 * MIB + 1)
    return (b"",) + tuple(src[:n] for n in CLASSIFY_SIZES for src in (big_r, big_t))


def test_classify_sizes_around_the_chunk_and_the_chunk_loop():
    cfg = CZ.IncompressibleConfig(block_size=4 * MIB)
    got = check(classify_extents(), cfg)
    n = 2 * len(CLASSIFY_SIZES)
    assert got[2][0].tolist() == [0, 0, 0, 0, 0]  # the empty extent
    verdicts = got[1][:n].tolist()
    assert verdicts[0::2] == [1] * len(CLASSIFY_SIZES) and verdicts[5::2] == [0] * (len(CLASSIFY_SIZES) - 2)
    # a piece of 64 chunks and one of 65: the wave sum's carry (random: every block Raw, the size is known)
    sizes = dict(zip(((k, s) for s in CLASSIFY_SIZES for k in "rt"), got[0][:n].tolist()))
    assert sizes["r", 2 * MIB] == 2 * MIB + 3 * 64 + 9 and sizes["r", 2 * MIB + 1] == 2 * MIB + 1 + 3 * 65 + 9


def test_classify_many_pieces_per_extent():
    """The same bytes cut at 32 KiB + 1: pieces of two chunks, and extents of 64 pieces and a shorter one."""
    cfg = CZ.IncompressibleConfig(block_size=32 * KIB + 1, generate_fragments=True)
    check(classify_extents()[-2:], cfg)


def test_ratio_edge_size_equals_ratio_times_n():
    data = IC.SC.repeats(9502, 1000)
    size = len(Z.host_encode(data)[0])
    ratio = size / 1000.0
    assert 0 < size < 1000 and ratio * 1000.0 == float(size)  # representable: the product is the size exactly
    above = float(np.nextafter(ratio, 2.0))
    assert above * 1000.0 > float(size)
    for r, verdict in ((ratio, 1), (above, 0)):
        cfg = CZ.IncompressibleConfig(max_ratio=r, generate_fragments=True)
        got = check((data,), cfg)
        assert got[0][0] == size and got[1][0] == verdict and got[2][0].tolist() == [1000, size, 1, verdict, verdict]
        assert got[3][0].tolist() == [verdict, 1000] and got[4][0] == 1


# ---------------------------------------------------------------------------
# fragments
# ---------------------------------------------------------------------------
BS = 256


@functools.lru_cache(maxsize=None)
def pattern(p: str, tail: int = 0, seed: int = 0) -> bytes:
    """An extent of one 256-byte piece per letter, T text (default) or R random (incompressible), then `tail`
    random bytes."""
    rnd = IC.random_bytes(9600 + seed, BS * len(p) + tail)
    text = IC.text(BS)
    return b"".join(text if c == "T" else rnd[BS * i:BS * (i + 1)] for i, c in enumerate(p)) + rnd[BS * len(p):]


def alternating(n: int, first: str = "T") -> str:
    return "".join("TR"[(i + (first == "R")) % 2] for i in range(n))


@functools.lru_cache(maxsize=None)
def fragment_extents():
    out = [("empty_first", b"")]
    for n in (1, 2, 63, 64, 65, 128, 129):
        out.append((f"alternating_{n}", pattern(alternating(n), seed=n)))
    out.append(("empty_between", b""))
    out.append(("alternating_from_R_65", pattern(alternating(65, "R"), seed=1)))
    out.append(("all_default_129", pattern("T" * 129)))
    out.append(("all_incompressible_65", pattern("R" * 65, seed=2)))
    out.append(("run_from_lane_63_to_lane_0", pattern("T" * 63 + "RR" + "T" * 10, seed=3)))
    out.append(("run_ends_with_the_tile", pattern("T" * 60 + "RRRR" + "T" * 64 + "R", seed=4)))
    out.append(("empty_twice", b""))
    out.append(("empty_twice_b", b""))
    out.append(("last_piece_one_byte", pattern("TT", tail=1, seed=5)))
    out.append(("last_piece_one_byte_after_R", pattern("TR" * 32, tail=1, seed=6)))
    out.append(("one_byte", pattern("", tail=1, seed=7)))
    out.append(("empty_last", b""))
    return tuple(out)


def rows_of(got, base, e):
    return got[3][base[e]:base[e] + got[4][e]].tolist()


def run_lengths(p: str, tail: int = 0):
    out = []
    for c, n in [("TR".index(c), BS) for c in p] + ([(1, tail)] if tail else []):
        if out and out[-1][0] == c:
            out[-1][1] += n
        else:
            out.append([c, n])
    return out


@pytest.mark.parametrize("fragments", (True, False))
def test_fragments_mixed_batch(fragments):
    cfg = CZ.IncompressibleConfig(block_size=BS, generate_fragments=fragments)
    names, extents = zip(*fragment_extents())
    got = check(extents, cfg)
    _, _, base = CZ.cut([len(x) for x in extents], BS)
    assert len(set(base.tolist())) < len(base) - 4  # repeated entries: the empty extents
    if not fragments:
        return
    e = dict(zip(names, range(len(names))))
    # the patterns are what they are meant to be: text pieces default, random pieces and the 1-byte piece not
    for n in (1, 2, 63, 64, 65, 128, 129):
        assert rows_of(got, base, e[f"alternating_{n}"]) == run_lengths(alternating(n)), n  # as long as the piece list
        assert got[4][e[f"alternating_{n}"]] == n
    assert rows_of(got, base, e["alternating_from_R_65"]) == run_lengths(alternating(65, "R"))
    assert rows_of(got, base, e["all_default_129"]) == [[0, 129 * BS]]
    assert rows_of(got, base, e["all_incompressible_65"]) == [[1, 65 * BS]]
    assert rows_of(got, base, e["run_from_lane_63_to_lane_0"]) == [[0, 63 * BS], [1, 2 * BS], [0, 10 * BS]]
    assert rows_of(got, base, e["run_ends_with_the_tile"]) == [[0, 60 * BS], [1, 4 * BS], [0, 64 * BS], [1, BS]]
    assert rows_of(got, base, e["last_piece_one_byte"]) == [[0, 2 * BS], [1, 1]]
    assert rows_of(got, base, e["last_piece_one_byte_after_R"])[-1] == [1, BS + 1]
    assert rows_of(got, base, e["one_byte"]) == [[1, 1]]
    for name in ("empty_first", "empty_between", "empty_twice", "empty_twice_b", "empty_last"):
        assert got[4][e[name]] == 0 and got[2][e[name]].tolist() == [0] * 5


def test_fragments_each_extent_alone():
    cfg = CZ.IncompressibleConfig(block_size=BS, generate_fragments=True)
    for name, data in fragment_extents():
        if data:
            check((data,), cfg, with_encoder=False)


# ---------------------------------------------------------------------------
# the categorizer
# ---------------------------------------------------------------------------
def test_reference_families_through_categorize_many():
    by = {c.name: c for c in IC.cases()}
    cfg = CZ.IncompressibleConfig(min_input_size=1000, block_size="8k", generate_fragments=True)
    small = [by["min_input_size_999"].data, IC.text(999), b""]
    files = [small[0], by["random_10000"].data, by["text_10000"].data, small[1], by["categorize_fragments"].data,
             by["min_input_size_10000"].data, small[2],
             [CZ.Hole(4096), by["max_ratio_text"].data, CZ.Hole(10), IC.random_bytes(9701, 3000), CZ.Hole(1)]]
    gpu, cpu = CZ.IncompressibleCategorizer(cfg, DEV), CZ.IncompressibleCategorizer(cfg, "cpu")
    got = gpu.categorize_many(files)
    assert got == cpu.categorize_many(files)
    assert got[0] == got[3] == got[6] == CZ.FileResult(None, None)
    F = CZ.Fragment
    assert got[1].fragments == [F("incompressible", 10000)] and got[2].fragments == [F("<default>", 10000)]
    assert got[4].fragments == [F("<default>", 16384), F("incompressible", 8192), F("<default>", 16384),
                                F("incompressible", 8192), F("<default>", 3072)]
    assert got[5].fragments == [F("incompressible", 10000)]
    assert got[7].fragments == [F("<default>", 4096), F("<default>", 10000), F("<default>", 10), F("incompressible", 3000),
                                F("<default>", 1)]
    # the files without a job sit inside the batch, and the buffer the call built does not hold their bytes
    with_job = sum(len(f) for f in (files[1], files[2], files[4], files[5])) + 10000 + 3000
    assert gpu.last_total_bytes == cpu.last_total_bytes == with_job
    assert with_job + sum(len(s) for s in small) == sum(
        len(p) for f in files for p in CZ.IncompressibleCategorizer._parts(f) if not isinstance(p, CZ.Hole))
    # without the fragment list, and the two ratios on one input
    off = CZ.IncompressibleConfig(min_input_size=1000, block_size="8k")
    got = CZ.IncompressibleCategorizer(off, DEV).categorize_many(files)
    assert got == CZ.IncompressibleCategorizer(off, "cpu").categorize_many(files)
    assert got[2].fragments == [] and got[1].fragments == [F("incompressible", 10000)]
    import json
    from pathlib import Path
    m = json.loads((Path(__file__).resolve().parent / "golden" / "incompressible_kat.json").read_text())["max_ratio"]
    text = by["max_ratio_text"].data
    for ratio, want in ((m["below"], [F("incompressible", len(text))]), (m["above"], [])):
        assert CZ.IncompressibleCategorizer(CZ.IncompressibleConfig(max_ratio=ratio), DEV).categorize(text).fragments == want


@pytest.mark.parametrize("options", (0, 3))
@pytest.mark.parametrize("search", (0, 8 | SEARCH_LAZY))
def test_options_and_search_on_one_mixed_batch(options, search):
    cfg = CZ.IncompressibleConfig(block_size="8k", generate_fragments=True, options=options, search=search)
    extents = tuple(c.data for c in IC.cases() if len(c.data) <= 64 * KIB) + (b"", classify_extents()[10])
    check(extents, cfg)
