"""GPU tests of the Zstandard encoder's `long` word: bytes, sizes, flags and statuses of ``encode_batch(long=1)``
against the host restatement (``host_encode``, which tests/test_zstd_long_host.py pins to libzstd's verdict and to
a plain-Python restatement of the matcher) over the inputs of tests/zstd_long_cases.py, with guard bytes behind
every frame; `long` 0 through the new entry point; tables of different sizes in one workspace; an over-size block
refused before any of it is read; the incompressible scan; and the decode kernels."""

import functools

import numpy as np
import pytest
import torch

import incompressible_cases as IC
import zstd_long_cases as LC
from dwarfs_amd import _native as N
from dwarfs_amd import categorize as CZ
from dwarfs_amd import section as S
from dwarfs_amd import zstd as Z
from dwarfs_amd.lz4 import _upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def expected(options, search, long):
    """[(name, input, host frame, host flag)], computed once per word triple"""
    return [(name, data, *Z.host_encode(data, options, search, long)) for name, data in LC.inputs()]


def encode(blocks, options, search, long, sizes=None):
    """rpp_zstd_encode_batch_long over `blocks` into slots filled with GUARD: (frames, flags, statuses); every byte
    of a slot behind its frame is checked to be GUARD still.  `sizes` replaces the blocks' sizes in the call."""
    flat, offs = _upload(blocks, DEV)
    sizes = [len(b) for b in blocks] if sizes is None else sizes
    n, total = len(blocks), sum(len(b) for b in blocks)
    slots = [Z.bound(len(b)) + 16 for b in blocks]
    out_offs, cap = Z._layout(slots)
    out = torch.full((cap,), GUARD, dtype=torch.uint8, device=DEV)
    got = torch.zeros(n, dtype=torch.int64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    st = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws_bytes = int(N.lib().rpp_zstd_encode_workspace_bytes_long(total, n, long))
    assert (ws_bytes > N.lib().rpp_zstd_encode_workspace_bytes(total, n)) == bool(long)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ptr = Z._ptr
    d_ioff, d_isz, d_ooff = S._i64(offs, DEV), S._i64(sizes, DEV), S._i64(out_offs, DEV)
    assert N.lib().rpp_zstd_encode_batch_long(ptr(flat), ptr(d_ioff), ptr(d_isz), n, options, search, long, ptr(out),
                                              ptr(d_ooff), ptr(got), ptr(fl), ptr(st), total, ptr(ws), ws_bytes,
                                              None) == N.RPP_OK
    torch.cuda.synchronize()
    host, got = out.cpu().numpy(), got.cpu().numpy()
    for o, size, slot in zip(out_offs, got, slots):
        assert (host[o + size:o + slot] == GUARD).all()
    return ([host[o:o + s].tobytes() for o, s in zip(out_offs, got)], fl.cpu().numpy().tolist(),
            st.cpu().numpy().tolist())


def check(cases, frames, flags, status):
    for (name, _, want, flag), got, f, st in zip(cases, frames, flags, status):
        assert st == N.RPP_OK, name
        assert len(got) == len(want) and got == want, name
        assert bool(f) == flag, name


@pytest.mark.parametrize("options,search", LC.PAIRS)
def test_one_batch_is_the_host_encoders(options, search):
    cases = expected(options, search, 1)
    check(cases, *encode([c[1] for c in cases], options, search, 1))


def test_long_0_through_the_new_entry_point():
    for options, search in ((0, 0), (3, 8 | 0x100)):
        cases = expected(options, search, 0)
        blocks = [c[1] for c in cases]
        frames, flags, status = encode(blocks, options, search, 0)
        check(cases, frames, flags, status)
        flat, offs = _upload(blocks, DEV)
        old = Z.encode_batch(flat, offs, [len(b) for b in blocks], options=options, search=search)
        torch.cuda.synchronize()
        data, sizes = old.data.cpu().numpy(), old.sizes.cpu().numpy()
        assert [data[o:o + n].tobytes() for o, n in zip(old.offsets.cpu().numpy(), sizes)] == frames


def test_tables_of_different_sizes_share_a_workspace():
    by_name = {c[0]: c for c in expected(3, 0, 1)}
    mix = [by_name[n] for n in ("size_0", "size_63", "far_gap_100001", "size_1", "three_copies", "size_0", "size_64",
                                "both_sides", "size_32769", "far_rr")]
    check(mix, *encode([c[1] for c in mix], 3, 0, 1))
    for c in mix[2::3]:  # and alone
        check([c], *encode([c[1]], 3, 0, 1))


def test_an_over_size_block_is_refused_unread():
    """The size vector alone says 2^27 + 1: the block has no chunks, so nothing of it is read."""
    by_name = {c[0]: c for c in expected(0, 0, 1)}
    cases = [by_name["far_rr"], by_name["size_64"], by_name["both_sides"]]
    blocks = [c[1] for c in cases]
    sizes = [len(blocks[0]), N.RPP_ZSTD_LONG_MAX_BLOCK + 1, len(blocks[2])]
    frames, flags, status = encode(blocks, 0, 0, 1, sizes)
    assert status == [N.RPP_OK, N.RPP_INVALID_ARGUMENT, N.RPP_OK] and frames[1] == b"" and flags[1] == 0
    check([cases[0], cases[2]], [frames[0], frames[2]], [flags[0], flags[2]], [status[0], status[2]])
    assert Z.LONG_MAX_BLOCK == 1 << 27
    with pytest.raises(ValueError):
        Z.encode_batch(torch.zeros(16, dtype=torch.uint8, device=DEV), [0], [Z.LONG_MAX_BLOCK + 1], long=1)
    L = N.lib()
    assert L.rpp_zstd_encode_batch_long(None, None, None, 0, 0, 0, 2, None, None, None, None, None, 0, None, 0,
                                        None) == N.RPP_INVALID_ARGUMENT
    assert L.rpp_zstd_encode_batch_long(None, None, None, 0, 0, 0, 1, None, None, None, None, None, 0, None, 0,
                                        None) == N.RPP_OK


def test_the_scan_is_the_host_scans():
    case = next(c for c in IC.cases() if c.name == "borderline_far_repeat")
    extents = [case.data, LC.own_inputs()[0][1], b"", dict(LC.own_inputs())["both_sides"]]
    for options, search in ((0, 0), (3, 8 | 0x100)):
        cfg = CZ.IncompressibleConfig(block_size=96 * 1024, generate_fragments=True, options=options, search=search,
                                      long=1)
        host, dev = CZ.scan_pieces(extents, cfg, "cpu"), CZ.scan_pieces(extents, cfg, DEV)
        for key in ("sizes", "verdicts", "totals", "frag_count", "piece_base", "piece_sizes"):
            assert np.array_equal(getattr(host, key), getattr(dev, key)), key
        for e in range(len(extents)):
            assert host.fragments(e) == dev.fragments(e)
    whole = CZ.IncompressibleConfig(long=1)
    assert CZ.scan_pieces([case.data], whole, DEV).verdicts.tolist() == [0]
    assert CZ.scan_pieces([case.data], CZ.IncompressibleConfig(), DEV).verdicts.tolist() == [1]


def test_the_decode_kernels_read_every_frame():
    cases = expected(3, 8 | 0x100, 1) + [("reach_20", LC.reach_20(), *Z.host_encode(LC.reach_20(), 3, 0, 1))]
    back = Z.decompress_many([Z.ZstdBlockDecompressor(c[2], DEV) for c in cases], DEV)
    assert back == [c[1] for c in cases]
    frames, flags, status = encode([LC.reach_20()], 3, 0, 1)  # the 1.5 MiB input's one appearance on the GPU
    assert frames == [cases[-1][2]] and status == [N.RPP_OK] and flags == [0]


def test_python_layer():
    by_name = dict(LC.own_inputs())
    comp = Z.block_compressor_long("zstd:long", DEV)
    assert comp.long == 1 and comp.describe() == "zstd [level=22, long]"
    blocks = [by_name["far_rr"], by_name["size_95"], by_name["three_copies"]]
    want = [Z.host_encode(b, 0, 0, 1) for b in blocks]
    assert comp.compress_many(blocks, keep_bad=True) == [None if flag else frame for frame, flag in want]
    image = comp.compress_many_sections(blocks)
    from dwarfs_amd import block_codec
    assert block_codec.decompress_sections(image, device=DEV, verify=1) == blocks
