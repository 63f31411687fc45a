"""GPU tests of the deeper match search (rpp_lz4_deep_search_kernel behind rpp_lz4_encode_batch_search and
rpp_zstd_encode_batch_search): for every search word the whole list of tests/search_cases.py in one batch, bytes,
sizes, flags and statuses against the host restatement (which tests/test_search_host.py pins to the definition
and to liblz4's and libzstd's verdict), guard bytes around every output region, the decode round trip on the GPU,
a batch larger than promised, and the Python layer on the device."""

import functools
import random

import numpy as np
import pytest
import torch

import search_cases as SC
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import lz4
from dwarfs_amd import section as S
from dwarfs_amd import zstd as Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 64, 0xA5
SHUFFLED = (2, 8 | SC.LAZY)  # the words that get a second batch in another order


@functools.lru_cache(maxsize=None)
def expected(codec, search):
    """[(name, input, host bytes, host flag)], computed once per codec ("lz4", or the zstd options word) and
    search word"""
    if codec == "lz4":
        return [(name, data, *lz4.host_encode(data, search)) for name, data in SC.inputs()]
    return [(name, data, *Z.host_encode(data, codec, search)) for name, data in SC.inputs()]


def encode(cases, codec, search, total=None):
    """One *_encode_batch_search call over the cases' inputs into regions with guard bytes between them:
    (return value, outputs, flags, statuses, whether every guard byte stands)."""
    blocks = [c[1] for c in cases]
    flat, offs = lz4._upload(blocks, DEV)
    bound = lz4.bound if codec == "lz4" else Z.bound
    n, sizes_in = len(blocks), [len(b) for b in blocks]
    out_offs, at = [], GUARD
    for s in sizes_in:
        out_offs.append(at)
        at += (bound(s) + 15) // 16 * 16 + GUARD
    out = torch.full((at,), FILL, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    status = torch.zeros(n, dtype=torch.int32, device=DEV)
    total = sum(sizes_in) if total is None else total
    L, ptr = N.lib(), lz4._ptr
    ws_bytes = int((L.rpp_lz4_encode_workspace_bytes if codec == "lz4" else L.rpp_zstd_encode_workspace_bytes)(total, n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    d_ioff, d_isz, d_ooff = S._i64(offs, DEV), S._i64(sizes_in, DEV), S._i64(out_offs, DEV)
    if codec == "lz4":
        ret = L.rpp_lz4_encode_batch_search(ptr(flat), ptr(d_ioff), ptr(d_isz), n, search, ptr(out), ptr(d_ooff),
                                            ptr(sizes), ptr(flags), ptr(status), total, ptr(ws), ws_bytes, None)
    else:
        ret = L.rpp_zstd_encode_batch_search(ptr(flat), ptr(d_ioff), ptr(d_isz), n, codec, search, ptr(out),
                                             ptr(d_ooff), ptr(sizes), ptr(flags), ptr(status), total, ptr(ws),
                                             ws_bytes, None)
    torch.cuda.synchronize()
    host, got = out.cpu().numpy(), sizes.cpu().numpy()
    outside = np.ones(at, bool)
    for o, s in zip(out_offs, sizes_in):
        outside[o:o + bound(s)] = False
    intact = bool((host[outside] == FILL).all())
    return (ret, [host[o:o + s].tobytes() for o, s in zip(out_offs, got)], flags.cpu().numpy().tolist(),
            status.cpu().numpy().tolist(), intact)


def check(cases, result):
    ret, outs, flags, status, intact = result
    assert ret == N.RPP_OK and intact
    for (name, _, want, flag), got, f, st in zip(cases, outs, flags, status):
        assert st == N.RPP_OK, name
        assert len(got) == len(want) and got == want, name
        assert bool(f) == flag, name


@pytest.mark.parametrize("search", SC.WORDS)
def test_lz4_one_batch_per_word(search):
    cases = expected("lz4", search)
    result = encode(cases, "lz4", search)
    check(cases, result)
    flat, offs = lz4._upload(result[1], DEV)
    out, out_offs, st = lz4.decode_batch(flat, offs, [len(b) for b in result[1]], [len(c[1]) for c in cases])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert st.cpu().numpy().tolist() == [N.RPP_OK] * len(cases)
    assert [host[o:o + len(c[1])].tobytes() for o, c in zip(out_offs, cases)] == [c[1] for c in cases]
    if search in SHUFFLED:
        again = list(cases)
        random.Random(search).shuffle(again)
        check(again, encode(again, "lz4", search))


@pytest.mark.parametrize("search", SC.WORDS)
def test_zstd_one_batch_per_word(search):
    cases = expected(3, search)
    result = encode(cases, 3, search)
    check(cases, result)
    back = Z.decompress_many([Z.ZstdBlockDecompressor(f, DEV) for f in result[1]], DEV)
    assert back == [c[1] for c in cases]
    if search in SHUFFLED:
        again = list(expected(0, search))
        random.Random(search + 1).shuffle(again)
        check(again, encode(again, 0, search))


def test_depth_1_and_search_0_through_the_new_entry_points():
    for codec in ("lz4", 0, 3):
        cases = expected(codec, 0)
        assert [c[2] for c in cases] == [c[2] for c in expected(codec, 1)]
        check(cases, encode(cases, codec, 0))  # the greedy kernel behind the new call


def test_a_batch_larger_than_promised_and_invalid_words():
    cases = expected("lz4", 8 | SC.LAZY)[-6:]
    for codec in ("lz4", 3):
        ret, outs, flags, status, intact = encode(cases, codec, 8 | SC.LAZY, total=SC.CHUNK)
        assert ret == N.RPP_OK and intact
        assert status == [N.RPP_INVALID_ARGUMENT] * len(cases) and outs == [b""] * len(cases)
        for bad in (3, 16, SC.LAZY, 0x200 | 2, 1 << 31):
            assert encode(cases[:1], codec, bad)[0] == N.RPP_INVALID_ARGUMENT


def test_python_layer_on_the_device():
    by_name = dict(SC.inputs())
    names = ["older_is_longer_8", "climb_3", "repeats_32769", "records_600", "zeros_then_zeros"]
    blocks = [by_name[n] for n in names]
    word = 8 | lz4.SEARCH_LAZY
    for comp in (lz4.Lz4BlockCompressor(9, DEV, search=word), block_codec.block_compressor("lz4hc:level=9:depth=8:lazy=1", DEV),
                 block_codec.block_compressor("lz4:depth=8:lazy=1", DEV).clone()):
        assert comp.search == word
        got = comp.compress_many(blocks)
        assert got == [lz4.frame_header(len(b)) + lz4.host_encode(b, word)[0] for b in blocks]
        assert [lz4.decompress(g, DEV) for g in got[:2]] == blocks[:2]
    for comp in (Z.ZstdBlockCompressor(device=DEV, options=3, search=word),
                 Z.block_compressor("zstd:level=3:depth=8:lazy=1", DEV)):
        assert comp.search == word and comp.clone().search == word
        want = [Z.host_encode(b, comp.options, word)[0] for b in blocks]
        assert comp.compress_many(blocks) == want
        assert Z.decompress_many([Z.ZstdBlockDecompressor(f, DEV) for f in want], DEV) == blocks
    image = lz4.Lz4BlockCompressor(9, DEV, search=4).compress_many_sections(blocks, first_number=2)
    assert block_codec.decompress_sections(image, device=DEV, verify=1) == blocks
