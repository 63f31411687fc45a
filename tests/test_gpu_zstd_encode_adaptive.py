"""GPU tests of the Zstandard encode kernels with the options word (1: per-block table modes, 2: repeat offsets,
3: both): bytes, sizes, flags and statuses of ``encode_batch`` against the host restatement (``host_encode``, which
tests/test_zstd_encode_adaptive_host.py pins to libzstd's verdict) over the inputs of
tests/zstd_enc_adaptive_cases.py, the decode round trip on the GPU, BLOCK sections, and options 0 through the new
entry point."""

import functools

import pytest
import torch

import zstd_enc_adaptive_cases as AC
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import section as S
from dwarfs_amd import zstd as Z
from dwarfs_amd.lz4 import _upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def expected(options):
    """[(name, input, host frame, host flag)], computed once per options word"""
    return [(name, data, *Z.host_encode(data, options)) for name, data in AC.inputs()]


def encode(blocks, options):
    """encode_batch over `blocks`: (frames, flags, statuses)."""
    flat, offs = _upload(blocks, DEV)
    res = Z.encode_batch(flat, offs, [len(b) for b in blocks], options=options)
    torch.cuda.synchronize()
    data, sizes = res.data.cpu().numpy(), res.sizes.cpu().numpy()
    frames = [data[o:o + n].tobytes() for o, n in zip(res.offsets.cpu().numpy(), sizes)]
    return frames, res.flags.cpu().numpy().tolist(), res.status.cpu().numpy().tolist()


def check(cases, frames, flags, status):
    for (name, _, want, flag), got, f, st in zip(cases, frames, flags, status):
        assert st == N.RPP_OK, name
        assert len(got) == len(want) and got == want, name
        assert bool(f) == flag, name


@pytest.mark.parametrize("options", AC.OPTIONS)
def test_one_batch_and_the_gpu_decoder(options):
    cases = expected(options)
    frames, flags, status = encode([c[1] for c in cases], options)
    check(cases, frames, flags, status)
    back = Z.decompress_many([Z.ZstdBlockDecompressor(f, DEV) for f in frames], DEV)
    assert back == [c[1] for c in cases]


@pytest.mark.parametrize("options", AC.OPTIONS)
def test_batches_of_one_block_and_empty_blocks(options):
    by_name = {c[0]: c for c in expected(options)}
    for name in ("records_two_chunks", "interleaved_mixed", "adaptive_sequences_1", "adaptive_sequences_65",
                 "dominant_50_14", "wide_alphabets", "same_offset_across_chunks", "random_two_chunks", "empty",
                 "single_byte"):
        check([by_name[name]], *encode([by_name[name][1]], options))
    mix = [by_name[n] for n in ("empty", "records_600", "empty", "empty", "rotating_one_code", "empty")]
    frames, flags, status = encode([c[1] for c in mix], options)
    check(mix, frames, flags, status)
    assert frames[0] == bytes.fromhex("28b52ffd2000010000") and flags == [1, 0, 1, 1, 0, 1]


def test_sections_with_a_block_that_does_not_shrink():
    by_name = dict(AC.inputs())
    names = ["records_600", "random_two_chunks", "interleaved_mixed", "empty", "wide_alphabets"]
    blocks = [by_name[n] for n in names]
    comp = Z.ZstdBlockCompressor(device=DEV, options=Z.ENC_ADAPTIVE)
    image = comp.compress_many_sections(blocks, first_number=3)
    assert block_codec.decompress_sections(image, device=DEV, verify=1) == blocks
    secs, bad_at = S.walk(image)
    assert bad_at is None
    assert [h.compression for _, h in secs] == [2, 0, 2, 0, 2]  # random bytes and the empty block: NONE
    assert comp.compress(by_name["records_600"]) == Z.host_encode(by_name["records_600"], 3)[0]
    assert comp.clone().compress_many(blocks[:1]) == [Z.host_encode(blocks[0], 3)[0]]


def test_options_0_through_the_new_entry_point():
    cases = expected(0)
    blocks = [c[1] for c in cases]
    frames, flags, status = encode(blocks, 0)
    check(cases, frames, flags, status)
    flat, offs = _upload(blocks, DEV)
    old = Z.ZstdBlockCompressor(device=DEV).compress_many(blocks, keep_bad=True)  # (options 0 is the default)
    assert [None if f else frame for frame, f in zip(frames, flags)] == old
    # ... and the old entry point itself
    n, total = len(blocks), sum(len(b) for b in blocks)
    out_offs, cap = Z._layout([Z.bound(len(b)) for b in blocks])
    out = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    st = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws_bytes = int(N.lib().rpp_zstd_encode_workspace_bytes(total, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ptr = Z._ptr
    d_ioff, d_isz, d_ooff = S._i64(offs, DEV), S._i64([len(b) for b in blocks], DEV), S._i64(out_offs, DEV)
    assert N.lib().rpp_zstd_encode_batch(ptr(flat), ptr(d_ioff), ptr(d_isz), n, ptr(out), ptr(d_ooff), ptr(sizes),
                                         ptr(fl), ptr(st), total, ptr(ws), ws_bytes, None) == N.RPP_OK
    torch.cuda.synchronize()
    host, got = out.cpu().numpy(), sizes.cpu().numpy()
    assert [host[o:o + s].tobytes() for o, s in zip(out_offs, got)] == frames
    assert fl.cpu().numpy().tolist() == flags and st.cpu().numpy().tolist() == [N.RPP_OK] * n
