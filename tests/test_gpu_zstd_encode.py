"""GPU tests of the Zstandard encode kernels: bytes, sizes, flags and statuses of ``encode_batch`` against the host
restatement (``host_encode``, which tests/test_zstd_encode_host.py pins to libzstd's verdict) over the inputs of
tests/zstd_enc_cases.py, the decode round trip, BLOCK sections, and the batch-level errors."""

import functools

import numpy as np
import pytest
import torch

import zstd_enc_cases as EC
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import section as S
from dwarfs_amd import zstd as Z
from dwarfs_amd.lz4 import _upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def expected():
    """[(name, input, host frame, host flag)], computed once"""
    return [(name, data, *Z.host_encode(data)) for name, data in EC.inputs()]


def encode(blocks, shift=0):
    """encode_batch over `blocks`, the inputs placed at offsets that are `shift` mod 4: (frames, flags, statuses)."""
    flat, offs = _upload([bytes(shift) + b for b in blocks], DEV)
    res = Z.encode_batch(flat, offs + shift, [len(b) for b in blocks])
    torch.cuda.synchronize()
    data, sizes = res.data.cpu().numpy(), res.sizes.cpu().numpy()
    frames = [data[o:o + n].tobytes() for o, n in zip(res.offsets.cpu().numpy(), sizes)]
    return frames, res.flags.cpu().numpy().tolist(), res.status.cpu().numpy().tolist()


def check(cases, frames, flags, status):
    for (name, _, want, flag), got, f, st in zip(cases, frames, flags, status):
        assert st == N.RPP_OK, name
        assert len(got) == len(want) and got == want, name
        assert bool(f) == flag, name


def test_one_batch_and_reversed():
    cases = expected()
    check(cases, *encode([c[1] for c in cases]))
    back = cases[::-1]
    check(back, *encode([c[1] for c in back]))


def test_each_input_alone():
    for case in expected():
        check([case], *encode([case[1]]))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_inputs_at_every_offset_mod_4(shift):
    cases = expected()
    check(cases, *encode([c[1] for c in cases], shift))


def test_guard_bytes_around_every_output_region():
    cases = expected()
    blocks = [c[1] for c in cases]
    guard = 48
    flat, offs = _upload(blocks, DEV)
    bounds = [Z.bound(len(b)) for b in blocks]
    out_offs, at = [], 0
    for bd in bounds:  # guard, region, guard; regions at every alignment
        out_offs.append(at + guard)
        at += guard + bd + guard + 1
    out = torch.full((at,), 0xA5, dtype=torch.uint8, device=DEV)
    n = len(blocks)
    total = sum(len(b) for b in blocks)
    sizes = torch.zeros(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    status = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws_bytes = int(N.lib().rpp_zstd_encode_workspace_bytes(total, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ptr = Z._ptr
    d_ioff, d_isz, d_ooff = S._i64(offs, DEV), S._i64([len(b) for b in blocks], DEV), S._i64(out_offs, DEV)
    assert N.lib().rpp_zstd_encode_batch(ptr(flat), ptr(d_ioff), ptr(d_isz), n, ptr(out), ptr(d_ooff), ptr(sizes),
                                         ptr(flags), ptr(status), total, ptr(ws), ws_bytes, None) == N.RPP_OK
    torch.cuda.synchronize()
    host, got_sizes = out.cpu().numpy(), sizes.cpu().numpy()
    for (name, _, want, _), o, bd, size in zip(cases, out_offs, bounds, got_sizes):
        assert host[o:o + size].tobytes() == want, name
        assert (host[o + size:o + bd + guard] == 0xA5).all() and (host[o - guard:o] == 0xA5).all(), name
    assert status.cpu().numpy().tolist() == [N.RPP_OK] * n


def test_decode_round_trip_of_device_frames():
    cases = expected()
    frames, _, _ = encode([c[1] for c in cases])
    d_in, offs = _upload(frames, DEV)
    blocks = sum(Z.count_blocks(f) for f in frames)
    sizes = [len(c[1]) for c in cases]
    out, out_offs, status = Z.decode_batch(d_in, offs, [len(f) for f in frames], sizes, blocks)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [N.RPP_OK] * len(cases)
    host = out.cpu().numpy()
    for (name, data, _, _), o, n in zip(cases, out_offs, sizes):
        assert host[o:o + n].tobytes() == data, name


def test_multi_chunk_inputs_decode_right():
    by_name = {c[0]: c for c in expected()}
    for name in ("repeat_across_chunks", "source_in_previous_chunk"):
        data = by_name[name][1]
        frame = Z.ZstdBlockCompressor(device=DEV).compress(data)
        assert len(EC.sections(frame)) == 2 and frame == by_name[name][2], name
        assert Z.decompress(frame, DEV) == data, name


def test_sections_with_a_block_that_does_not_shrink():
    by_name = {c[0]: c[1] for c in expected()}
    names = ["sentence_18000", "random_5000", "skewed_full_range", "empty", "zeros_70000"]
    blocks = [by_name[n] for n in names]
    image = Z.ZstdBlockCompressor(device=DEV).compress_many_sections(blocks, first_number=3)
    assert block_codec.decompress_sections(image, device=DEV, verify=2) == blocks
    secs, bad_at = S.walk(image)
    assert bad_at is None
    kinds = [h.compression for _, h in secs]  # the section header's compression field
    assert kinds == [2, 0, 2, 0, 2]  # random bytes and the empty block do not shrink: NONE


def test_a_promise_smaller_than_the_batch():
    blocks = [EC.K.rnd(1, 40000, 4), EC.K.rnd(2, 40000, 4), b""]
    flat, offs = _upload(blocks, DEV)
    n, total = len(blocks), 1000  # promises one chunk per block; the batch holds four
    out_offs, cap = Z._layout([Z.bound(len(b)) for b in blocks])
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    status = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws_bytes = int(N.lib().rpp_zstd_encode_workspace_bytes(total, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ptr = Z._ptr
    d_ioff, d_isz, d_ooff = S._i64(offs, DEV), S._i64([len(b) for b in blocks], DEV), S._i64(out_offs, DEV)
    assert N.lib().rpp_zstd_encode_batch(ptr(flat), ptr(d_ioff), ptr(d_isz), n, ptr(out), ptr(d_ooff), ptr(sizes),
                                         ptr(flags), ptr(status), total, ptr(ws), ws_bytes, None) == N.RPP_OK
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [N.RPP_INVALID_ARGUMENT] * n
    assert bool((out == 0xA5).all())


def test_an_empty_block_inside_a_batch():
    blocks = [EC.K.rnd(3, 3000, 4), b"", EC.K.rnd(4, 3000, 4)]
    frames, flags, status = encode(blocks)
    assert status == [N.RPP_OK] * 3
    assert frames == [Z.host_encode(b)[0] for b in blocks]
    assert frames[1] == bytes.fromhex("28b52ffd2000010000") and flags == [0, 1, 0]
