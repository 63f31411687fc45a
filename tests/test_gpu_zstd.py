"""GPU tests of the Zstandard block decoder: the three kernels on libzstd's recorded frames and on damaged ones,
the block promise, ZSTD sections beside LZ4, NONE and ricepp sections in one image fragment, and the Python
classes on the device."""

import numpy as np
import pytest
import torch

import zstd_cases as ZC
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import lz4 as L4
from dwarfs_amd import section as S
from dwarfs_amd import zstd as Z

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 48
FILL = 0xA5


def pack(frames, phase=0):
    """The frames in one buffer, frame i at an offset of (phase + i) mod 4, with 0xFF bytes behind each."""
    offs, at = [], 0
    for i, f in enumerate(frames):
        at = (at + 3) // 4 * 4 + (phase + i) % 4
        offs.append(at)
        at += len(f) + 5
    flat = np.full(at + 16, 0xFF, np.uint8)
    for o, f in zip(offs, frames):
        flat[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return torch.from_numpy(flat).to(DEV), offs


def gpu_decode(frames, sizes, max_blocks=None, phase=0, total_out=None):
    """One rpp_zstd_decode_batch: (statuses, outputs, True if every byte outside the outputs is untouched)."""
    d_in, in_offs = pack(frames, phase)
    out_offs, at = [], GUARD
    for n in sizes:
        out_offs.append(at)
        at += n + GUARD + 1  # (odd strides: the outputs are not aligned either)
    out = torch.full((at,), FILL, dtype=torch.uint8, device=DEV)
    if max_blocks is None:
        max_blocks = sum(max(Z.count_blocks(f), 1) for f in frames)
    _, _, st = Z.decode_batch(d_in, in_offs, [len(f) for f in frames], sizes, max_blocks, out=out, out_offsets=out_offs,
                              total_out=total_out)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    mask = np.ones(at, bool)
    for o, n in zip(out_offs, sizes):
        mask[o:o + n] = False
    return st.cpu().numpy(), [host[o:o + n].tobytes() for o, n in zip(out_offs, sizes)], bool((host[mask] == FILL).all())


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_decode_whole_fixture_in_one_batch(phase):
    names, frames, want = zip(*ZC.frames())
    st, outs, intact = gpu_decode(frames, [len(w) for w in want], phase=phase)
    assert (st == N.RPP_OK).all(), [n for n, s in zip(names, st) if s != N.RPP_OK]
    assert intact
    for name, got, w in zip(names, outs, want):
        assert got == w, name


def test_decode_one_frame_per_call():
    for case, data, frames in ZC.cases():  # a frame of every case, and every windowed and checksum frame
        for key in [next(iter(frames))] + [k for k in ("windowed", "checksum") if k in frames]:
            st, outs, intact = gpu_decode([frames[key]], [len(data)])
            assert (int(st[0]), intact) == (N.RPP_OK, True), (case, key)
            assert outs[0] == data, (case, key)


def test_damaged_frames():
    """Per record libzstd's verdict (refused where the RFC is stricter), outputs equal where accepted, nothing
    outside an output written, and the valid frames placed between the damaged ones decode as if alone."""
    good = [(f, data) for _, f, data in ZC.frames() if len(data) <= 2000]
    frames, sizes, expect = [], [], []
    for k, (what, frame, n, accepted, want, rule) in enumerate(ZC.damaged()):
        frames.append(frame)
        sizes.append(n)
        expect.append((what, N.RPP_OK, want) if accepted and not rule else (what, N.RPP_CORRUPT_INPUT, None))
        f, data = good[k % len(good)]
        frames.append(f)
        sizes.append(len(data))
        expect.append((f"valid neighbour of {what}", N.RPP_OK, data))
    frames.append(ZC.COUNT_0_IN_TWO_BYTES)
    sizes.append(4)
    expect.append(("a sequence count of 0 in two bytes", N.RPP_CORRUPT_INPUT, None))
    # (a damaged frame whose block headers cannot be walked is promised one block)
    st, outs, intact = gpu_decode(frames, sizes)
    assert intact
    for (what, want_st, want), got_st, got in zip(expect, st, outs):
        assert got_st == want_st, what
        if want is not None:
            assert got == want, what
    assert {N.RPP_OK, N.RPP_CORRUPT_INPUT} == {int(s) for s in st}


def test_more_blocks_than_promised():
    by_name = {name: (data, fs) for name, data, fs in ZC.cases()}
    small, (big, big_frames) = by_name["sentence_400"], by_name["zeros_300000"]
    frames = [small[1]["l3"], big_frames["l3"], small[1]["l1"]]
    sizes = [len(small[0]), len(big), len(small[0])]
    assert [Z.count_blocks(f) for f in frames] == [1, 3, 1]
    st, outs, intact = gpu_decode(frames, sizes, max_blocks=3)  # the second frame finds 2 slots left
    assert intact
    assert list(st) == [N.RPP_OK, N.RPP_OUTPUT_TOO_SMALL, N.RPP_OK]
    assert outs[0] == small[0] and outs[2] == small[0]
    assert outs[1] == bytes([FILL]) * len(big)  # nothing of it is decoded
    st, outs, _ = gpu_decode(frames, sizes, max_blocks=5)
    assert list(st) == [N.RPP_OK] * 3 and outs[1] == big
    # the same for the output bytes the workspace was sized for
    st, outs, intact = gpu_decode(frames, sizes, total_out=1000)
    assert intact and list(st) == [N.RPP_OK, N.RPP_OUTPUT_TOO_SMALL, N.RPP_OK]
    d = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception):
        Z.decode_batch(d, [0, 8], [8, 8], [1, 1], max_blocks=1)  # fewer blocks promised than frames


def zstd_sections(frames, first_number):
    """BLOCK sections of compression type ZSTD around recorded frames, built with the section helpers."""
    payload, offs = L4._upload(frames, DEV)
    lens = np.array([len(f) for f in frames], np.int64)
    d_fr, d_fl = S._rows([b""] * len(frames), S.FRAME_ROW, DEV)
    headers = S.section_headers_batch(payload, offs, lens, first_number, S.SECTION_TYPE_BLOCK, Z.COMPRESSION_TYPE_ZSTD,
                                      d_fr, d_fl)
    capacity = int(lens.sum()) + len(frames) * (S.HEADER_BYTES + S.FRAME_ROW)
    return S.sections_assemble_batch(headers, payload, offs, lens, capacity, d_fr, d_fl).bytes()


def test_mixed_image_zstd_lz4_none_ricepp():
    by_name = {name: (data, fs) for name, data, fs in ZC.cases()}
    picks = [("prefixes_8000", "l19"), ("below64_20000", "l3"), ("zeros_300000", "l1"), ("sentence_300000", "windowed"),
             ("sentence_400", "checksum"), ("empty", "l3")]
    zstd_part = zstd_sections([by_name[n][1][k] for n, k in picks], 0)
    lz4_blocks = [by_name["sentence_400"][0] * 20, by_name["below256_2000"][0]]  # the second becomes a NONE section
    lz4_part = L4.Lz4BlockCompressor(None, DEV).compress_many_sections(lz4_blocks, None, first_number=len(picks))
    rng = np.random.default_rng(5)
    pix = [(rng.poisson(900, 3000).astype(np.uint16) << 1).byteswap().tobytes() for _ in range(2)]
    meta = '{"endianness":"big","bytes_per_sample":2,"unused_lsb_count":1,"component_count":1}'
    rpp_part = block_codec.compress_many_sections(pix, meta, first_number=len(picks) + 2)
    more = zstd_sections([by_name["below4_700"][1]["l3"]], len(picks) + 4)
    image = zstd_part + lz4_part + rpp_part + more
    secs, bad = S.walk(image)
    assert bad is None
    assert [h.compression for _, h in secs] == [2] * 6 + [3, 0, 7, 7, 2]
    want = [by_name[n][0] for n, _ in picks] + lz4_blocks + pix + [by_name["below4_700"][0]]
    for verify in (0, 1, 2):
        assert block_codec.decompress_sections(image, verify=verify, device=DEV) == want
    at, h = secs[1]  # a flipped payload byte in a ZSTD section: caught before anything is decoded
    broken = bytearray(image)
    broken[at + S.HEADER_BYTES + int(h.length) // 2] ^= 0x40
    with pytest.raises(RuntimeError, match=S.INTEGRITY_ERROR):
        block_codec.decompress_sections(bytes(broken), verify=1, device=DEV)


def test_decompressor_on_the_gpu():
    by_name = {name: (data, fs) for name, data, fs in ZC.cases()}
    data, frames = by_name["prefixes_8000"]
    assert Z.decompress(frames["l3"], DEV) == data
    dec = Z.ZstdBlockDecompressor(frames["l19"], DEV)
    target = bytearray()
    dec.start_decompression(target)
    assert dec.decompress_frame() and bytes(target) == data and not dec.decompress_frame()
    many = [by_name[n] for n in ("below4_300000", "sandwich", "single_byte")]
    assert Z.decompress_many([Z.ZstdBlockDecompressor(f["l1"], DEV) for _, f in many], DEV) == [d for d, _ in many]
    with pytest.raises(RuntimeError, match=r"^failed to decompress frame \(zstd error: -8\)$"):
        Z.decompress(frames["l3"][:-1], DEV)
