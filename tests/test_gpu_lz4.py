"""GPU tests of the LZ4 block codec: the decode kernel on liblz4's blocks and on damaged ones, the encode
kernels against their host restatement byte for byte, and LZ4 / NONE / ricepp sections in one image fragment."""

import ctypes as C

import numpy as np
import pytest
import torch

import lz4_cases as LC
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import lz4 as Z
from dwarfs_amd import section as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 48
FILL = 0xA5


def pack_odd(blocks):
    """The blocks in one buffer, each at an odd byte offset, with room between them."""
    offs, at = [], 1
    for b in blocks:
        offs.append(at)
        at += len(b) + 2
        at |= 1
    flat = np.full(at + 16, FILL, np.uint8)
    for o, b in zip(offs, blocks):
        flat[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(flat).to(DEV), offs


def gpu_decode(blocks, sizes):
    """One rpp_lz4_decode_batch: (statuses, outputs, True if every byte outside the outputs is untouched)."""
    d_in, in_offs = pack_odd(blocks)
    out_offs, at = [], GUARD
    for n in sizes:
        out_offs.append(at)
        at += n + GUARD + 1  # (odd strides: the outputs are not aligned either)
    out = torch.full((at,), FILL, dtype=torch.uint8, device=DEV)
    _, _, st = Z.decode_batch(d_in, in_offs, [len(b) for b in blocks], sizes, out=out, out_offsets=out_offs)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    mask = np.ones(at, bool)
    for o, n in zip(out_offs, sizes):
        mask[o:o + n] = False
    return st.cpu().numpy(), [host[o:o + n].tobytes() for o, n in zip(out_offs, sizes)], bool((host[mask] == FILL).all())


def test_decode_whole_fixture_in_one_batch():
    blocks, want = [], []
    for _, data, d, h in LC.cases():
        blocks += [d, h]
        want += [data, data]
    st, outs, intact = gpu_decode(blocks, [len(w) for w in want])
    assert (st == N.RPP_OK).all(), st
    assert intact
    for (name, *_), got, w in zip([c for c in LC.cases() for _ in (0, 1)], outs, want):
        assert got == w, name


def test_damaged_blocks_match_the_host_decoder():
    """Statuses and bytes equal the host decoder's (which starts from the same fill), nothing outside an output
    is written, and the valid blocks placed between the damaged ones decode as if alone."""
    good = [(d, data) for _, data, d, _ in LC.cases() if len(data) <= 600]
    blocks, sizes, expect = [], [], []
    for k, (what, block, n, _, _) in enumerate(LC.damaged()):
        blocks.append(block)
        sizes.append(n)
        src = np.frombuffer(block, np.uint8)
        buf = np.full(max(n, 1), FILL, np.uint8)
        st = N.lib().rpp_lz4_host_decode(src.ctypes.data_as(C.c_void_p), len(src), buf.ctypes.data_as(C.c_void_p), n)
        expect.append((what, st, buf[:n].tobytes()))
        d, data = good[k % len(good)]
        blocks.append(d)
        sizes.append(len(data))
        expect.append((f"valid neighbour of {what}", N.RPP_OK, data))
    st, outs, intact = gpu_decode(blocks, sizes)
    assert intact
    for (what, want_st, want), got_st, got in zip(expect, st, outs):
        assert got_st == want_st, what
        assert got == want, what
    assert {N.RPP_OK, N.RPP_CORRUPT_INPUT} == {int(s) for s in st}


def gpu_encode(inputs):
    d_in, offs = Z._upload(inputs, DEV)
    res = Z.encode_batch(d_in, offs, [len(b) for b in inputs])
    torch.cuda.synchronize()
    res.check()
    data, o, n = res.data.cpu().numpy(), res.offsets.cpu().numpy(), res.sizes.cpu().numpy()
    return [data[a:a + b].tobytes() for a, b in zip(o, n)], res.flags.cpu().numpy().astype(bool), res


def test_encode_equals_the_host_restatement_and_round_trips():
    names, inputs = zip(*LC.encoder_inputs())
    host = [Z.host_encode(b) for b in inputs]
    streams, flags, res = gpu_encode(inputs)
    for name, s, f, (hs, hf) in zip(names, streams, flags, host):
        assert s == hs, name
        assert f == hf, name
    again, flags2, _ = gpu_encode(inputs)
    assert again == streams and (flags2 == flags).all()
    # the GPU decodes the GPU's blocks, straight from the encoder's device buffer
    out, offs, st = Z.decode_batch(res.data, res.offsets, res.sizes, [len(b) for b in inputs])
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == N.RPP_OK).all()
    host_out = out.cpu().numpy()
    for name, o, b in zip(names, offs, inputs):
        assert host_out[o:o + len(b)].tobytes() == b, name


def test_encode_reports_a_batch_larger_than_promised():
    inputs = [bytes(100000), bytes(10)]
    d_in, offs = Z._upload(inputs, DEV)
    n = len(inputs)
    d_off, d_sz, d_ooff = S._i64(offs, DEV), S._i64([len(b) for b in inputs], DEV), S._i64([0, 150000], DEV)
    out = torch.zeros(200000, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    status = torch.zeros(n, dtype=torch.int32, device=DEV)
    promised = 20  # far fewer bytes than the blocks hold: the workspace has room for two chunks
    ws_bytes = N.lib().rpp_lz4_encode_workspace_bytes(promised, n)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert N.lib().rpp_lz4_encode_batch(p(d_in), p(d_off), p(d_sz), n, p(out), p(d_ooff), p(sizes),
                                        p(flags), p(status), promised, p(ws), ws_bytes,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)) == N.RPP_OK
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == N.RPP_INVALID_ARGUMENT).all()
    assert int(out.sum().item()) == 0


def test_compressor_and_decompressor_on_the_gpu():
    by_name = dict(LC.encoder_inputs())
    comp = block_codec.block_compressor("lz4hc:level=9", DEV)
    data = by_name["sentence_18000"]
    payload = comp.compress(data)
    assert payload == Z.frame_header(len(data)) + Z.host_encode(data)[0]
    assert Z.decompress(payload, DEV) == data
    with pytest.raises(Z.BadCompressionRatioError):
        comp.compress(by_name["random_4096"])
    with pytest.raises(RuntimeError, match=r"^LZ4: decompression failed \(error: -8\)$"):
        Z.decompress(payload[:-1], DEV)
    many = comp.compress_many([by_name["zeros_70000"], by_name["random_4096"], data], keep_bad=True)
    assert many[1] is None and many[2] == payload
    assert Z.decompress_many([Z.Lz4BlockDecompressor(many[0], DEV), Z.Lz4BlockDecompressor(many[2], DEV)], DEV) == \
        [by_name["zeros_70000"], data]


def test_mixed_image_lz4_none_ricepp():
    by_name = dict(LC.encoder_inputs())
    blocks = [by_name["sentence_18000"], by_name["random_4096"], by_name["zeros_70000"], by_name["sandwich"]]
    lz4_part = Z.Lz4BlockCompressor(None, DEV).compress_many_sections(blocks, None, first_number=0)
    hc_part = block_codec.block_compressor("lz4hc", DEV).compress_many_sections([by_name["random_below_4"]], None,
                                                                               first_number=len(blocks))
    rng = np.random.default_rng(5)
    pix = [(rng.poisson(900, 3000).astype(np.uint16) << 1).byteswap().tobytes() for _ in range(2)]
    meta = '{"endianness":"big","bytes_per_sample":2,"unused_lsb_count":1,"component_count":1}'
    rpp_part = block_codec.compress_many_sections(pix, meta, first_number=len(blocks) + 1)
    image = lz4_part + hc_part + rpp_part
    secs, bad = S.walk(image)
    assert bad is None
    assert [(h.number, h.compression) for _, h in secs] == [(0, 3), (1, 0), (2, 3), (3, 3), (4, 4), (5, 7), (6, 7)]
    assert all(h.type == S.SECTION_TYPE_BLOCK for _, h in secs)
    assert secs[1][1].length == 4096  # the NONE section: the raw bytes, no frame
    want = blocks + [by_name["random_below_4"]] + pix
    for verify in (0, 1, 2):
        assert block_codec.decompress_sections(image, verify=verify, device=DEV) == want
    for at, h in (secs[0], secs[1], secs[4]):  # a flipped payload byte in an LZ4, a NONE and an LZ4HC section
        broken = bytearray(image)
        broken[at + S.HEADER_BYTES + int(h.length) // 2] ^= 0x40
        with pytest.raises(RuntimeError, match=S.INTEGRITY_ERROR):
            block_codec.decompress_sections(bytes(broken), verify=2, device=DEV)
