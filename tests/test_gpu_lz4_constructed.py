"""GPU tests of the LZ4 kernels on constructed blocks (tests/lz4_build.py): every family is one
rpp_lz4_decode_batch over all its blocks, packed at odd input offsets and odd output strides with guard bytes
between the outputs, and the inputs aimed at the encoder are one rpp_lz4_encode_batch.  The expected bytes come
from the sequence lists, checked on the CPU against tests/lz4_ref.py and liblz4 by
tests/test_lz4_constructed_host.py; nothing here is compared with the GPU's own output or, for decode, with the
host restatement."""

import time

import numpy as np
import pytest
import torch

import lz4_build as B
import lz4_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import lz4 as Z
from test_gpu_lz4 import DEV, FILL, GUARD, gpu_encode, pack_odd

pytestmark = pytest.mark.gpu
assert FILL == B.FILL


def gpu_decode(cases):
    """One rpp_lz4_decode_batch over the cases: (statuses, output regions, True if every byte outside the
    regions is untouched).  Outputs lie GUARD + 1 bytes apart (odd strides), or at the misalignment mod 4 a
    case asks for."""
    d_in, in_offs = pack_odd([c.block for c in cases])
    out_offs, at = [], GUARD
    for c in cases:
        if c.out_mis is not None:
            at += (c.out_mis - at) % 4
        out_offs.append(at)
        at += c.out_n + GUARD + 1
    out = torch.full((at,), FILL, dtype=torch.uint8, device=DEV)
    assert out.data_ptr() % 4 == 0
    sizes = [c.out_n for c in cases]
    _, _, st = Z.decode_batch(d_in, in_offs, [len(c.block) for c in cases], sizes, out=out, out_offsets=out_offs)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    mask = np.ones(at, bool)
    for o, n in zip(out_offs, sizes):
        mask[o:o + n] = False
    return st.cpu().numpy(), [host[o:o + n].tobytes() for o, n in zip(out_offs, sizes)], bool((host[mask] == FILL).all())


def check(cases):
    t0 = time.perf_counter()
    st, outs, intact = gpu_decode(cases)
    print(f"{len(cases)} blocks, {sum(c.out_n for c in cases)} output bytes, launch and copies "
          f"{time.perf_counter() - t0:.3f} s")
    wrong = [c.what for c, s in zip(cases, st) if s != (N.RPP_OK if c.ok else N.RPP_CORRUPT_INPUT)]
    assert not wrong, (len(wrong), wrong[:8])
    # a refused block leaves what the sequences before the refusal stored, and the fill behind it
    wrong = [c.what for c, got in zip(cases, outs) if got != c.want + bytes([FILL]) * (c.out_n - len(c.want))]
    assert not wrong, (len(wrong), wrong[:8])
    assert intact
    return st


def test_decode_overlap():
    """Offsets 1..130 and around 192 and 256, match lengths around every multiple of 64 up to 193 and 300,
    the destination at each misalignment: the overlapped copy's wrap, with patterns of distinct bytes."""
    check(B.overlap())


def test_decode_apart():
    """The wide copy's 256-byte turns and its byte tail for a match: lengths around 256, 512 and 1023, the
    source 0, 1 and 3 bytes before the destination, all 16 misalignments of the two over the family."""
    check(B.apart())


def test_decode_literals():
    """Literal runs of 0..515 bytes starting at every byte of the 64-byte window: stored from the window up
    to its last byte, by the wide copy beyond."""
    check(B.literals())


def test_decode_window_edges():
    """Tokens at bytes 62..65, length extensions of 1..130 bytes of 255 across one and two reloads of the
    window, for literal and for match lengths, and an offset whose two bytes lie on either side of a reload."""
    check(B.window_edges())


def test_decode_watermark():
    """Chains of matches whose sources end exactly at the watermark (no wait), one byte past it, straddle it,
    lie in what the sequence before stored, or copy the output of the match before: 1248 chains in one launch,
    so that many waves share a CU.  This pins the bytes at the rule's edges and makes a stale read possible to
    observe (the literals avoid the buffer's fill byte); it cannot make one certain, and whether a missing
    wait is observable on this hardware has not been measured."""
    check(B.watermark())


def test_decode_output_size():
    """Blocks offered one byte too few, the exact size and one too many on each store path: RPP_OK only when
    exact, the bytes stored before the refusal and nothing else, the guards intact.  And no input at all, a
    lone 0x00 token, and an offset that reaches the output's first byte or one before it."""
    st = check(B.output_size())
    assert {int(s) for s in st} == {N.RPP_OK, N.RPP_CORRUPT_INPUT}


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5, 9])
def test_decode_batch_shape(batch):
    """The same nine blocks in batches that fill a workgroup's four waves, and that leave 1, 2 and 3 over."""
    check(B.batch_shape()[:batch])


def test_encode_aimed_inputs():
    """The inputs of lz4_build.encoder_inputs in one rpp_lz4_encode_batch: the GPU's blocks equal the host
    encoder's, the independent reader gets the inputs back from them, they keep the end rules, the ratio flag
    is 4 + len(block) >= n, and the GPU decodes them."""
    names, inputs = zip(*B.encoder_inputs(N.lib().rpp_lz4_chunk_bytes(), N.lib().rpp_lz4_step_positions()))
    t0 = time.perf_counter()
    streams, flags, res = gpu_encode(inputs)
    print(f"{len(inputs)} inputs, {sum(map(len, inputs))} bytes, launch and copies {time.perf_counter() - t0:.3f} s")
    for name, data, s, f in zip(names, inputs, streams, flags):
        assert s == Z.host_encode(data)[0], name
        assert R.decode(s, len(data)) == data, name
        R.check_end_rules(s, len(data))
        assert bool(f) == (4 + len(s) >= len(data)), name
    out, offs, st = Z.decode_batch(res.data, res.offsets, res.sizes, [len(b) for b in inputs])
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == N.RPP_OK).all()
    host_out = out.cpu().numpy()
    for name, o, b in zip(names, offs, inputs):
        assert host_out[o:o + len(b)].tobytes() == b, name
