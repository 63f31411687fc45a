"""GPU tests of the Zstandard kernels on constructed frames (tests/zstd_build.py): every family is one
rpp_zstd_decode_batch over all its frames, packed at odd input phases and odd output strides with guard bytes
between the outputs.  Statuses and bytes are compared with the builder's records only: the expected bytes come
from the builder's executor of the sequence lists, checked on the CPU against tests/zstd_ref.py and libzstd by
tests/test_zstd_constructed_host.py; nothing here is compared with the GPU's own output or with the host
restatement."""

import time

import pytest

import zstd_build as B
from dwarfs_amd import _native as N
from test_gpu_zstd import FILL, gpu_decode

pytestmark = pytest.mark.gpu
assert FILL == B.FILL


def check(cases, phase=1, spare=0):
    t0 = time.perf_counter()
    st, outs, intact = gpu_decode([c.frame for c in cases], [c.out_n for c in cases],
                                  max_blocks=sum(c.blocks for c in cases) + spare, phase=phase)
    print(f"{len(cases)} frames, {sum(c.out_n for c in cases)} output bytes, launch and copies "
          f"{time.perf_counter() - t0:.3f} s")
    wrong = [c.what for c, s in zip(cases, st) if s != (N.RPP_OK if c.ok else N.RPP_CORRUPT_INPUT)]
    assert not wrong, (len(wrong), wrong[:8])
    # a refused frame leaves what the blocks before the failing one produced
    wrong = [c.what for c, got in zip(cases, outs) if got[:len(c.want)] != c.want]
    assert not wrong, (len(wrong), wrong[:8])
    assert intact
    return st


def test_decode_overlap():
    """execute's pattern copy: offsets 1..130 and around 192 and 256, match lengths around every multiple of
    64 up to 193 and 300, patterns of distinct bytes, the destination at each misalignment."""
    check(B.overlap())


def test_decode_apart():
    """wave_copy's 256-byte turns and its byte tail for literal runs, matches and trailing literals of 255..1023
    bytes, the match's source 0, 1 and 3 bytes clear of its destination."""
    check(B.apart())


def test_decode_batches_of_64():
    """Blocks of 1, 63, 64, 65, 127, 128, 129 and 200 sequences, dealt to the wave 64 at a time, with repeat
    codes without literals on both sides of a group's edge."""
    check(B.batches_of_64())


def test_decode_watermark():
    """Chains of matches whose sources end exactly at the store watermark (no wait), one byte past it, straddle
    it, lie in the literals the same sequence just stored, in the sequence before, in the previous match's
    output, or in the last bytes of a Raw or RLE block right before: several hundred chains in one launch, so
    that many waves share a CU.  This pins the bytes at the rule's edges and makes a stale read possible to
    observe (the literals avoid the buffer's fill byte); it cannot make one certain, and whether a missing wait
    is observable on this hardware has not been measured."""
    check(B.watermark())


def test_decode_repeat_offsets():
    """All six repeat-offset cases, the history carried across Raw, RLE and zero-sequence blocks, the initial
    history 1, 4, 8, and "repeat offset 1 minus 1" refused where it is 0."""
    st = check(B.repeat_offsets())
    assert list(st).count(N.RPP_CORRUPT_INPUT) == 2


def test_decode_chains():
    """Which earlier block supplies a Treeless tree and each Repeat table: suppliers one, two and five blocks
    back with every kind of block in between, each table from another block, Repeat of a Repeat, of an RLE and
    of a Predefined table, suppliers whose table lies behind other descriptions; refused where nothing came
    before."""
    check(B.chains())


def test_decode_isolation():
    """A frame that opens with Treeless or Repeat is refused although the frame before it in the batch left a
    tree and tables; its valid neighbours decode as if alone.  A frame cut in a block header and frames with a
    byte too many or too few behind their last block are refused with the sound blocks' bytes written."""
    check(B.isolation())


def test_decode_cut_frame_ahead_of_valid_frames():
    """A frame of two Raw blocks and a cut third header, which is promised one block as every frame whose
    headers cannot be walked, ahead of all the valid frames of the family, and exactly the blocks promised: the
    two blocks walked take no valid frame's slot, so every valid frame decodes; the one slot left does not hold
    them, and nothing outside the outputs is written.  With one more slot they are written too."""
    cut, valid = B.isolation()[0], [c for c in B.isolation() if c.ok]
    assert (cut.ok, cut.blocks, len(cut.want)) == (False, 1, 103) and len(valid) == 7
    batch = [cut] + valid
    st, outs, intact = gpu_decode([c.frame for c in batch], [c.out_n for c in batch],
                                  max_blocks=sum(c.blocks for c in batch), phase=2)
    assert intact
    assert list(st) == [N.RPP_CORRUPT_INPUT] + [N.RPP_OK] * len(valid)
    assert [c.what for c, got in zip(valid, outs[1:]) if got != c.want] == []
    check(batch, phase=2, spare=1)


@pytest.mark.parametrize("blocks", B.ISOLATION_BATCHES)
def test_decode_isolation_batch_shape(blocks):
    """The same valid frames in batches of 1, 2, 3, 4, 5 and 9 blocks: an entropy workgroup's four waves hold
    blocks of different frames, Raw and RLE blocks and blocks without Huffman literals beside Huffman ones."""
    check(B.isolation_batch(blocks), phase=blocks)


def test_decode_literals():
    """Every literals type in every size format, four streams with 0, 1 and 2 literals in the last one, streams
    of 1..17 bytes (both refill paths), the last code 1 bit under an 11-bit table, and trees of 2, 129 and 256
    symbols and of depth 11; depth 12 is refused."""
    check(B.literals())


def test_decode_sequences():
    """All tables RLE with up to 32513 sequences (the 3-byte count), FSE tables at accuracy logs 5 and 9/8/9 in
    every mix of modes, the widest sequence the format holds, offset code 31 and a sequence one byte over the
    block maximum refused."""
    check(B.sequences())


def test_decode_window_and_size():
    """Offsets at the window and at the output's start and one past them, blocks at the block maximum and one
    over, every store path offered one byte too few, the exact size and one too many, every frame header."""
    st = check(B.window_and_size())
    assert {int(s) for s in st} == {N.RPP_OK, N.RPP_CORRUPT_INPUT}
