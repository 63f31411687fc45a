"""The constructed FLAC cases (flac_cases.py) on the GPU decoder.

The streams are written field by field (flac_build.py), so a code starts, a partition ends and a unary run lies
exactly where the case says; test_flac_constructed_host.py proves that geometry from the writer's recorded bit
positions and checks every case against two CPU readers.  Here each valid case is decoded as a block
(FL.decompress), by one direct rpp_flac_decode call, and in one batch with every other case, 16-bit blocks (the
wave decoder, and the lane decoder's int32 instance for what the wave decoder hands on) beside 32-bit ones (the
lane decoder's int64 instance) in the same launches; each refused case must end in the FLAC error and no samples.

Every comparison is for equality.
"""

import numpy as np
import pytest

import flac_cases as K
import flac_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import flac as FL
from dwarfs_amd.pcm import PcmSampleEndianness as E, PcmSamplePadding as Pd, PcmSampleSignedness as S
from test_gpu_flac import pcm_bytes
from test_gpu_flac_conformance import direct_decode, le_block

pytestmark = pytest.mark.gpu

VALID = K.ids(K.CASES)
BAD = K.ids(K.REFUSED)
_pcm = {}


def as_int32(samples):
    return (np.array(samples, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def pcm_le(name, bits) -> bytes:
    """The writer's samples as the block's PCM: little-endian signed, ceil(bits / 8) bytes a sample."""
    if (name, bits) not in _pcm:
        st = K.built(name, bits)
        if bits in (8, 16, 32):
            _pcm[name, bits] = np.array(st.samples, dtype=np.int64).astype(f"<i{bits // 8}").tobytes()
        elif bits == 24:
            _pcm[name, bits] = R.pcm_le(st.samples, bits)
        else:   # 12 and 20 bits: the package's own packing of padded samples (test_pcm.py covers it)
            _pcm[name, bits] = pcm_bytes(as_int32(st.samples), E.Little, S.Signed, Pd.Msb, (bits + 7) // 8, bits)
    return _pcm[name, bits]


def block_of(st) -> bytes:
    return le_block(st.data, len(st.samples), st.channels, st.bits)


@pytest.mark.parametrize("name,bits", VALID)
def test_valid_case(name, bits):
    c, st = K.BY_NAME[name], K.built(name, bits)
    status, found, y = direct_decode(st.body, st.channels, bits, st.max_blocksize, st.total, len(st.frames) + 64)
    assert status == N.RPP_OK and found >= len(st.frames)
    assert np.array_equal(y, as_int32(st.samples))
    if c.direct_only:
        # blocks of 16 to 600 samples in one stream: the block decompressor sizes its workspace from
        # STREAMINFO's range and refuses one this wide; the p_frame_lengths_* cases carry the same frames to it
        with pytest.raises(RuntimeError, match="too wide"):
            FL.decompress(block_of(st))
        return
    assert FL.decompress(block_of(st)) == pcm_le(name, bits)


def test_all_valid_cases_in_one_batch():
    """Every case of every width in one decompress_many: the wave decoder and both instances of the lane
    decoder share the launches.  The result of each block is the one it has alone (test_valid_case)."""
    todo = [(c.name, b) for c in K.CASES if not c.direct_only for b in c.widths]
    assert {b for _, b in todo} >= {8, 16, 24, 32}
    out = FL.decompress_many([block_of(K.built(n, b)) for n, b in todo])
    wrong = [(n, b) for (n, b), pcm in zip(todo, out) if pcm != pcm_le(n, b)]
    assert not wrong


@pytest.mark.parametrize("name,bits", BAD)
def test_refused_case(name, bits):
    st = K.built_refused(name, bits)
    block = block_of(st)
    status, found, y = direct_decode(st.body, st.channels, bits, st.max_blocksize, st.total, len(st.frames) + 64)
    assert status != N.RPP_OK and found >= 2
    with pytest.raises(RuntimeError, match="FLAC"):
        FL.decompress(block)
    good = block_of(K.built("e_bs64_po0_o1", bits))
    with pytest.raises(RuntimeError, match="FLAC"):
        FL.decompress_many([good, block, good])

