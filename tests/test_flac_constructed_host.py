"""The constructed FLAC cases (flac_cases.py, written field by field by flac_build.py) on the CPU.

Every valid case decodes to the writer's samples under the independent RFC 9639 reader (flac_ref.py) and under
the CPU restatement (oracle/flac_oracle.c); every refused case is refused by both.  The geometry each case
claims -- a code on a 32-bit segment boundary, a unary run of 2049 bits at the last bit of lane 63's segment,
a partition that ends at a lane's exit -- is asserted here from the bit positions the writer recorded, through a
model of the wave decoder's window (flac_cases.wave_model): a kernel change that moves a constant makes these
assertions fail instead of leaving the case vacuous.  test_gpu_flac_constructed.py runs the same list on the GPU.
"""

from pathlib import Path

import numpy as np
import pytest

import flac_build as B
import flac_cases as K
import flac_ref as R
from oracle import flac as F

VALID = K.ids(K.CASES)
BAD = K.ids(K.REFUSED)


def as_int32(samples):
    return (np.array(samples, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def test_writer_crcs_are_the_readers():
    rng = np.random.default_rng(2)
    for n in (0, 1, 7, 300):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert B.crc8(b) == R.crc8(b) and B.crc16(b) == R.crc16(b)
    assert B.crc8(b"123456789") == 0xF4 and B.crc16(b"123456789") == 0xFEE8


def test_writer_refuses_what_it_cannot_express():
    for bs, code in ((191, 1), (577, 2), (257, 6), (0, 6), (65537, 7), (300, 8), (16, 0)):
        with pytest.raises(ValueError):
            B.blocksize_field(bs, code)
    assert B.blocksize_field(256, 6) == b"\xff" and B.blocksize_field(65535, 7) == b"\xff\xfe"
    x = [0, -(1 << 31)] + [0] * 14
    with pytest.raises(ValueError, match="9.2.7.3"):
        B.frame(16, [B.fixed(0, x, B.Residual(1, 0, (30,)))], 32, bs_code=6)
    B.frame(16, [B.fixed(0, x, B.Residual(1, 0, (30,)))], 32, bs_code=6, allow_wide=True)
    with pytest.raises(ValueError):   # a side value that needs 18 bits
        B.frame(16, [B.verbatim([0] * 16), B.verbatim([1 << 16] * 16)], 16, bs_code=6, assignment="left_side")
    with pytest.raises(ValueError):
        B.stream(1, 16, [B.frame(b, [B.constant([0] * b)], 16, bs_code=6) for b in (16, 17, 16)])
    assert [len(B.utf8(v)) for v in (127, 128, 2047, 2048, 65535, 65536, (1 << 21) - 1, 1 << 21, 1 << 26, 1 << 31,
                                     (1 << 36) - 1)] == [1, 2, 2, 3, 3, 4, 4, 5, 6, 7, 7]


def test_every_family_is_present():
    assert {c.family for c in K.CASES} == set(K.FAMILIES)
    assert len(K.REFUSED) >= 17
    assert (K.SEG_BITS, K.LANES, K.FWIN, K.FLOOK) == (32, 64, 512, 64)
    # the constants the cases aim at are still the kernel's
    src = (Path(__file__).resolve().parent.parent / "dwarfs_amd" / "csrc" / "flac_kernels.hip").read_text()
    assert "constexpr uint32_t kFWin = 512;" in src and "constexpr uint32_t kFLook = 64;" in src
    assert "constexpr uint32_t kWave = 64;" in src and "const uint64_t ss = ((pos >> 5) + lane) << 5;" in src
    assert "constexpr uint32_t kFlacWaveLds = 144 * 1024;" in src


@pytest.mark.parametrize("name,bits", VALID)
def test_valid_case_on_both_cpu_readers(name, bits):
    c, st = K.BY_NAME[name], K.built(name, bits)
    assert st.bits == bits
    if c.check:
        c.check(st, bits)
    info = R.parse_streaminfo(st.data)
    assert (info.channels, info.bits, info.total_samples, info.frames_at) == (st.channels, bits, st.total, 42)
    if c.wide == "min":
        # a residual of -2^31: the RFC reader enforces section 9.2.7.3; the restatement (and the GPU decoder,
        # test_gpu_flac_constructed.py) still decode the samples, which fit their width
        for reader in (R.walk_frames, R.decode):
            with pytest.raises(R.FlacError, match="9.2.7.3"):
                reader(st.data)
    else:
        frames = R.walk_frames(st.data, info)
        assert [(f.pos, f.length) for f in frames] == st.frames
        assert [f.blocksize for f in frames] == st.blocksizes
        assert all(f.crc8_ok and f.crc16_ok for f in frames)
        assert R.decode(st.data) == st.samples
    status, y, ch, b = F.decode(st.data, len(st.samples))
    assert status == F.OK and (ch, b) == (st.channels, bits)
    assert np.array_equal(y, as_int32(st.samples))
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assert lo <= min(st.samples) and max(st.samples) <= hi


def test_the_widest_residuals_on_the_cpu_readers():
    """Family h under allow_wide: a residual of -2^31 (which RFC 9639 section 9.2.7.3 excludes: the range is
    that of a 32-bit one's complement integer) and one of 2^31.  The RFC reader refuses the first by that
    section and, like the restatement, decodes the second; the restatement enforces neither and decodes the
    samples, which fit their width.  The GPU test requires the same of the codec."""
    wide = [c for c in K.CASES if c.wide]
    assert sorted(c.wide for c in wide) == ["min", "min", "ok", "ok"]
    assert {c.name for c in wide if c.wide == "min"} == {"h_res_min_32", "h_res_min_16"}
    for c in wide:
        for bits in c.widths:
            st = K.built(c.name, bits)
            sub = st.marks[0][1]
            assert sub.params == [("rice", 30 if bits == 32 else 28)]
            assert F.decode(st.data, len(st.samples))[0] == F.OK
            if c.wide == "min":
                with pytest.raises(R.FlacError, match="9.2.7.3"):
                    R.decode(st.data)
            else:
                assert R.decode(st.data) == st.samples


@pytest.mark.parametrize("name,bits", BAD)
def test_refused_case_on_both_cpu_readers(name, bits):
    st = K.built_refused(name, bits)
    assert len(st.frames) == 3
    # the frames around the bad one are valid, and every CRC-8 and CRC-16 is right: only the parser can refuse
    for i, (pos, n) in enumerate(st.frames):
        h = R.parse_header(st.data, pos)
        assert h.crc8_ok and h.coded == i
        assert R.crc16(st.data[pos:pos + n - 2]) == int.from_bytes(st.data[pos + n - 2:pos + n], "big")
        if i != 1:
            f = R.frame_at(st.data, pos, st.channels, bits)
            assert f.length == n and f.crc16_ok
    if name == "last_code_ends_in_the_crc16":
        pos, n = st.frames[1]
        assert st.data[pos + n - 2:pos + n] != b"\0\0"
    if name == "unary_run_reaches_the_frame_end":
        pos, n = st.frames[1]
        assert st.data[pos + n - 2:pos + n] == b"\0\0" and st.data[pos + n] == 0xFF
    with pytest.raises(R.FlacError):
        R.decode(st.data)
    assert F.decode(st.data, len(st.samples))[0] != F.OK
