"""FLAC conformance, CPU side.

Decode is pinned to libFLAC 1.3.3 by the three example streams of RFC 9639
Appendix D (tests/golden/flac_rfc9639.json): each stream's STREAMINFO carries
the MD5 libFLAC took over the PCM it encoded, and a decoder whose samples hash
to it agrees with libFLAC on that stream.  The encoders are pinned to the
format by an independent reader written from the RFC (tests/flac_ref.py).
Neither encoder is pinned bit-for-bit to libFLAC's encoder choices (model
search, apodization): that remains unpinned.

This module also builds the phantom-sync streams of test_gpu_flac_conformance.py
(frame headers, and whole frames, spelled by the samples of a verbatim
subframe) and checks them on the CPU: serial decoders are unaffected by them.
"""

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import flac_ref as R
from oracle import flac as F
from test_flac import OPTS

FIXTURES = json.loads((Path(__file__).resolve().parent / "golden" / "flac_rfc9639.json").read_text())
FIX_IDS = [fx["name"] for fx in FIXTURES]


def fixture_stream(fx) -> bytes:
    return bytes.fromhex(fx["stream_hex"])


def test_crc_check_values():
    """The published check values of CRC-8 (poly 0x07) and CRC-16/UMTS (poly 0x8005), both MSB first from 0."""
    assert R.crc8(b"123456789") == 0xF4
    assert R.crc16(b"123456789") == 0xFEE8
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 255, 1000):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert R.crc16_fast(b) == R.crc16(b)


@pytest.mark.parametrize("fx", FIXTURES, ids=FIX_IDS)
def test_fixture_self_check(fx):
    """The fixture is consistent by hashlib and bitwise CRCs alone: the frames' CRC-8 and CRC-16 are the RFC's
    and match a from-scratch CRC, the walker accepts the stream, and md5(pack(samples)) is STREAMINFO's MD5."""
    s = fixture_stream(fx)
    info = R.parse_streaminfo(s)
    assert (info.channels, info.bits) == (fx["channels"], fx["bits"])
    assert info.total_samples * info.channels == len(fx["samples"])
    assert [list(b) for b in info.blocks] == fx["metadata_blocks"]
    assert info.md5.hex() == fx["md5"]
    assert hashlib.md5(R.pcm_le(fx["samples"], fx["bits"])).hexdigest() == fx["md5"]
    frames = R.walk_frames(s, info)
    assert [f.blocksize for f in frames] == fx["blocksizes"]
    assert frames[-1].pos + frames[-1].length == len(s)
    for f, c8, c16 in zip(frames, fx["crc8"], fx["crc16"], strict=True):
        h = R.parse_header(s, f.pos)
        assert f.crc8_ok and f.crc16_ok
        assert s[f.pos + h.length - 1] == int(c8, 16) == R.crc8(s[f.pos:f.pos + h.length - 1])
        assert s[f.pos + f.length - 2:f.pos + f.length].hex() == c16
        assert R.crc16(s[f.pos:f.pos + f.length - 2]) == int(c16, 16)


@pytest.mark.parametrize("fx", FIXTURES, ids=FIX_IDS)
def test_libflac_streams_decode(fx):
    """libFLAC's streams through the independent reader and the CPU restatement: the fixture's samples, whose MD5
    is libFLAC's own; any single flipped bit of a frame's CRC-8 or CRC-16 is an error in the restatement."""
    s = fixture_stream(fx)
    assert R.decode(s) == fx["samples"]
    st, y, ch, bits = F.decode(s, len(fx["samples"]))
    assert st == F.OK and (ch, bits) == (fx["channels"], fx["bits"])
    assert y.tolist() == fx["samples"]
    assert hashlib.md5(R.pcm_le(y.tolist(), bits)).hexdigest() == fx["md5"]
    for f in R.walk_frames(s):
        h = R.parse_header(s, f.pos)
        for at in (f.pos + h.length - 1, f.pos + f.length - 2, f.pos + f.length - 1):
            for bit in range(8):
                bad = bytearray(s)
                bad[at] ^= 1 << bit
                assert F.decode(bytes(bad), len(fx["samples"]))[0] != F.OK, (at, bit)
                with pytest.raises(R.FlacError):
                    R.decode(bytes(bad))


def signal(channels, n, bits, seed):
    """Two tones per channel with a little noise and full-scale outliers, interleaved int32."""
    rng = np.random.default_rng(seed)
    lim = 1 << (bits - 1)
    t = np.arange(n)[:, None]
    x = 0.4 * lim * np.sin(t * (0.05 + 0.013 * np.arange(channels))) + 0.1 * lim * np.sin(t * 0.31)
    x = np.rint(x).astype(np.int64) + rng.integers(-3, 4, (n, channels))
    x[::37] = rng.integers(-lim, lim, x[::37].shape)
    return np.clip(x, -lim, lim - 1).reshape(-1).astype(np.int32)


ENC_OPTS = dict(OPTS, **{f"stereo{s}": F.EncodeOptions(stereo=s) for s in (0, 8, 9, 10)})


@pytest.mark.parametrize("name", sorted(ENC_OPTS))
@pytest.mark.parametrize("channels,bits", [(1, 16), (2, 16), (2, 24), (3, 8), (2, 32)])
def test_independent_reader_decodes_the_oracle_encoder(name, channels, bits):
    """Every option of the restatement's encoder (test_flac.OPTS and each stereo setting) read by the independent
    decoder: the input back exactly, and no rule of the walker broken."""
    x = signal(channels, 300, bits, len(name) + channels + bits)
    for blocksize in (16, 200, 4096):
        s = F.encode(x, channels, bits, blocksize, ENC_OPTS[name])
        frames = R.walk_frames(s)
        assert all(f.crc8_ok and f.crc16_ok for f in frames), (name, blocksize)
        assert sum(f.blocksize for f in frames) == 300
        assert R.decode(s) == x.tolist(), (name, blocksize)


def many_small_frames():
    """16 * 2050 + 3 mono 8-bit samples for block size 16: frame numbers cross 127 -> 128 (two UTF-8 bytes) and
    2047 -> 2048 (three)."""
    n = 16 * 2050 + 3
    rng = np.random.default_rng(7)
    x = np.rint(90 * np.sin(np.arange(n) * 0.02)).astype(np.int64) + rng.integers(-9, 10, n)
    return np.clip(x, -128, 127).astype(np.int32)


def test_frame_numbers_cross_the_utf8_lengths():
    x = many_small_frames()
    s = F.encode(x, 1, 8, 16)
    frames = R.walk_frames(s)
    assert len(frames) == 2051 and frames[-1].coded == 2050 and frames[-1].blocksize == 3
    assert all(f.crc8_ok and f.crc16_ok for f in frames)
    lengths = {k: R.parse_header(s, frames[k].pos).length for k in (127, 128, 2047, 2048)}
    assert lengths[128] == lengths[127] + 1 and lengths[2048] == lengths[2047] + 1
    st, y, _, _ = F.decode(s, x.size)
    assert st == F.OK and np.array_equal(y, x)
    assert R.decode(s) == x.tolist()


def test_walker_rejects_rule_breaks():
    """Each rule of the walker fires: the checks of the GPU encoder's streams are not vacuous."""
    x = signal(2, 40, 16, 3)
    s = bytearray(F.encode(x, 2, 16, 16))
    info = R.parse_streaminfo(bytes(s))
    frames = R.walk_frames(bytes(s))
    p1 = frames[1].pos

    def refix(buf, p):  # recompute the CRC-8 of the header at p
        n = R.parse_header(bytes(buf), p).length
        buf[p + n - 1] = R.crc8(bytes(buf[p:p + n - 1]))

    for what, edit in [("reserved bit after sync", lambda b: b.__setitem__(p1 + 1, b[p1 + 1] | 2)),
                       ("reserved bit after size", lambda b: b.__setitem__(p1 + 3, b[p1 + 3] | 1)),
                       ("block size code 0", lambda b: b.__setitem__(p1 + 2, b[p1 + 2] & 0x0F)),
                       ("sample rate code 15", lambda b: b.__setitem__(p1 + 2, b[p1 + 2] | 0x0F)),
                       ("sample size code 3", lambda b: b.__setitem__(p1 + 3, (b[p1 + 3] & 0xF1) | 6)),
                       ("sample size 24", lambda b: b.__setitem__(p1 + 3, (b[p1 + 3] & 0xF1) | 12)),
                       ("three channels", lambda b: b.__setitem__(p1 + 3, (b[p1 + 3] & 0x0F) | 0x20)),
                       ("assignment 11", lambda b: b.__setitem__(p1 + 3, (b[p1 + 3] & 0x0F) | 0xB0)),
                       ("frame number", lambda b: b.__setitem__(p1 + 4, 5))]:
        bad = bytearray(s)
        edit(bad)
        with pytest.raises(R.FlacError):
            R.walk_frames(bytes(bad))
    # block sizes against STREAMINFO: maximum 8 (< 16), then minimum 32 with short frames before the last
    for at, value in ((10, 8), (8, 32)):
        bad = bytearray(s)
        bad[at:at + 2] = value.to_bytes(2, "big")
        if at == 8:
            bad[10:12] = (32).to_bytes(2, "big")
        with pytest.raises(R.FlacError):
            R.walk_frames(bytes(bad))
    # variable blocking: sample numbers must continue
    v = bytearray(F.encode(x, 2, 16, 16, F.EncodeOptions(variable_blocking=True)))
    fv = R.walk_frames(bytes(v))
    assert [f.coded for f in fv] == [0, 16, 32]
    v[fv[1].pos + 4] = 17
    refix(v, fv[1].pos)
    with pytest.raises(R.FlacError, match="starts at sample"):
        R.walk_frames(bytes(v))
    assert info.frames_at == 42


# ---- phantom syncs: streams whose verbatim samples spell frame headers and frames ----

BS = 4096
N_PHANTOM = 2 * BS + 100  # three frames: 4096, 4096, 100
VERBATIM = F.EncodeOptions(subframe_type="verbatim", wasted=False, stereo=0)


def header_bytes(number: int, channels: int = 1, rate_code: int = 10, bs_code: int = 12, extra: bytes = b"") -> bytes:
    """A frame header of a 16-bit stream with a good CRC-8: block size code (12: 4096; 6: ``extra`` + 1), frame
    number below 128."""
    h = bytes([0xFF, 0xF8, (bs_code << 4) | rate_code, ((channels - 1) << 4) | (4 << 1), number]) + extra
    return h + bytes([R.crc8(h)])


def frames_of(stream: bytes):
    """The frames of an oracle stream, as bytes."""
    return [stream[f.pos:f.pos + f.length] for f in R.walk_frames(stream)]


class Phantom:
    """A verbatim stream built from per-channel payload bytes (big-endian 16-bit samples, three frames)."""

    def __init__(self, channels: int = 1, seed: int = 0):
        rng = np.random.default_rng(seed)
        self.channels = channels
        # (no 0xFF byte: the only sync codes are the true frames' and the planted ones)
        self.payload = rng.integers(0, 255, (channels, 2 * N_PHANTOM), dtype=np.uint8)
        self.planted = 0

    def plant(self, frame: int, offset: int, data: bytes, channel: int = 0, count: int = 1):
        """``data`` at byte ``offset`` of frame ``frame``'s subframe ``channel``."""
        at = 2 * BS * frame + offset
        assert offset >= 0 and offset + len(data) <= 2 * min(BS, N_PHANTOM - BS * frame)
        self.payload[channel, at:at + len(data)] = np.frombuffer(data, np.uint8)
        self.planted += count

    def samples(self) -> np.ndarray:
        x = self.payload.view(">i2").astype(np.int32)  # [channels][n]
        return np.ascontiguousarray(x.T).reshape(-1)

    def stream(self) -> bytes:
        s = F.encode(self.samples(), self.channels, 16, BS, VERBATIM)
        body = s[42:]
        # the payload is in the stream as built: 6-byte headers, one byte per subframe, the samples
        at = 0
        for f in range(3):
            n = 2 * min(BS, N_PHANTOM - BS * f)
            at += 6 if f < 2 else 7
            for c in range(self.channels):
                assert body[at] == 0x02
                assert body[at + 1:at + 1 + n] == self.payload[c, 2 * BS * f:2 * BS * f + n].tobytes()
                at += 1 + n
            at += 2
        assert at == len(body)
        return s

    def pcm(self) -> bytes:
        """The samples as little-endian signed 16-bit PCM."""
        return self.samples().astype("<i2").tobytes()


def small_frame(channels: int, number: int, seed: int = 11) -> bytes:
    """A complete valid frame of 16 samples with frame number ``number``, both CRCs good (the oracle's encoder)."""
    x = signal(channels, 16 * (number + 1), 16, seed)
    return frames_of(F.encode(x, channels, 16, 16, F.EncodeOptions(stereo=0)))[number]


def phantom_bad_payload() -> Phantom:
    """Case 1: headers valid for the stream whose frames do not parse (subframe padding bit set) or parse and fail
    the CRC-16 (a verbatim frame of 16 samples over the stream's random bytes)."""
    p = Phantom(seed=1)
    p.plant(1, 1000, header_bytes(1) + b"\x80")
    p.plant(1, 3001, header_bytes(1, bs_code=6, extra=b"\x0f") + b"\x02")
    p.plant(0, 5000, header_bytes(0, rate_code=9) + b"\x02")
    return p


def phantom_whole_frame(channels: int = 1) -> Phantom:
    """Case 2: a complete valid frame (number 0, 16 samples) in the middle of frame 1 -- of its second subframe for
    stereo; the byte after it starts no header."""
    p = Phantom(channels, seed=2)
    p.plant(1, 4001, small_frame(channels, 0), channel=channels - 1)
    return p


def solve_free_sample(frame: bytearray, at: int, want: int) -> int:
    """The 16-bit value at frame[at:at+2] for which crc16(frame) == want.  The CRC is linear over GF(2), so the
    effect of each of the sample's bits is found once; the search then runs over the 2^16 values."""
    tail = len(frame) - at - 2
    frame[at:at + 2] = b"\0\0"
    delta = want ^ R.crc16_fast(bytes(frame))
    basis = [R.crc16_fast((1 << i).to_bytes(2, "big") + bytes(tail)) for i in range(16)]
    for v in range(1 << 16):
        d = 0
        for i in range(16):
            if (v >> i) & 1:
                d ^= basis[i]
        if d == delta:
            return v
    raise AssertionError("no value gives the CRC-16")


def phantom_shared_crc(linking: bool) -> Phantom:
    """Case 3: a complete valid phantom whose last byte is the last payload byte of true frame 1 and whose CRC-16 is
    frame 1's own (one earlier sample of frame 1 is chosen so that the two agree), so the phantom ends exactly where
    true frame 2 starts.

    linking=False: frame number 2, block size 16.  A decoder that places frames by their coded number puts it at
    sample 2 * 4096, where true frame 2 is: it overlaps the chain instead of continuing it.
    linking=True: frame number 1, block size 4096, one constant subframe.  Its coded number puts it at sample 4096
    and true frame 2 right after it, so its link to true frame 2 holds; every link of every valid candidate holds,
    and only the sum of the block sizes (3 * 4096 + 100, not the stream's 2 * 4096 + 100) and the serial walk
    tell it from true frame 1."""
    p = Phantom(seed=3 + linking)
    if linking:
        x = np.full(2 * BS, -12345, np.int32)
        ph = frames_of(F.encode(x, 1, 16, BS, F.EncodeOptions(subframe_type="constant", wasted=False)))[1]
        assert len(ph) == 6 + 3 + 2
    else:
        ph = small_frame(1, 2)
    body, crc = ph[:-2], int.from_bytes(ph[-2:], "big")
    p.plant(1, 2 * BS - len(body), body)
    free = (2 * BS - len(body)) // 2 - 1  # a sample of frame 1 before the phantom
    frame1 = bytearray(header_bytes(1) + b"\x02" + p.payload[0, 2 * BS:4 * BS].tobytes())
    v = solve_free_sample(frame1, 7 + 2 * free, crc)
    p.plant(1, 2 * free, v.to_bytes(2, "big"), count=0)
    return p


def phantom_many_headers(count: int = 1200) -> Phantom:
    """Case 4: ``count`` distinct valid headers in the payload of frames 0 and 1 (128 frame numbers x the
    sample-rate codes that add no bytes), far more than the decoder's first candidate table holds
    (8292 / 4096 + 65 = 67): which candidates that table keeps is a race, and among some 1200 the three true
    frames do not all win it."""
    p = Phantom(seed=5)
    for k in range(count):
        p.plant(k % 2, 40 + 12 * (k // 2), header_bytes(k % 128, rate_code=k // 128))
    return p


PHANTOMS = {
    "bad_payload": phantom_bad_payload,
    "whole_frame": phantom_whole_frame,
    "whole_frame_stereo": lambda: phantom_whole_frame(2),
    "shared_crc_number2": lambda: phantom_shared_crc(False),
    "shared_crc_linking": lambda: phantom_shared_crc(True),
    "many_headers": phantom_many_headers,
}
_built = {}


def phantom_case(name):
    """(Phantom, stream), built once and shared."""
    if name not in _built:
        p = PHANTOMS[name]()
        _built[name] = (p, p.stream())
    return _built[name]


@pytest.mark.parametrize("name", sorted(PHANTOMS))
def test_phantom_streams_on_the_cpu(name):
    """The planted phantoms exist (the header count of the scan rule is the true frames plus at least the planted
    ones), and serial decoders -- the restatement and the independent reader -- return the samples."""
    p, s = phantom_case(name)
    body = s[42:]
    found = R.count_header_candidates(body, p.channels, 16, BS)
    assert found >= 3 + p.planted
    if name == "many_headers":
        heads = {body[q:q + R.parse_header(body, q).length] for q in R.header_candidates(body, 1, 16, BS)}
        assert p.planted >= 200 and len(heads) >= 200 + 3  # (distinct headers)
    x = p.samples()
    st, y, _, _ = F.decode(s, x.size)
    assert st == F.OK and np.array_equal(y, x)
    assert R.decode(s) == x.tolist()
    if name.startswith(("whole_frame", "shared_crc")):
        # the phantom is a whole frame: header, subframes, both CRCs
        frames = R.walk_frames(s)
        whole = []
        for q in R.header_candidates(body, p.channels, 16, BS):
            if q + 42 not in {f.pos for f in frames}:
                try:
                    f = R.frame_at(body, q, p.channels, 16)
                except R.FlacError:
                    continue
                if f.crc8_ok and f.crc16_ok:
                    whole.append(f)
        assert len(whole) == 1
        if name.startswith("shared_crc"):
            assert 42 + whole[0].pos + whole[0].length == frames[2].pos
            assert (whole[0].coded, whole[0].blocksize) == ((1, BS) if name.endswith("linking") else (2, 16))
