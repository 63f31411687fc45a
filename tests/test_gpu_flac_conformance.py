"""FLAC conformance on the GPU (dwarfs_amd.flac over rpp_flac_encode / rpp_flac_decode).

* Decode is pinned to libFLAC 1.3.3: the three example streams of RFC 9639 Appendix D
  (tests/golden/flac_rfc9639.json) decode to PCM whose MD5 is the one libFLAC stored in STREAMINFO.
* The encoder is pinned to the format: an independent reader written from the RFC (tests/flac_ref.py)
  walks every frame the GPU writes against the RFC's field rules and decodes it back to the input.
  It is not pinned bit-for-bit to libFLAC's encoder choices; that remains unpinned.
* Phantom syncs: frame headers, and whole valid frames, spelled by the samples of a verbatim subframe
  (built and checked on the CPU in test_flac_conformance.py).  Only a decoder that looks for frames
  at every byte at once meets them: candidates that must be rejected, the fall-back from the parallel
  link check to the serial walk, and the retry of all three callers when the candidate table overflows.

Every comparison is for equality of samples, bytes, CRCs or MD5 digests.
"""

import ctypes as C
import hashlib
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import flac_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import flac as FL
from dwarfs_amd.pcm import PcmSampleEndianness as E, PcmSamplePadding as Pd, PcmSampleSignedness as S
from oracle import flac as F
from test_flac_conformance import BS, FIX_IDS, FIXTURES, N_PHANTOM, PHANTOMS, fixture_stream, many_small_frames, \
    phantom_case
from test_gpu_flac import ar_audio, meta, pcm_bytes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = Path(__file__).resolve().parent.parent


def le_block(stream: bytes, nvalues: int, channels: int, bits: int) -> bytes:
    """A DwarFS FLAC block around ``stream`` whose PCM is little-endian signed, ceil(bits / 8) bytes a sample."""
    nbytes = (bits + 7) // 8
    return FL.frame_header(nvalues * nbytes, channels, bits, 0x40 | (nbytes - 1)) + stream


def gpu_block(x: np.ndarray, channels: int, bits: int, nbytes: int, level: int = 5):
    """(PCM, block) of interleaved samples through the GPU encoder, little-endian signed PCM."""
    data = pcm_bytes(x, E.Little, S.Signed, Pd.Msb, nbytes, bits)
    return data, FL.FlacBlockCompressor(level).compress(data, meta(E.Little, S.Signed, Pd.Msb, channels, nbytes, bits))


# ---- a. libFLAC's streams ----

def check_fixture_pcm(fx, pcm: bytes):
    assert hashlib.md5(pcm).hexdigest() == fx["md5"]  # libFLAC's own MD5 of the PCM it encoded
    nbytes = (fx["bits"] + 7) // 8
    assert np.frombuffer(pcm, f"<i{nbytes}").tolist() == fx["samples"]


@pytest.mark.parametrize("fx", FIXTURES, ids=FIX_IDS)
def test_libflac_stream_decodes_to_its_md5(fx):
    block = le_block(fixture_stream(fx), len(fx["samples"]), fx["channels"], fx["bits"])
    check_fixture_pcm(fx, FL.decompress(block))


def test_libflac_streams_in_one_batch():
    """All three in one decompress_many with two GPU-encoded blocks, one 32-bit (the lane decoder's int64 instance
    beside the wave decoder in the same launches) and one 16-bit."""
    rng = np.random.default_rng(3)
    x32 = rng.integers(-(1 << 31), 1 << 31, 2 * 5000).astype(np.int32)
    d32, b32 = gpu_block(x32, 2, 32, 4)
    d16, b16 = gpu_block(ar_audio(2, 4096 + 9, 16), 2, 16, 2)
    fb = [le_block(fixture_stream(fx), len(fx["samples"]), fx["channels"], fx["bits"]) for fx in FIXTURES]
    out = FL.decompress_many([fb[0], b32, fb[1], b16, fb[2]])
    assert out[1] == d32 and out[3] == d16
    for fx, pcm in zip(FIXTURES, (out[0], out[2], out[4])):
        check_fixture_pcm(fx, pcm)


# ---- b. the GPU encoder's streams under the independent reader ----

FORMATS = [(1, 8, 1), (2, 16, 2), (2, 24, 3), (3, 12, 2), (2, 32, 4), (8, 20, 3)]  # channels, bits, bytes
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 1]  # samples per channel
ENC_CASES = [(c, b, nb, n, 5, "ar") for c, b, nb in FORMATS for n in SIZES]
ENC_CASES += [(c, b, nb, n, 5, kind) for c, b, nb in FORMATS for n in (17, 4097) for kind in ("const", "wasted")]
ENC_CASES += [(2, 32, 4, n, 5, "full32") for n in (17, 4097, 2 * 4096 + 1)]
ENC_CASES += [(2, 16, 2, 4097, 0, "ar"), (2, 24, 3, 4097, 8, "ar"), (2, 32, 4, 4097, 8, "full32")]


def enc_input(kind, channels, n, bits):
    """Interleaved int32 samples: all-pole 'audio' (ar_audio of test_gpu_flac.py); with channel 0 constant; with the
    last channel's low 3 bits wasted (bit 3 set, so exactly 3); or, 32-bit stereo, full scale: L = -2^31,
    R = 2^31 - 1 alternating with its mirror (a side channel of -(2^32 - 1) and 2^32 - 1: 33 bits), then uniform
    noise over the whole range."""
    if kind == "full32":
        rng = np.random.default_rng(n)
        x = rng.integers(-(1 << 31), 1 << 31, (n, 2))
        lo, hi = -(1 << 31), (1 << 31) - 1
        half = (n + 1) // 2
        x[:half:2] = (lo, hi)
        x[1:half:2] = (hi, lo)
        return x.reshape(-1).astype(np.int32)
    x = ar_audio(channels, n, bits, seed=n % 97 + bits).reshape(n, channels).astype(np.int64)
    if kind == "const":
        x[:, 0] = 1234 % (1 << (bits - 2))
    elif kind == "wasted":
        x[:, -1] = (x[:, -1] & ~7) | 8
    return x.reshape(-1).astype(np.int32)


@pytest.mark.parametrize("channels,bits,nbytes,n,level,kind", ENC_CASES)
def test_gpu_encoder_under_the_independent_reader(channels, bits, nbytes, n, level, kind):
    x = enc_input(kind, channels, n, bits)
    data, block = gpu_block(x, channels, bits, nbytes, level)
    d = FL.FlacBlockDecompressor(block)
    s = d.stream
    info = R.parse_streaminfo(s)
    # what the settings of the reference's compressor imply: fixed blocks of 4096, the stream's true shape
    assert (info.min_blocksize, info.max_blocksize, info.sample_rate) == (4096, 4096, 48000)
    assert (info.channels, info.bits, info.total_samples) == (channels, bits, n)
    assert info.blocks == ((0, 34),) and info.frames_at == 42
    frames = R.walk_frames(s, info)  # (raises on any broken field rule)
    assert all(f.crc8_ok and f.crc16_ok for f in frames)
    assert [f.blocksize for f in frames] == [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
    assert frames[-1].pos + frames[-1].length == len(s)
    assert R.decode(s) == x.tolist()
    st, y, ch, b = F.decode(s, x.size)
    assert st == F.OK and (ch, b) == (channels, bits) and np.array_equal(y, x)
    assert d.decompress() == data


def test_gpu_encoder_frame_number_128():
    """129 frames of mono 8-bit samples: the frame number reaches 128, two UTF-8 bytes.  Silence for most frames
    (constant subframes, which the walker passes at once), audio around the frames of interest, two of noise."""
    n = 129 * 4096
    x = np.zeros(n, np.int32)
    rng = np.random.default_rng(8)
    for f in (0, 1, 126, 127, 128):
        x[f * 4096:(f + 1) * 4096] = ar_audio(1, 4096, 8, seed=f)
    for f in (5, 64):
        x[f * 4096:(f + 1) * 4096] = rng.integers(-128, 128, 4096)
    data, block = gpu_block(x, 1, 8, 1)
    d = FL.FlacBlockDecompressor(block)
    frames = R.walk_frames(d.stream)
    assert [f.coded for f in frames] == list(range(129))
    assert all(f.crc8_ok and f.crc16_ok and f.blocksize == 4096 for f in frames)
    assert R.parse_header(d.stream, frames[128].pos).length == R.parse_header(d.stream, frames[127].pos).length + 1
    assert d.decompress() == data


def test_gpu_decodes_frame_numbers_across_the_utf8_lengths():
    """The restatement's block-size-16 stream of test_flac_conformance.py (frame numbers 127 -> 128 and
    2047 -> 2048) decoded by the GPU."""
    x = many_small_frames()
    block = le_block(F.encode(x, 1, 8, 16), x.size, 1, 8)
    assert FL.decompress(block) == x.astype(np.int8).tobytes()


# ---- c. phantom syncs ----

def direct_decode(body: bytes, channels: int, bits: int, max_bs: int, n: int, max_cand: int):
    """One rpp_flac_decode call: (status, candidates found, interleaved samples)."""
    L = N.lib()
    d_in = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(DEV)
    x = torch.zeros(n * channels, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    ncand = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(L.rpp_flac_decode_workspace_bytes(len(body), channels, bits, max_bs, max_cand))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    rc = L.rpp_flac_decode(C.c_void_p(d_in.data_ptr()), len(body), channels, bits, max_bs, n,
                           C.c_void_p(x.data_ptr()), C.c_void_p(status.data_ptr()), max_cand,
                           C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(ncand.data_ptr()),
                           C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == N.RPP_OK
    torch.cuda.synchronize()
    return int(status.item()), int(ncand.item()), x.cpu().numpy()


def check_phantoms_are_candidates(name):
    """The planted phantoms exist on the CPU (the scan rule restated) and on the GPU (d_ncand of a direct
    rpp_flac_decode call with room for all): a malformed phantom would make the case vacuous."""
    p, s = phantom_case(name)
    body = s[42:]
    cpu = R.count_header_candidates(body, p.channels, 16, BS)
    assert cpu >= 3 + p.planted
    st, found, y = direct_decode(body, p.channels, 16, BS, N_PHANTOM, cpu + 64)
    print(f"phantoms[{name}]: planted {p.planted} + 3 true frames, CPU count {cpu}, d_ncand {found}")
    assert found >= 3 + p.planted and found == cpu
    assert st == N.RPP_OK and np.array_equal(y, p.samples())
    return p, s


@pytest.mark.parametrize("name", sorted(set(PHANTOMS) - {"many_headers"}))
def test_phantom_candidates_are_rejected(name):
    """Cases 1-3 (see the builders in test_flac_conformance.py): a header whose frame does not parse or fails its
    CRC-16; a whole valid frame inside a frame's payload, mono and in the second subframe of a stereo frame; a
    whole valid frame that ends where a true frame ends, shares its CRC-16 and so has the next true frame as its
    successor -- numbered to overlap that frame, or numbered so that every link holds and only the sum of the block
    sizes and the serial walk reject it.  The result is the samples themselves."""
    p, s = check_phantoms_are_candidates(name)
    block = le_block(s, p.samples().size, p.channels, 16)
    assert FL.decompress(block) == p.pcm()
    assert FL.decompress_many([block])[0] == p.pcm()


def _facade_exe():
    exe = ROOT / "tests" / "cpp" / "build" / "facade_test"
    if not exe.exists():
        subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build.sh")], check=True)
    return exe


def _cpp_decompress(tmp_path, block: bytes):
    (tmp_path / "block.bin").write_bytes(block)
    out = tmp_path / "pcm.bin"
    r = subprocess.run([str(_facade_exe()), "--flac-decompress", str(tmp_path / "block.bin"), str(out)],
                       capture_output=True, text=True, timeout=120)
    return r, (out.read_bytes() if out.exists() else None)


def test_candidate_table_overflow_is_retried(tmp_path):
    """Case 4: 1200 distinct valid headers in the payload, far more than the first table of 8292 / 4096 + 65 = 67
    holds; candidates are dropped in atomic order, true frames among them, and each caller decodes again with room
    for all: FL.decompress, FL.decompress_many (this block second of three) and the C++ flac_block_decompressor."""
    p, s = check_phantoms_are_candidates("many_headers")
    assert 3 + p.planted > N_PHANTOM // BS + 65
    block = le_block(s, p.samples().size, 1, 16)
    d = FL.FlacBlockDecompressor(block)
    assert d._plan()[6] == 67
    assert d.decompress() == p.pcm()
    d16, b16 = gpu_block(ar_audio(2, 5000, 16), 2, 16, 2)
    d8, b8 = gpu_block(ar_audio(1, 300, 8), 1, 8, 1)
    assert FL.decompress_many([b16, block, b8]) == [d16, p.pcm(), d8]
    r, pcm = _cpp_decompress(tmp_path, block)
    assert r.returncode == 0 and "flac-decompress: OK" in r.stdout, r.stdout + r.stderr
    assert pcm == p.pcm()


def test_candidate_table_overflow_with_a_corrupt_frame(tmp_path):
    """Case 5: the stream of case 4 with one byte of true frame 1 flipped: all three callers report the FLAC error
    after their retry; none returns samples."""
    p, s = phantom_case("many_headers")
    frames = R.walk_frames(s)
    bad = bytearray(s)
    bad[frames[1].pos + 7 + 7900] ^= 0x20  # (payload of frame 1, past the planted headers)
    block = le_block(bytes(bad), p.samples().size, 1, 16)
    with pytest.raises(RuntimeError, match="FLAC"):
        FL.decompress(block)
    d16, b16 = gpu_block(ar_audio(2, 5000, 16), 2, 16, 2)
    with pytest.raises(RuntimeError, match="FLAC"):
        FL.decompress_many([b16, block, b16])
    r, pcm = _cpp_decompress(tmp_path, block)
    assert r.returncode == 3 and "[FLAC] failed to process frame" in r.stdout, r.stdout + r.stderr
    assert pcm is None
