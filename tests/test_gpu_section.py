"""GPU tests of the section checksums and headers (rpp_xxh3_64_batch ... rpp_sections_verify_batch and
their Python / C++ layers).  Every comparison is for equality, against tests/golden/section_kat.json: the
reference's own non-BLOCK sections and synthetic messages with digests from xxhash / hashlib."""

import hashlib
import json
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import datagen
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import section as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_section_kat as K  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "section_kat.json").read_text())


@pytest.fixture(scope="module")
def messages(kat):
    """The synthetic messages' bytes, regenerated once."""
    return [K.message_bytes(m) for m in kat["messages"]]


@pytest.fixture(scope="module")
def ref_sections(kat):
    return [(bytes.fromhex(s["header"]), bytes.fromhex(s["payload"])) for s in kat["sections"]]


def _u64(hexes):
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64)


def _split(s, width):
    return [s[i:i + width] for i in range(0, len(s), width)]


def _place(chunks, misalign):
    """Chunks laid into one buffer, chunk i starting at a 16-byte boundary + misalign(i); returns the buffer
    (with 16 spare bytes) and the offsets."""
    offs, at = [], 0
    for i, c in enumerate(chunks):
        at = (at + 15) // 16 * 16 + misalign(i)
        offs.append(at)
        at += len(c)
    buf = np.zeros(at + 16, np.uint8)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = np.frombuffer(c, np.uint8)
    return buf, offs


def test_synthetic_lengths_one_batch(kat, messages):
    buf, offs = _place(messages, lambda i: (5 * i) % 16)
    d = torch.from_numpy(buf).to(DEV)
    sizes = [len(m) for m in messages]
    got_x = S.xxh3_64_batch(d, offs, sizes).cpu().numpy().view(np.uint64)
    got_s = S.sha512_256_batch(d, offs, sizes).cpu().numpy()
    want_x = _u64(m["xxh3_64"] for m in kat["messages"])
    bad = np.nonzero(got_x != want_x)[0]
    assert len(bad) == 0, [(sizes[i], f"{got_x[i]:016x}", kat["messages"][i]["xxh3_64"]) for i in bad[:8]]
    for i, m in enumerate(kat["messages"]):
        assert got_s[i].tobytes().hex() == m["sha512_256"], sizes[i]


def test_prefixes_and_payload_misalignments(kat, messages):
    """Every message behind prefixes of 0, 1, 16, 24, 47 and 64 bytes, its payload at each misalignment 0..15,
    in one batch per hash; against the stored digests of the concatenations."""
    n = len(messages)
    plens = kat["prefix_lengths"]
    assert plens == [0, 1, 16, 24, 47, 64]
    copies = [m for mis in range(16) for m in messages]
    buf, offs = _place(copies, lambda i: i // n)
    d = torch.from_numpy(buf).to(DEV)
    rows = np.stack([np.frombuffer(K.prefix_bytes(i), np.uint8) for i in range(n)])
    m_off, m_size, m_row, m_plen, want_x, want_s = [], [], [], [], [], []
    for p in plens:
        wx = _split(kat["prefixed"][str(p)]["xxh3_64"], 16)
        ws = _split(kat["prefixed"][str(p)]["sha512_256"], 64)
        for mis in range(16):
            for i in range(n):
                assert offs[mis * n + i] % 16 == mis
                m_off.append(offs[mis * n + i])
                m_size.append(len(messages[i]))
                m_row.append(i)
                m_plen.append(p)
                want_x.append(wx[i])
                want_s.append(ws[i])
    d_rows = torch.from_numpy(rows[np.array(m_row)]).to(DEV)
    d_plen = torch.tensor(m_plen, dtype=torch.int32, device=DEV)
    got_x = S.xxh3_64_batch(d, m_off, m_size, d_rows, d_plen).cpu().numpy().view(np.uint64)
    got_s = S.sha512_256_batch(d, m_off, m_size, d_rows, d_plen).cpu().numpy()
    bad = np.nonzero(got_x != _u64(want_x))[0]
    assert len(bad) == 0, [(m_plen[i], m_off[i] % 16, m_size[i]) for i in bad[:8]]
    want = np.frombuffer(bytes.fromhex("".join(want_s)), np.uint8).reshape(-1, 32)
    bad = np.nonzero((got_s != want).any(axis=1))[0]
    assert len(bad) == 0, [(m_plen[i], m_off[i] % 16, m_size[i]) for i in bad[:8]]


@pytest.mark.parametrize("frame_bytes", [0, 7, 32])
def test_headers_reproduce_reference_sections(ref_sections, frame_bytes):
    """rpp_section_headers_batch on each reference section's payload gives its 64 header bytes; with the
    payload's first bytes passed as the frame row (as a ricepp block's frame header is), the same.  The one
    byte that may differ is the minor version (index 7, covered by neither checksum): the call writes the
    current MINOR_VERSION 5, the reference's test images were written at minor versions 2..5."""
    assert {h[7] for h, _ in ref_sections} <= {2, 3, 4, 5}
    for hdr, payload in ref_sections:
        hdr = hdr[:7] + b"\x05" + hdr[8:]
        number, typ, comp, length = struct.unpack_from("<IHHQ", hdr, 48)
        assert length == len(payload)
        fb = min(frame_bytes, len(payload))
        buf, offs = _place([payload[fb:]], lambda i: 3)
        d = torch.from_numpy(buf).to(DEV)
        got = S.section_headers_batch(d, offs, [len(payload) - fb], number, typ, comp,
                                      [payload[:fb]] if frame_bytes else None)
        assert got.cpu().numpy().tobytes() == hdr


def test_headers_batch_numbers_sections(ref_sections):
    """One call for many sections: number = first_number + b, every header as a call of its own gives it."""
    payloads = [p for _, p in ref_sections]
    buf, offs = _place(payloads, lambda i: i % 16)
    d = torch.from_numpy(buf).to(DEV)
    sizes = [len(p) for p in payloads]
    got = S.section_headers_batch(d, offs, sizes, 1000, 8, 2).cpu().numpy()
    for b, p in enumerate(payloads):
        h = got[b].tobytes()
        assert h[:8] == b"DWARFS\x02\x05" and struct.unpack_from("<IHHQ", h, 48) == (1000 + b, 8, 2, len(p))
        assert hashlib.new("sha512_256", h[40:] + p).digest() == h[8:40]
    st = S.sections_verify_batch(*_image_of([(got[b].tobytes(), p) for b, p in enumerate(payloads)]), level=2)
    assert st.cpu().tolist() == [0] * len(payloads)


def _image_of(sections, cut=0):
    """(device image, image_bytes, section offsets) of header + payload pairs laid back to back."""
    image = b"".join(h + p for h, p in sections)
    offs = np.cumsum([0] + [len(h) + len(p) for h, p in sections])[:-1]
    host = np.frombuffer(image, np.uint8)[:len(image) - cut]
    return torch.from_numpy(host.copy()).to(DEV), len(image) - cut, offs


def test_verify_reference_image(ref_sections):
    n = len(ref_sections)
    for level in (1, 2):
        st = S.sections_verify_batch(*_image_of(ref_sections), level=level)
        assert st.cpu().tolist() == [N.RPP_OK] * n

    def corrupt(idx, at, payload=False):
        secs = [(bytearray(h), bytearray(p)) for h, p in ref_sections]
        (secs[idx][1] if payload else secs[idx][0])[at] ^= 0x10
        return [(bytes(h), bytes(p)) for h, p in secs]

    big = max(range(n), key=lambda i: len(ref_sections[i][1]))
    for idx, at in ((0, 0), (big, 1500), (5, len(ref_sections[5][1]) - 1)):  # (short, multi-block long, mid classes)
        for level in (1, 2):
            st = S.sections_verify_batch(*_image_of(corrupt(idx, at, payload=True)), level=level).cpu().tolist()
            assert st == [N.RPP_CHECKSUM_MISMATCH if i == idx else N.RPP_OK for i in range(n)]
    # a flipped SHA byte: level 1 does not look at it
    assert S.sections_verify_batch(*_image_of(corrupt(3, 8 + 17)), level=1).cpu().tolist() == [N.RPP_OK] * n
    st = S.sections_verify_batch(*_image_of(corrupt(3, 8 + 17)), level=2).cpu().tolist()
    assert st == [N.RPP_CHECKSUM_MISMATCH if i == 3 else N.RPP_OK for i in range(n)]
    # a flipped XXH3 byte: both levels (the SHA covers it)
    for level in (1, 2):
        st = S.sections_verify_batch(*_image_of(corrupt(4, 40)), level=level).cpu().tolist()
        assert st == [N.RPP_CHECKSUM_MISMATCH if i == 4 else N.RPP_OK for i in range(n)]
    # a cut image: the last section's payload, then its header, run past the end
    for cut in (1, len(ref_sections[-1][1]) + 1):
        st = S.sections_verify_batch(*_image_of(ref_sections, cut=cut), level=2).cpu().tolist()
        assert st == [N.RPP_OK] * (n - 1) + [N.RPP_TRUNCATED_INPUT]
    # bad magic, another major version
    for at in (2, 6):
        st = S.sections_verify_batch(*_image_of(corrupt(7, at)), level=1).cpu().tolist()
        assert st == [N.RPP_INVALID_ARGUMENT if i == 7 else N.RPP_OK for i in range(n)]


def test_assemble_every_destination_misalignment():
    rng = np.random.default_rng(11)
    # (sizes fixed so that header and payload destinations take every misalignment, asserted below)
    sizes = [0, 1, 2, 15, 16, 17, 31, 33, 5000, 70001] + [(43 * k + 7) % 300 for k in range(70)]
    frames = [rng.integers(0, 256, (5 * k) % 33, dtype=np.uint8).tobytes() for k in range(len(sizes))]
    frames[0], frames[1] = b"", bytes(range(32))
    payloads = [rng.integers(0, 256, s, dtype=np.uint8).tobytes() for s in sizes]
    headers = rng.integers(0, 256, (len(sizes), 64), dtype=np.uint8)
    buf, offs = _place(payloads, lambda i: (7 * i + 1) % 16)
    want = b"".join(headers[b].tobytes() + frames[b] + payloads[b] for b in range(len(sizes)))
    image = torch.full((len(want) + 64,), 0xAA, dtype=torch.uint8, device=DEV)
    res = S.sections_assemble_batch(torch.from_numpy(headers).to(DEV), torch.from_numpy(buf).to(DEV), offs, sizes,
                                    0, frames, image=image)
    assert int(res.total.item()) == len(want)
    sec_sizes = [64 + len(f) + len(p) for f, p in zip(frames, payloads)]
    assert res.sizes.cpu().tolist() == sec_sizes
    sec_offs = res.offsets.cpu().tolist()
    assert sec_offs == [int(v) for v in np.cumsum([0] + sec_sizes)[:-1]]
    assert {o % 16 for o in sec_offs} == set(range(16))
    assert {(o + 64 + len(f)) % 16 for o, f in zip(sec_offs, frames)} == set(range(16))
    got = image.cpu().numpy().tobytes()
    assert got[:len(want)] == want
    assert got[len(want):] == b"\xaa" * 64  # (nothing written past the fragment)
    # without frames
    want = b"".join(headers[b].tobytes() + payloads[b] for b in range(len(sizes)))
    res = S.sections_assemble_batch(torch.from_numpy(headers).to(DEV), torch.from_numpy(buf).to(DEV), offs, sizes,
                                    len(want))
    assert res.bytes() == want


def test_compress_many_sections_end_to_end():
    rng = np.random.default_rng(5)
    meta = '{"endianness":"big","bytes_per_sample":2,"unused_lsb_count":0,"component_count":1}'
    blocks = [datagen.poisson_data(rng, 4096, lam=500, ulsb=0, big_endian=True).tobytes() for _ in range(8)]
    comp = block_codec.RiceppBlockCompressor(128)
    image = comp.compress_many_sections(blocks, meta, first_number=40)
    assert image == block_codec.compress_many_sections(blocks, meta, first_number=40)
    plain = comp.compress_many(blocks, meta)
    found, bad = S.walk(image)
    assert bad is None and len(found) == 8
    try:
        import xxhash
    except ImportError:
        xxhash = None
    for b, (at, h) in enumerate(found):
        raw, data = image[at:at + 64], image[at + 64:at + 64 + h.length]
        assert raw[:8] == b"DWARFS\x02\x05"
        assert (h.number, h.type, h.compression, h.length) == (40 + b, 0, 7, len(plain[b]))
        assert data == plain[b]  # frame header + bitstream, as compress_many gives them
        assert hashlib.new("sha512_256", raw[40:] + data).digest() == raw[8:40]
        if xxhash:
            assert xxhash.xxh3_64_intdigest(raw[48:] + data) == h.xxh3_64
    d = torch.from_numpy(np.frombuffer(image, np.uint8).copy()).to(DEV)
    assert S.sections_verify_batch(d, len(image), [at for at, _ in found], 2).cpu().tolist() == [0] * 8
    for verify in (0, 1, 2):
        assert block_codec.decompress_sections(image, verify=verify) == blocks
    for at in (found[3][0] + 64 + 100, found[6][0] + 50, len(image) - 1):  # bitstream, header field, last byte
        bad_image = bytearray(image)
        bad_image[at] ^= 1
        with pytest.raises(RuntimeError, match="^block data integrity check failed$"):
            block_codec.decompress_sections(bytes(bad_image))
    with pytest.raises(RuntimeError, match="^block data integrity check failed$"):
        block_codec.decompress_sections(image[:-3])
    sha_flipped = bytearray(image)
    sha_flipped[found[2][0] + 9] ^= 1
    assert block_codec.decompress_sections(bytes(sha_flipped), verify=1) == blocks
    with pytest.raises(RuntimeError, match="^block data integrity check failed$"):
        block_codec.decompress_sections(bytes(sha_flipped), verify=2)
    assert comp.compress_many_sections([], meta) == b"" and block_codec.decompress_sections(b"") == []


def test_cpp_sections(ref_sections, tmp_path):
    """tests/cpp/section_test: ricepp_amd::make_sections / check_sections against two reference sections
    (given as an image file) and one round trip."""
    exe = ROOT / "tests" / "cpp" / "build" / "section_test"
    if not exe.exists():
        subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_section.sh")], check=True)
    big = max(ref_sections, key=lambda s: len(s[1]))
    small = min(ref_sections, key=lambda s: len(s[1]))
    path = tmp_path / "two_sections.bin"
    path.write_bytes(small[0] + small[1] + big[0] + big[1])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "section_test: OK" in r.stdout
