"""GPU tests of the file extraction: ``rpp_extract_gather_batch`` bit for bit against the host definition over every
family of tests/extract_cases.py (output pre-filled, guard bytes around the files, the bytes of a bad chunk left
alone, the statuses), ``file_checksums`` against ``file_hash_batch`` over the same bytes uploaded contiguously,
``check_files`` on one flipped byte, and ``decode_sections_device`` + ``extract_files`` over a mixed image fragment."""

import functools

import numpy as np
import pytest
import torch

import extract_cases as EC
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec, dedup
from dwarfs_amd import extract as X
from dwarfs_amd import lz4 as L4
from dwarfs_amd import zstd as Z
from test_extract_host import FILL, expect, flat_blocks, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
FAMILIES = ["align", "tile_edges", "block_edges", "holes", "empty", "bad"]


def device_blocks(case):
    flat, boff, bsz = flat_blocks(case)
    return X.padded_blocks(torch.from_numpy(flat.copy()).to(DEV)), boff, bsz, len(flat)


@pytest.mark.parametrize("family", FAMILIES)
def test_gather_batch_is_the_host_gather(family):
    for case in EC.families(X.tile_bytes(), GUARD)[family]:
        table, file_dst, chunk_dst, out_bytes = tables(case, GUARD)
        flat, boff, bsz = flat_blocks(case)
        host_out = np.full(out_bytes, FILL, np.uint8)
        _, _, _, host_status = X.host_gather(flat, boff, bsz, table, file_dst=file_dst, chunk_dst=chunk_dst,
                                             out_bytes=out_bytes, out=host_out)
        d_blocks, _, _, blocks_bytes = device_blocks(case)
        plan = X.plan_gather(table, DEV, file_dst=file_dst, chunk_dst=chunk_dst, out_bytes=out_bytes)
        out = torch.full((out_bytes + 64,), FILL, dtype=torch.uint8, device=DEV)
        status = X.gather_into(d_blocks, boff, bsz, plan, out, blocks_bytes=blocks_bytes)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert status.cpu().tolist() == host_status.tolist(), case.name
        assert got[:out_bytes].tobytes() == host_out.tobytes(), case.name
        assert (got[out_bytes:] == FILL).all(), case.name
        want, want_status = expect(case, table, chunk_dst, out_bytes)
        assert got[:out_bytes].tobytes() == want and host_status.tolist() == want_status, case.name
        # the guard bytes before, between and after the files' regions
        clean = X.FileTable.from_files(case.files)
        mask = np.ones(out_bytes, bool)
        for at, n in zip(file_dst.tolist(), clean.file_sizes.tolist()):
            mask[at:at + n] = False
            assert mask[at - GUARD:at].all() and mask[at + n:at + n + GUARD].all(), case.name  # (the guards are there)
        assert (got[:out_bytes][mask] == FILL).all(), case.name
        # a bad chunk's destination is as it was
        for c, _ in case.patches:
            at, room = int(chunk_dst[c]), int(chunk_dst[c + 1] - chunk_dst[c])
            assert room > 0 and (got[at:at + room] == FILL).all(), case.name
        if family == "bad" and not case.patches:
            bad = case.bad_files[0]
            rows = table.chunks.tolist()
            for c in range(int(table.first_chunk[bad]), int(table.first_chunk[bad + 1])):
                b, o, s = rows[c]
                if b != EC.HOLE and (b >= len(case.blocks) or o + s > len(case.blocks[b])):
                    assert (got[int(chunk_dst[c]):int(chunk_dst[c]) + s] == FILL).all(), case.name


def file_bytes(case):
    return [b"".join(bytes(s) if b == EC.HOLE else case.blocks[b][o:o + s] for b, o, s in f) for f in case.files]


def striped_case():
    """One file of 5000 bytes cut into chunks of 1..97 bytes across 7 blocks: the chunk edges cross XXH3's 64-byte
    stripes and 1024-byte blocks and SHA-512's 128-byte blocks at every phase."""
    blocks = [EC.block_bytes(700 + b, 1500 + 13 * b) for b in range(7)]
    chunks, left, k = [], 5000, 0
    while left:
        size = min(1 + (37 * k) % 97, left)
        chunks.append((k % 7, (53 * k) % 1300, size))
        left -= size
        k += 1
    assert {s for _, _, s in chunks} >= set(range(1, 98)) and sum(s for _, _, s in chunks) == 5000
    return EC.Case("striped_5000", blocks, [chunks, [(3, 1, 700)], [], [(0, 0, 16)], [(1, 5, 300)], [(2, 9, 300)],
                                            [(5, 0, 200)]])


@functools.lru_cache(maxsize=None)
def checksum_cases():
    return [EC.align_case(), EC.holes_cases(X.tile_bytes())[0], striped_case()]


@pytest.mark.parametrize("algo", dedup.ALGORITHMS)
def test_file_checksums_are_the_hashes_of_the_contiguous_bytes(algo):
    for case in checksum_cases():
        want_files = file_bytes(case)
        table = X.FileTable.from_files(case.files)
        d_blocks, boff, bsz, _ = device_blocks(case)
        # the same bytes uploaded contiguously
        sizes = np.array([len(f) for f in want_files], np.int64)
        offs = np.zeros(len(sizes), np.int64)
        offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
        flat = np.zeros(int(offs[-1] + sizes[-1]) + 16, np.uint8)
        for o, f in zip(offs, want_files):
            flat[o:o + len(f)] = np.frombuffer(f, np.uint8)
        want = dedup.file_hash_batch(torch.from_numpy(flat).to(DEV), offs, sizes, algo).cpu().numpy()
        max_bytes = {"align": 16384, "holes": 4096, "striped_5000": 512}[case.name]  # three batches and more
        cut = X.batches(table.file_sizes, max_bytes)
        assert len(cut) >= 4 and any(hi - lo == 1 and sizes[lo] > max_bytes for lo, hi in cut) == (case.name != "align")
        for mb in (max_bytes, X.DEFAULT_MAX_BYTES):
            digests, status = X.file_checksums(d_blocks, boff, bsz, table, algo, max_bytes=mb, device=DEV)
            assert status.cpu().tolist() == [0] * len(sizes), case.name
            assert np.array_equal(digests.cpu().numpy(), want), (case.name, mb)
        assert X.hexdigests(digests) == [bytes(r).hex() for r in want]


def test_check_files_marks_the_files_that_use_a_flipped_byte():
    case = EC.block_edges_case()
    table = X.FileTable.from_files(case.files)
    d_blocks, boff, bsz, _ = device_blocks(case)
    expected, status = X.file_checksums(d_blocks, boff, bsz, table, device=DEV)
    assert X.check_files(d_blocks, boff, bsz, table, expected, device=DEV) == []
    assert X.check_files(d_blocks, boff, bsz, table, X.hexdigests(expected), device=DEV, max_bytes=2048) == []
    block, byte = 1, 130
    users = [f for f, rows in enumerate(case.files) if any(b == block and o <= byte < o + s for b, o, s in rows)]
    assert 2 < len(users) < len(case.files)
    broken = d_blocks.clone()
    broken[boff[block] + byte] ^= 0x10
    for algo in dedup.ALGORITHMS:
        want = X.file_checksums(d_blocks, boff, bsz, table, algo, device=DEV)[0]
        assert X.check_files(broken, boff, bsz, table, want, algo, device=DEV) == users, algo
    # a file whose status is not OK is marked whatever its digest
    bad = EC.bad_cases()[0]
    table = X.FileTable.from_files(bad.files)
    d_blocks, boff, bsz, _ = device_blocks(bad)
    digests, status = X.file_checksums(d_blocks, boff, bsz, table, device=DEV)
    assert status.cpu().tolist() == [0, 0, N.RPP_BAD_CHUNK, 0, 0]
    assert X.check_files(d_blocks, boff, bsz, table, digests, device=DEV) == [2]
    with pytest.raises(RuntimeError, match="^file 2: BAD_CHUNK"):
        X.extract_files(d_blocks, boff, bsz, table, device=DEV)


def test_decode_sections_device_then_extract_files():
    text = (b"The archive grows by one more block while the scanner reads on. " * 400)[:20011]
    lz4_blocks = [text, EC.block_bytes(801, 4096)]  # (random bytes do not shrink: a NONE section)
    zstd_blocks = [text[::-1] * 2, b"", bytes(70000), EC.block_bytes(802, 5000)]
    rng = np.random.default_rng(5)
    pix = [(rng.poisson(900, n).astype(np.uint16) << 1).byteswap().tobytes() for n in (3000, 1111)]
    meta = '{"endianness":"big","bytes_per_sample":2,"unused_lsb_count":1,"component_count":1}'
    image = (block_codec.compress_many_sections(pix, meta, first_number=0)
             + L4.Lz4BlockCompressor(None, DEV).compress_many_sections(lz4_blocks, None, first_number=2)
             + Z.ZstdBlockCompressor(device=DEV).compress_many_sections(zstd_blocks, first_number=4))
    plain = block_codec.decompress_sections(image, verify=1, device=DEV)
    assert plain == pix + lz4_blocks + zstd_blocks
    blocks, boff, bsz = block_codec.decode_sections_device(image, verify=1, device=DEV)
    assert blocks.data_ptr() % 16 == 0 and blocks.numel() % 16 == 0 and bsz.tolist() == [len(p) for p in plain]
    host = blocks.cpu().numpy()
    assert [host[o:o + n].tobytes() for o, n in zip(boff.tolist(), bsz.tolist())] == plain
    files = [[X.Chunk(b, 0, len(plain[b]))] for b in range(len(plain))]               # every block whole
    files += [[X.Chunk(2, 100, 5000), X.Hole(33), X.Chunk(0, 7, 555), X.Chunk(4, 1, 20000), X.Chunk(6, 69999, 1)],
              [], [X.Chunk(3, 4095, 1), X.Chunk(1, 0, 2222), X.Chunk(7, 17, 4983)]]
    want = [b"".join(bytes(c.size) if isinstance(c, X.Hole) else plain[c.block][c.offset:c.offset + c.size] for c in f)
            for f in files]
    table = X.FileTable.from_files(files)
    assert X.extract_files(blocks, boff, bsz, table, device=DEV) == want
    assert X.extract_files(blocks, boff, bsz, table, device=DEV, max_bytes=30000) == want
    data, offsets, sizes, status = X.gather_files(blocks, boff, bsz, table, device=DEV)
    assert data.is_cuda and offsets.is_cuda and sizes.is_cuda and status.is_cuda and sizes.tolist() == [len(w) for w in want]
    broken = bytearray(image)
    broken[len(image) // 2] ^= 1
    with pytest.raises(RuntimeError, match="^block data integrity check failed$"):
        block_codec.decode_sections_device(bytes(broken), verify=2, device=DEV)
    empty = block_codec.decode_sections_device(b"", device=DEV)
    assert empty[1].numel() == 0 and empty[2].numel() == 0
