"""GPU tests of the named digests: ``rpp_digest_batch`` bit for bit against tests/golden/digest_kat.bin (hashlib's
digests) on every batch shape of tests/digest_cases.py -- the length sweep, the boundary lengths at every payload
misalignment, batches around the wave width and one above the lane spread, a select mask over a pre-filled output with
guard bytes behind the last row -- the three forwarded names against ``dedup.file_hash_batch``, ``file_checksums`` /
``check_files`` with the new names against hashlib over the host extraction, and one graph-capture replay."""

import functools
import hashlib

import numpy as np
import pytest
import torch

import digest_cases as DC
import extract_cases as EC
from dwarfs_amd import _native as N
from dwarfs_amd import dedup, digest
from dwarfs_amd import extract as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def device_shape(shape):
    """One shape's buffer on the device, uploaded once and left unchanged: (data, offsets, sizes, indices)."""
    idx = DC.batch_shapes()[shape]
    buf, offs, sizes = DC.place(idx)
    data = torch.from_numpy(buf).to(DEV)
    assert data.data_ptr() % 16 == 0
    return data, torch.from_numpy(offs).to(DEV), torch.from_numpy(sizes).to(DEV), np.array(idx)


def device_digests(name, shape, select=None):
    data, offs, sizes, idx = device_shape(shape)
    width = DC.WIDTH[name]
    out = DC.guarded_out(len(idx), width, torch).to(DEV)
    got = digest.digest_batch(data, offs, sizes, name, select=select, out=out[:len(idx) * width])
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu().numpy(), DC.expected(name)[idx]


@pytest.mark.parametrize("name", DC.NEW)
def test_digest_batch_on_every_shape(name):
    for shape in DC.batch_shapes():
        got, want = device_digests(name, shape)
        DC.check_rows(got, want, what=(name, shape))


@pytest.mark.parametrize("name", DC.NEW)
def test_select_mask_over_a_prefilled_output(name):
    select = DC.select_mask(len(DC.batch_shapes()["all"]))
    got, want = device_digests(name, "all", select)
    DC.check_rows(got, want, select, what=(name, "select"))


def test_fresh_output_and_published_vectors():
    data = torch.from_numpy(np.frombuffer(b"abc", np.uint8).copy()).to(DEV)
    for name in DC.NEW:
        pub = DC.kat()["published"][name]
        got = digest.digest_batch(data, [0, 0, 1], [3, 0, 0], name.upper(), select=[1, 1, 0])
        assert got.is_cuda and tuple(got.shape) == (3, DC.WIDTH[name])
        assert digest.hexdigests(got) == [pub["abc"], pub["empty"], "00" * DC.WIDTH[name]], name
    with pytest.raises(ValueError, match="unknown digest algorithm 'shake128'"):
        digest.digest_batch(data, [0], [3], "shake128")


@pytest.mark.parametrize("name", DC.OLD)
def test_forwarded_names_are_file_hash_batch(name):
    data, offs, sizes, idx = device_shape("all")
    select = DC.select_mask(len(idx))
    want = dedup.file_hash_batch(data, offs, sizes, name, select=select)
    got = digest.digest_batch(data, offs, sizes, name, select=select)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(digest.digest_batch(data, offs, sizes, name), dedup.file_hash_batch(data, offs, sizes, name))


def test_sha512_256_device_and_host_forms_agree():
    data, offs, sizes, idx = device_shape("n65")
    got = digest.digest_batch(data, offs, sizes, "sha512-256").cpu()
    assert torch.equal(got, digest.digest_batch(data.cpu(), offs.cpu(), sizes.cpu(), "sha512-256"))


def checksum_case():
    """A small table with a hole, an empty file and a bad chunk (file 2 of the bad case), over blocks whose sizes
    are no multiples of 16."""
    bad = EC.bad_cases()[0]
    files = [list(f) for f in bad.files] + [[EC.hole(100), (0, 5, 300)], [], [(1, 0, 300), EC.hole(77), (0, 1, 50)],
                                           [(0, 0, 700)], [(1, 3, 0)]]
    return bad.blocks, files


@pytest.mark.parametrize("name,hname", [("sha256", "sha256"), ("sha1", "sha1"), ("blake2b512", "blake2b")])
def test_file_checksums_and_check_files(name, hname):
    blocks, files = checksum_case()
    flat = np.frombuffer(b"".join(blocks), np.uint8)
    boff, bsz = EC.block_offsets(blocks), [len(b) for b in blocks]
    table = X.FileTable.from_files(files)
    # the host extraction: the bytes of every file, zeros in the bad chunk's place
    data, offsets, sizes, host_status = X.gather_files(flat, boff, bsz, table, device="cpu")
    content = [data[o:o + n].numpy().tobytes() for o, n in zip(offsets.tolist(), sizes.tolist())]
    want = [hashlib.new(hname, c).hexdigest() for c in content]
    assert host_status.tolist() == [0, 0, N.RPP_BAD_CHUNK] + [0] * 7 and b"" in content
    d_blocks = X.padded_blocks(torch.from_numpy(flat.copy()).to(DEV))
    assert len(X.batches(table.file_sizes, 400)) >= 4
    for max_bytes in (X.DEFAULT_MAX_BYTES, 400):  # one batch; several, a file above max_bytes alone
        digests, status = X.file_checksums(d_blocks, boff, bsz, table, name, max_bytes=max_bytes, device=DEV)
        assert digests.is_cuda and status.cpu().tolist() == host_status.tolist()
        assert X.hexdigests(digests) == want, (name, max_bytes)
    # the device route and the host route agree
    host_digests, _ = X.file_checksums(flat, boff, bsz, table, name, device="cpu")
    assert torch.equal(digests.cpu(), host_digests)
    # check_files: the file with the bad chunk is marked whatever its digest; a wrong digest is found
    assert X.check_files(d_blocks, boff, bsz, table, want, name, device=DEV, max_bytes=400) == [2]
    wrong = list(want)
    wrong[5] = want[6]
    assert X.check_files(d_blocks, boff, bsz, table, wrong, name, device=DEV) == [2, 5]
    broken = d_blocks.clone()
    broken[boff[1] + 7] ^= 0x01
    users = [f for f, rows in enumerate(files) if any(b == 1 and o <= 7 < o + s for b, o, s in rows)]
    assert X.check_files(broken, boff, bsz, table, want, name, device=DEV) == sorted(set(users) | {2})
    with pytest.raises(ValueError, match="unknown digest algorithm 'crc32'"):
        X.file_checksums(d_blocks, boff, bsz, table, "crc32", device=DEV)


def test_digest_graph_capture():
    """One rpp_digest_batch call captured in a graph and replayed twice."""
    name = "sha256"
    data, offs, sizes, idx = device_shape("n65")
    out = digest.digest_batch(data, offs, sizes, name)  # (warm-up outside the capture; provides the buffer)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            digest.digest_batch(data, offs, sizes, name, out=out)
    want = DC.expected(name)[idx]
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
