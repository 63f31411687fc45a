"""CPU tests of the file extraction (no GPU needed): ``rpp_extract_host_gather``, the definition, against the
plain-Python restatement of tests/extract_cases.py (``model``: slices joined in place) over every family, the
statuses and the untouched neighbours of a bad chunk, the argument rules of both calls, the Python layer on
``device="cpu"``, and the host code alone under AddressSanitizer and UBSan."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import extract_cases as EC
from dwarfs_amd import _native as N
from dwarfs_amd import extract as X

ROOT = Path(__file__).resolve().parent.parent
FILL = 0xA5


def tables(case, guard=0):
    """(table with the case's patches, file_dst, chunk_dst, out_bytes): the destinations come from the rows as the
    case lists them, the patches go in afterwards.  With ``guard`` the files lie on 16-byte boundaries with at least
    ``guard`` bytes before, between and after them."""
    table = X.FileTable.from_files(case.files)
    file_dst = None
    if guard:
        file_dst, at = [], guard
        for n in table.file_sizes.tolist():
            file_dst.append(at)
            at = (at + n + guard + 15) // 16 * 16
    file_dst, chunk_dst, out_bytes = table.layout(file_dst=file_dst)
    out_bytes += guard
    for c, row in case.patches:
        table.chunks[c] = row
    return table, file_dst, chunk_dst, out_bytes


def flat_blocks(case):
    flat = np.frombuffer(b"".join(case.blocks), np.uint8)
    return flat, EC.block_offsets(case.blocks), [len(b) for b in case.blocks]


def expect(case, table, chunk_dst, out_bytes):
    out = bytearray([FILL]) * out_bytes
    status = EC.model(case.blocks, table.chunks.tolist(), chunk_dst.tolist(), table.first_chunk.tolist(), out)
    return bytes(out), status


@pytest.mark.parametrize("family", ["align", "tile_edges", "block_edges", "holes", "empty", "bad"])
@pytest.mark.parametrize("guard", [0, 64])
def test_host_gather_is_the_restatement(family, guard):
    for case in EC.families(X.tile_bytes(), guard)[family]:
        table, file_dst, chunk_dst, out_bytes = tables(case, guard)
        flat, boff, bsz = flat_blocks(case)
        out = np.full(out_bytes, FILL, np.uint8)
        got, _, _, status = X.host_gather(flat, boff, bsz, table, file_dst=file_dst, chunk_dst=chunk_dst,
                                          out_bytes=out_bytes, out=out)
        want, want_status = expect(case, table, chunk_dst, out_bytes)
        assert status.tolist() == want_status, case.name
        assert got.tobytes() == want, case.name
        assert [f for f, s in enumerate(want_status) if s] == list(case.bad_files), case.name
        assert set(want_status) <= {N.RPP_OK, N.RPP_BAD_CHUNK}


def test_a_bad_file_leaves_its_neighbours_right():
    for case in EC.bad_cases():
        table, file_dst, chunk_dst, out_bytes = tables(case)
        flat, boff, bsz = flat_blocks(case)
        out = np.full(out_bytes, FILL, np.uint8)
        X.host_gather(flat, boff, bsz, table, chunk_dst=chunk_dst, out_bytes=out_bytes, out=out)
        clean = X.FileTable.from_files(case.files)  # (the sizes before the patches)
        for f, (at, n) in enumerate(zip(file_dst.tolist(), clean.file_sizes.tolist())):
            if f in case.bad_files:
                continue
            want = b"".join(bytes(s) if b == EC.HOLE else case.blocks[b][o:o + s] for b, o, s in case.files[f])
            assert out[at:at + n].tobytes() == want, (case.name, f)
        # the bad chunk's own bytes are as they were, the good chunks of the same file are copied
        bad = case.bad_files[0]
        c0 = int(table.first_chunk[bad])
        rows = table.chunks[c0:int(table.first_chunk[bad + 1])].tolist()
        states = []
        for k, (b, o, s) in enumerate(rows):
            at, room = int(chunk_dst[c0 + k]), int(chunk_dst[c0 + k + 1] - chunk_dst[c0 + k])
            good = b == EC.HOLE and s <= room or b < len(case.blocks) and o + s <= len(case.blocks[b]) and s <= room
            if good:
                assert out[at:at + s].tobytes() == (bytes(s) if b == EC.HOLE else case.blocks[b][o:o + s])
            else:
                assert (out[at:at + room] == FILL).all(), case.name
            states.append(good)
        assert not all(states), case.name


def test_python_layer_on_the_cpu():
    case = EC.holes_cases(X.tile_bytes())[0]
    flat, boff, bsz = flat_blocks(case)
    files = [[X.Hole(s) if b == EC.HOLE else X.Chunk(b, o, s) for b, o, s in f] for f in case.files]
    table = X.FileTable.from_files(files)
    assert table.chunks.tolist() == X.FileTable.from_files(case.files).chunks.tolist()
    want = [b"".join(bytes(s) if b == EC.HOLE else case.blocks[b][o:o + s] for b, o, s in f) for f in case.files]
    assert table.file_sizes.tolist() == [len(w) for w in want] and table.nfiles == len(want)
    data, offsets, sizes, status = X.gather_files(flat, boff, bsz, table, device="cpu")
    assert status.tolist() == [0] * len(want) and (offsets % 16 == 0).all()
    assert [data[o:o + n].numpy().tobytes() for o, n in zip(offsets.tolist(), sizes.tolist())] == want
    assert X.extract_files(flat, boff, bsz, table, device="cpu") == want
    assert X.extract_files(flat, boff, bsz, table, device="cpu", max_bytes=1000) == want  # several batches
    bad = EC.bad_cases()[0]
    flat, boff, bsz = flat_blocks(bad)
    with pytest.raises(RuntimeError, match="^file 2: BAD_CHUNK"):
        X.extract_files(flat, boff, bsz, X.FileTable.from_files(bad.files), device="cpu")
    with pytest.raises(RuntimeError, match="^file 2: BAD_CHUNK"):
        X.extract_files(flat, boff, bsz, X.FileTable.from_files(bad.files), device="cpu", max_bytes=100)


def test_batches_are_cut_at_file_boundaries():
    assert X.batches([10, 20, 30], 1 << 20) == [(0, 3)]
    assert X.batches([], 100) == []
    assert X.batches([16, 16, 16, 16, 16], 32) == [(0, 2), (2, 4), (4, 5)]
    assert X.batches([1, 500, 1, 1, 0], 32) == [(0, 1), (1, 2), (2, 5)]  # a file above max_bytes is alone
    assert X.batches([17, 15], 32) == [(0, 1), (1, 2)]  # (17 bytes take 32 of the buffer)


def test_argument_errors_of_the_abi():
    L = N.lib()
    for name in ("rpp_extract_tile_bytes", "rpp_extract_workspace_bytes", "rpp_extract_gather_batch",
                 "rpp_extract_host_gather"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(L, name)
    assert N.RPP_BAD_CHUNK == -9 and N.STATUS_NAMES[-9] == "BAD_CHUNK" and C.sizeof(N.RppChunk) == 16
    assert X.CHUNK_DTYPE.itemsize == 16 and X.tile_bytes() % 16 == 0 and X.tile_bytes() >= 4096
    blocks = np.frombuffer(EC.block_bytes(1, 100), np.uint8)
    boff, bsz = np.array([0], np.uint64), np.array([100], np.uint64)
    chunks = np.array([(0, 10, 20), (0, 30, 5)], X.CHUNK_DTYPE)
    dst, first = np.array([0, 20, 25], np.uint64), np.array([0, 1, 2], np.uint64)
    out, status = np.zeros(25, np.uint8), np.full(2, 7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def host(first=first, nchunks=2, nfiles=2, chunks=p(chunks), status=p(status)):
        return L.rpp_extract_host_gather(p(blocks), 100, p(boff), p(bsz), 1, chunks, p(dst), nchunks, p(first), nfiles,
                                         p(out), 25, status)

    assert host() == N.RPP_OK and status.tolist() == [0, 0]
    assert out.tobytes() == blocks[10:30].tobytes() + blocks[30:35].tobytes()
    assert host(chunks=None) == host(status=None) == N.RPP_INVALID_ARGUMENT  # a null pointer
    assert host(first=np.array([0, 2, 1], np.uint64)) == N.RPP_INVALID_ARGUMENT  # the file table decreases
    assert host(first=np.array([1, 1, 2], np.uint64)) == N.RPP_INVALID_ARGUMENT  # does not start at 0
    assert host(nchunks=1) == N.RPP_INVALID_ARGUMENT                             # does not end at nchunks
    assert host(nfiles=0) == N.RPP_INVALID_ARGUMENT                              # chunks without a file
    assert L.rpp_extract_host_gather(None, 0, None, None, 0, None, None, 0, None, 0, None, 0, None) == N.RPP_OK
    # the batch call checks its arguments before it touches the device (pointers that are never followed)
    ws_bytes = L.rpp_extract_workspace_bytes(1000, 10, 1 << 20)
    assert ws_bytes >= 1000 and ws_bytes % 16 == 0 and L.rpp_extract_workspace_bytes(0, 0, 0) > 0
    fake = C.c_void_p(0x1000)

    def batch(ws=fake, ws_n=ws_bytes, d_blocks=fake, d_out=fake, d_chunks=fake, nfiles=10, status=fake):
        return L.rpp_extract_gather_batch(d_blocks, 4096, fake, fake, 3, d_chunks, fake, 1000, fake, nfiles, d_out,
                                          1 << 20, status, ws, ws_n, None)

    assert batch(ws_n=ws_bytes - 1) == N.RPP_INVALID_ARGUMENT  # a workspace one byte short
    assert batch(ws=None) == batch(d_chunks=None) == batch(status=None) == N.RPP_INVALID_ARGUMENT
    assert batch(d_blocks=None) == batch(d_out=None) == N.RPP_INVALID_ARGUMENT
    assert batch(nfiles=0) == N.RPP_INVALID_ARGUMENT
    for name in ("ws", "d_blocks", "d_out"):
        assert batch(**{name: C.c_void_p(0x1008)}) == N.RPP_INVALID_ARGUMENT, name  # not on a 16-byte boundary
    assert L.rpp_extract_gather_batch(None, 0, None, None, 0, None, None, 0, None, 0, None, 0, None, None, 0,
                                      None) == N.RPP_OK  # nothing to do


def test_cpp_host_gather_under_asan_ubsan():
    """tests/cpp/extract_test.cpp: the host gather over generated families in a program of its own, built with
    AddressSanitizer and UBSan, with exact-size heap buffers, against a byte-by-byte restatement."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_extract.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "extract_test")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "extract_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
