"""GPU tests of the similarity hashes (rpp_similarity_update_batch ... rpp_similarity_hash_batch and their Python /
C++ layers).  Every comparison is for equality, and of raw states (counters, window, size) with the host
restatement's, not only of digests: a counter off by one rarely flips a thresholded bit.  Digests are also
compared with tests/golden/similarity_kat.json (the reference's recorded nilsimsa answers and the pure-Python
model)."""

import json
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from dwarfs_amd import similarity as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_similarity_kat as SK  # noqa: E402

DEV = "cuda"
KINDS = ("nilsimsa", "similarity")


def _lengths():
    c = S.chunk_bytes()
    return [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, c - 1, c, c + 1, 2 * c + 3]


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "similarity_kat.json").read_text())


def _fill(kind: str, n: int, i: int, rng) -> bytes:
    """File i of a data kind; neighbours differ, so a byte leaked from one shows in the other's counters."""
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "zero":
        return bytes([0x00 if i % 2 == 0 else 0x5A]) * n
    pair = b"\xa5\x3c" if i % 2 == 0 else b"\x11\xee"
    return (pair * (n // 2 + 1))[:n]


def _pack(files, lead: int = 0):
    """The files back to back behind `lead` bytes of filler: (device bytes, offsets, sizes)."""
    sizes = np.array([len(f) for f in files], dtype=np.int64)
    offsets = lead + np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.int64)
    blob = b"\xc3" * lead + b"".join(files) + b"\x3c" * 16
    return torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(DEV), offsets, sizes


def _host_states(files, kind, start=None) -> np.ndarray:
    rows = [S.HostState(kind, None if start is None else start[i]).update(f).raw() for i, f in enumerate(files)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(files), -1)


def _assert_states_equal(got: np.ndarray, want: np.ndarray, what):
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{what}: states differ for entries {bad[:20]} ({len(bad)} of {len(want)})")


def test_kat_digests_one_batch(kat):
    """Every KAT message and every reference vector, both kinds, each in one batch."""
    ref = kat["nilsimsa_reference"]
    texts = [b"", b"abcdefgh", b"abcdefghijk"] + [ref["alphabet"][:i + 1].encode() for i in range(26)]
    want_texts = [ref["empty"], ref["abcdefgh"], ref["incremental"][1]["hexdigest"]] + ref["alphabet_prefixes"]
    files = texts + [SK.message_bytes(m) for m in kat["messages"]]
    got = S.similarity_hashes(files, "nilsimsa")
    assert got.has.tolist() == [1] * len(files)
    assert [got.hexdigest(i) for i in range(len(texts))] == want_texts
    assert [got.hexdigest(len(texts) + i) for i in range(len(kat["messages"]))] == [m["nilsimsa"] for m in kat["messages"]]
    got = S.similarity_hashes(files, "similarity")
    assert [got.hexdigest(len(texts) + i) for i in range(len(kat["messages"]))] == [m["similarity"] for m in kat["messages"]]
    assert got.value(0) == 0x00010203 and got.hexdigest(0) == "00010203"
    assert [got.digests[i].tobytes() for i in range(len(files))] == S.host_hashes(files, "similarity")


@pytest.mark.parametrize("data_kind", ["random", "zero", "period2"])
def test_lengths_at_every_misalignment(data_kind):
    """Every length of _lengths() starting at every offset modulo 16, files back to back (16 groups, group a behind
    a bytes of filler at a 16-aligned place), in one batch of more than 256 files."""
    rng = np.random.default_rng(11)
    LENGTHS = _lengths()
    files, starts, at = [], [], 0
    for a in range(16):
        at = (at + 15) // 16 * 16 + a
        for n in LENGTHS:
            files.append(_fill(data_kind, n, len(files), rng))
            starts.append(at)
            at += n
    blob = bytearray(b"\xc3" * (at + 16))
    for o, f in zip(starts, files):
        blob[o:o + len(f)] = f
    assert {(o % 16, len(f)) for o, f in zip(starts, files)} == {(a, n) for a in range(16) for n in LENGTHS}
    data = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(DEV)
    sizes = [len(f) for f in files]
    for kind in KINDS:
        st = S.update(S.SimilarityState.new(len(files), kind, DEV), data, starts, sizes)
        digests = S.finalize(st).cpu().numpy()
        _assert_states_equal(st.cpu(), _host_states(files, kind), (data_kind, kind))
        assert [d.tobytes() for d in digests] == S.host_hashes(files, kind)


def test_incremental_two_states():
    """Two states fed by five calls: pieces that end inside the first 4 bytes, pieces of C, C - 1 and C + 1
    bytes, an empty piece; a finalize between two updates leaves the states unchanged; the result equals the
    one-shot states."""
    rng = np.random.default_rng(12)
    C = S.chunk_bytes()
    pieces = [[1, 2, C, C - 1, 40], [3, 0, C + 1, 1, C]]
    msgs = [rng.integers(0, 256, sum(p), dtype=np.uint8).tobytes() for p in pieces]
    data, offsets, sizes = _pack(msgs, lead=5)
    for kind in KINDS:
        st = S.SimilarityState.new(2, kind, DEV)
        host = [S.HostState(kind), S.HostState(kind)]
        done = [0, 0]
        for call in range(5):
            sz = [pieces[0][call], pieces[1][call]]
            S.update(st, data, [int(offsets[i]) + done[i] for i in range(2)], sz)
            for i in range(2):
                host[i].update(msgs[i][done[i]:done[i] + sz[i]])
                done[i] += sz[i]
            before = st.cpu().copy()
            digests = S.finalize(st).cpu().numpy()
            assert st.cpu().tobytes() == before.tobytes(), (kind, call)
            want = np.frombuffer(host[0].raw() + host[1].raw(), np.uint8).reshape(2, -1)
            _assert_states_equal(before, want, (kind, call))
            assert [d.tobytes() for d in digests] == [h.digest() for h in host], (kind, call)
        one_shot = S.update(S.SimilarityState.new(2, kind, DEV), data, offsets, sizes)
        assert one_shot.cpu().tobytes() == st.cpu().tobytes()


def test_select_and_max_size():
    """Skipped rows keep a sentinel and get has = 0; a file of exactly max_size is hashed, one byte more is not."""
    rng = np.random.default_rng(13)
    lengths = [10, 100, 101, 0, 5000, 100, 99]
    select = [1, 1, 1, 0, 1, 0, 1]
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]
    data, offsets, sizes = _pack(files, lead=3)
    for kind in KINDS:
        want = S.host_hashes(files, kind)
        out = S.DeviceSimilarity.new(len(files), kind, DEV)
        out.digests.fill_(0xAB)
        out.has.fill_(7)
        digests, has = S.similarity_hash_batch(data, offsets, sizes, kind, max_size=100, select=select, out=out)
        assert has.cpu().tolist() == [1, 1, 0, 0, 0, 0, 1]
        rows = [d.tobytes() for d in digests.cpu().numpy()]
        sentinel = b"\xab" * len(want[0])
        assert rows == [want[0], want[1], sentinel, sentinel, sentinel, sentinel, want[6]]
        # no max_size, no select: everything is hashed
        digests, has = S.similarity_hash_batch(data, offsets, sizes, kind)
        assert has.cpu().tolist() == [1] * len(files)
        assert [d.tobytes() for d in digests.cpu().numpy()] == want
        # update honours select as well: unselected states stay as they were
        st = S.update(S.SimilarityState.new(len(files), kind, DEV), data, offsets, sizes, select=select)
        got = st.cpu()
        host = _host_states(files, kind)
        for i, s in enumerate(select):
            assert got[i].tobytes() == (host[i].tobytes() if s else bytes(host.shape[1])), (kind, i)


def test_counter_carry():
    """States whose counters are preloaded to 2^32 - 1 (both kinds: nilsimsa's 64-bit carry, similarity's wrap)
    and to 2^63 (nilsimsa), updated with 64 bytes: equal to the host update from the same states."""
    rng = np.random.default_rng(14)
    msgs = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), bytes(64)]
    data, offsets, sizes = _pack(msgs, lead=1)
    start = {
        "nilsimsa": [struct.pack("<256QQ4B4x", *([v] * 256), 1000, 1, 2, 3, 4) for v in (2**32 - 1, 2**63)],
        "similarity": [struct.pack("<256II4xQ", *([2**32 - 1] * 256), 0x01020304, 1000)] * 2,
    }
    for kind in KINDS:
        raw = np.frombuffer(b"".join(start[kind]), np.uint8).reshape(2, -1)
        st = S.update(S.SimilarityState.from_host(raw, kind, DEV), data, offsets, sizes)
        _assert_states_equal(st.cpu(), _host_states(msgs, kind, start[kind]), kind)
    nil = S.HostState("nilsimsa", start["nilsimsa"][0]).update(msgs[0]).raw()
    assert max(struct.unpack_from("<256Q", nil)) >= 2**32  # (the carry did happen)


@pytest.mark.parametrize("data_kind", ["random", "zero"])
def test_lone_large_file(data_kind):
    """One file of 4 MiB + 5 bytes alone in its batch: many chunks of one message on many workgroups.  The state
    equals the host's, and two runs give byte-identical states."""
    n = 4 * 2**20 + 5
    blob = _fill(data_kind, n, 0, np.random.default_rng(15))
    data, offsets, sizes = _pack([blob], lead=7)
    for kind in KINDS:
        runs = [S.update(S.SimilarityState.new(1, kind, DEV), data, offsets, sizes).cpu() for _ in range(2)]
        assert runs[0].tobytes() == runs[1].tobytes()
        _assert_states_equal(runs[0], _host_states([blob], kind), (data_kind, kind))


def test_hash_batch_graph_capture(kat):
    """One rpp_similarity_hash_batch call captured in a graph on a side stream and replayed twice."""
    files = [SK.message_bytes(m) for m in kat["messages"]]
    host, offsets, sizes = S.pack_files(files)
    data = torch.from_numpy(host).to(DEV)
    d_off, d_sz = torch.from_numpy(offsets).to(DEV), torch.from_numpy(sizes).to(DEV)
    for kind in KINDS:
        out = S.DeviceSimilarity.new(len(files), kind, DEV)
        S.similarity_hash_batch(data, d_off, d_sz, kind, out=out)  # (warm-up outside the capture)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                S.similarity_hash_batch(data, d_off, d_sz, kind, out=out)
        results = []
        for _ in range(2):
            out.digests.zero_()
            out.has.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            results.append((out.digests.cpu().numpy().copy(), out.has.cpu().tolist()))
        assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1] == results[1][1] == [1] * len(files)
        assert [S.hexdigest(d, kind) for d in results[1][0]] == [m[kind] for m in kat["messages"]]


def test_cpp_similarity(kat, tmp_path):
    """tests/cpp/similarity_test: ricepp_amd::similarity_hashes on the KAT messages, given as a file of the
    files' bytes and a table `size nilsimsa similarity` per file."""
    exe = ROOT / "tests" / "cpp" / "build" / "similarity_test"
    if not exe.exists():
        subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_similarity.sh")], check=True)
    files = [SK.message_bytes(m) for m in kat["messages"]]
    (tmp_path / "files.bin").write_bytes(b"".join(files))
    (tmp_path / "table.txt").write_text("".join(
        f"{m['length']} {m['nilsimsa']} {m['similarity']}\n" for m in kat["messages"]))
    r = subprocess.run([str(exe), str(tmp_path / "files.bin"), str(tmp_path / "table.txt")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "similarity_test: OK" in r.stdout
