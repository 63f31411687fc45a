"""CPU tests of the similarity group of the C ABI: exported symbols, kind names and sizes, argument checks, and
the host restatement (rpp_similarity_host_update / _finalize) against tests/golden/similarity_kat.json -- the
reference's recorded nilsimsa answers and the pure-Python model of tests/golden/make_similarity_kat.py."""

import ctypes as C
import itertools
import json
import struct
import sys
from pathlib import Path

import pytest

from dwarfs_amd import _native as N
from dwarfs_amd import similarity as S

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_similarity_kat as SK  # noqa: E402

NEW_SYMBOLS = ("rpp_similarity_kind", "rpp_similarity_state_bytes", "rpp_similarity_digest_bytes",
               "rpp_similarity_chunk_bytes", "rpp_similarity_update_batch", "rpp_similarity_finalize_batch",
               "rpp_similarity_hash_workspace_bytes", "rpp_similarity_hash_batch", "rpp_similarity_host_update",
               "rpp_similarity_host_finalize")
KINDS = ("nilsimsa", "similarity")


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "similarity_kat.json").read_text())


def _model(kind):
    return SK.Nilsimsa() if kind == "nilsimsa" else SK.Similarity()


def _model_raw(m) -> bytes:
    """A model's state in the layout of include/ricepp_amd.h."""
    if isinstance(m, SK.Nilsimsa):
        w1, w2, w3, w4 = m.w
        return struct.pack("<256QQ4B4x", *m.acc, m.size, w4, w3, w2, w1)
    return struct.pack("<256II4xQ", *m.acc, m.val, m.size)


def test_library_exports_new_symbols():
    raw = C.CDLL(str(N.LIB_PATH))
    header = (Path(__file__).resolve().parent.parent / "include" / "ricepp_amd.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in N.EXPORTED_SYMBOLS
        assert name + "(" in header, name
    assert N.lib().rpp_abi_version() == 1


def test_kind_names_and_sizes():
    L = N.lib()
    assert L.rpp_similarity_kind(b"nilsimsa") == N.RPP_SIMILARITY_NILSIMSA == 0
    assert L.rpp_similarity_kind(b"similarity") == N.RPP_SIMILARITY_HISTOGRAM == 1
    for bad in (b"", b"Nilsimsa", b"nilsimsa ", b"xxh3-128", b"none"):
        assert L.rpp_similarity_kind(bad) < 0, bad
    assert L.rpp_similarity_kind(None) < 0
    assert [L.rpp_similarity_digest_bytes(k) for k in (0, 1, 2, -1)] == [32, 4, 0, 0]
    # 256 x uint64 + size + 4 window bytes + padding; 256 x uint32 + val + padding + uint64 size
    assert [L.rpp_similarity_state_bytes(k) for k in (0, 1, 2, -1)] == [256 * 8 + 8 + 8, 256 * 4 + 8 + 8, 0, 0]
    c = L.rpp_similarity_chunk_bytes()
    assert c == S.chunk_bytes() and 4096 <= c and 8 * c < 2**32  # a workgroup's uint32 counters cannot overflow
    for k in (0, 1):
        assert L.rpp_similarity_hash_workspace_bytes(k, 0) == 0
        assert L.rpp_similarity_hash_workspace_bytes(k, 1000) >= 1000 * L.rpp_similarity_state_bytes(k)


def test_unknown_kind_raises_value_error():
    with pytest.raises(ValueError, match="md5"):
        S._kind("md5")
    with pytest.raises(ValueError, match="md5"):
        S.host_hash(b"abc", "md5")
    assert S._kind("nilsimsa") == (0, 32, 2064) and S._kind("similarity") == (1, 4, 1040)


def test_argument_checks_without_gpu():
    L, null = N.lib(), C.c_void_p(0)
    big = 1 << 40
    for k in (0, 1):
        # empty batches
        assert L.rpp_similarity_update_batch(k, null, null, null, null, 0, null, null) == N.RPP_OK
        assert L.rpp_similarity_finalize_batch(k, null, null, 0, null, null) == N.RPP_OK
        assert L.rpp_similarity_hash_batch(k, null, null, null, null, 0, 0, null, null, null, 0, null) == N.RPP_OK
        # null pointers with work to do are refused before anything is launched
        assert L.rpp_similarity_update_batch(k, null, null, null, null, 1, null, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_finalize_batch(k, null, null, 1, null, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_hash_batch(k, null, null, null, null, 0, 1, null, null, null, big,
                                           null) == N.RPP_INVALID_ARGUMENT
        # a workspace that is too small (host memory stands in for the pointers: nothing is launched)
        buf = (C.c_uint64 * 64)()
        p = C.cast(buf, C.c_void_p)
        need = L.rpp_similarity_hash_workspace_bytes(k, 8)
        assert L.rpp_similarity_hash_batch(k, p, p, p, null, 0, 8, p, p, p, need - 1, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_host_update(k, null, p, 1) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_host_update(k, p, null, 1) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_host_finalize(k, null, p) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_host_finalize(k, p, null) == N.RPP_INVALID_ARGUMENT
    # an unknown kind, with or without work
    for k in (2, -1):
        assert L.rpp_similarity_update_batch(k, null, null, null, null, 0, null, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_finalize_batch(k, null, null, 0, null, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_hash_batch(k, null, null, null, null, 0, 0, null, null, null, 0,
                                           null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_similarity_host_update(k, null, null, 0) == N.RPP_INVALID_ARGUMENT


def test_transition_table():
    assert sorted(SK.T) == list(range(256))
    assert SK.T[:4] == [0x02, 0xD6, 0x9E, 0x6F] and SK.T[-2:] == [0x72, 0x4E]


def test_reference_vectors(kat):
    """test/nilsimsa_test.cpp: empty, abcdefgh, the 26 prefixes of the alphabet."""
    ref = kat["nilsimsa_reference"]
    assert S.HostState("nilsimsa").hexdigest() == ref["empty"] == "00" * 32
    assert S.HostState("nilsimsa").update(b"abcdefgh").hexdigest() == ref["abcdefgh"]
    assert len(ref["alphabet_prefixes"]) == 26
    for i, want in enumerate(ref["alphabet_prefixes"]):
        assert S.HostState("nilsimsa").update(ref["alphabet"][:i + 1].encode()).hexdigest() == want, i
    assert S.host_hash(b"", "similarity") == bytes([3, 2, 1, 0])  # 0x00010203
    assert S.HostState("similarity").hexdigest() == "00010203"


def test_reference_incremental(kat):
    """"a","bc","defgh", digest, then "i","jk", digest again: finalize leaves the state usable."""
    h = S.HostState("nilsimsa")
    for step in kat["nilsimsa_reference"]["incremental"]:
        for piece in step["pieces"]:
            h.update(piece.encode())
        before = h.raw()
        assert h.hexdigest() == step["hexdigest"]
        assert h.raw() == before
    assert [s["pieces"] for s in kat["nilsimsa_reference"]["incremental"]] == [["a", "bc", "defgh"], ["i", "jk"]]


def test_kat_messages(kat):
    """Every synthetic message: digests and raw states equal the Python model's."""
    assert len(kat["messages"]) >= 39
    for m in kat["messages"]:
        data = SK.message_bytes(m)
        for kind in KINDS:
            h = S.HostState(kind).update(data)
            assert h.hexdigest() == m[kind], (kind, m)
            if m["length"] <= 4097:
                assert h.raw() == _model_raw(_model(kind).update(data)), (kind, m)


def test_every_split_of_nine_bytes():
    """Every 2- and 3-way split of a 9-byte message (all splits inside the first 4 bytes among them) gives the
    one-shot state, byte for byte."""
    msg = bytes([0x61, 0x00, 0xFF, 0x62, 0x63, 0x7F, 0x80, 0x01, 0x64])
    for kind in KINDS:
        whole = S.HostState(kind).update(msg).raw()
        assert whole == _model_raw(_model(kind).update(msg))
        for i, j in itertools.combinations_with_replacement(range(10), 2):
            h = S.HostState(kind).update(msg[:i]).update(msg[i:j]).update(msg[j:])
            assert h.raw() == whole, (kind, i, j)


def test_total_and_threshold_rule():
    """total = 1, 4, 8 * size - 28 at sizes 3, 4, 5; threshold = total / 256; bit i = acc[i] > threshold."""
    for size, total in ((3, 1), (4, 4), (5, 12), (40, 292), (100, 772)):
        assert total == (1 if size == 3 else 4 if size == 4 else 8 * size - 28)
        threshold = total // 256
        acc = [0] * 256
        acc[7], acc[8], acc[255] = threshold, threshold + 1, threshold + 2
        raw = struct.pack("<256QQ4B4x", *acc, size, 0, 0, 0, 0)
        digest = S.HostState("nilsimsa", raw).digest()
        want = bytearray(32)
        for i in (8, 255):
            want[i >> 3] |= 1 << (i & 7)
        if threshold == 0:
            assert acc[7] == 0
        assert digest == bytes(want), size
    # sizes 3, 4, 5 from real bytes: every incremented bucket is above a threshold of 0
    for size, total in ((3, 1), (4, 4), (5, 12)):
        m = SK.Nilsimsa().update(b"abcde"[:size])
        assert sum(m.acc) == total == m.total()
        assert S.host_hash(b"abcde"[:size], "nilsimsa") == m.digest()
        assert sum(bin(b).count("1") for b in m.digest()) == sum(1 for c in m.acc if c)


def test_similarity_ties_and_wrap():
    """The four highest counts, ties to the lower index; counters are uint32 and wrap."""
    acc = [0] * 256
    acc[200], acc[17], acc[18], acc[3] = 9, 5, 5, 1
    raw = struct.pack("<256II4xQ", *acc, 0, 100)
    assert S.HostState("similarity", raw).hexdigest() == "c8111203"
    acc = [0xFFFFFFFF] * 256
    h = S.HostState("similarity", struct.pack("<256II4xQ", *acc, 0, 100)).update(b"wxyz")
    m = SK.Similarity()
    m.acc, m.size = list(acc), 100
    assert h.raw() == _model_raw(m.update(b"wxyz"))
    counts = struct.unpack_from("<256I", h.raw())
    assert min(counts) < 4 and sum(1 for c in counts if c != 0xFFFFFFFF) in (1, 2, 3, 4)


def test_kat_regenerates(kat):
    """tests/golden/similarity_kat.json is what make_similarity_kat.py writes."""
    assert SK.build() == kat
