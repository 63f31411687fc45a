"""CPU tests of the nilsimsa fragment ordering (no GPU needed): the order group's host-side entry points, and the
host restatement (rpp_order_host_nilsimsa / _split / _chain: the reference's sequential loops) against
tests/golden/order_kat.json -- the answers of the pure-Python model tests/golden/make_order_kat.py."""

import base64
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from dwarfs_amd import _native as N
from dwarfs_amd import ordering as O
from dwarfs_amd import similarity as S
from dwarfs_amd.codec import UnsupportedConfiguration

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_order_kat as K  # noqa: E402

NEW_SYMBOLS = ("rpp_order_check_options", "rpp_order_split_pass_children", "rpp_order_chain_threads",
               "rpp_order_chain_stage_rows", "rpp_order_split_workspace_bytes", "rpp_order_split_batch",
               "rpp_order_chain_workspace_bytes", "rpp_order_chain_batch", "rpp_order_host_split",
               "rpp_order_host_chain", "rpp_order_host_nilsimsa")


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "order_kat.json").read_text())


def table(kat, name):
    t = kat["tables"][name]
    bits = np.frombuffer(base64.b64decode(t["digests"]), "<u8").reshape(-1, 4).astype(np.uint64)
    sizes = np.array(t["size_choices"], dtype=np.uint64)[np.frombuffer(t["sizes"].encode(), np.uint8) - ord("0")]
    return bits, sizes, np.array(K.unpack(t["rank"]), dtype=np.uint32)


def names(cases):
    return [c["name"] for c in cases]


KAT = json.loads((GOLDEN / "order_kat.json").read_text()) if (GOLDEN / "order_kat.json").exists() else {}


def test_kat_file_is_current(kat):
    """The committed file -- inputs, permutations and statistics -- is what the model writes; the model's own
    conditions (fallbacks and ties, depth 8 with an oversized final leaf, B - 1 / B / B + 1 children) run here."""
    assert json.loads(json.dumps(K.build())) == kat
    assert (GOLDEN / "order_kat.json").stat().st_size < 512 * 1024
    assert max(len(K.unpack(c["index"])) for c in kat["order"]) <= 2000
    assert K.unpack(K.pack([5, 6, 7, 8, 2, 3, 9, 10, 11, 12, 13])) == [5, 6, 7, 8, 2, 3, 9, 10, 11, 12, 13]


def test_symbols_options_and_sizes(kat):
    L = N.lib()
    for name in NEW_SYMBOLS:
        assert name in N.EXPORTED_SYMBOLS and hasattr(L, name)
    assert C.sizeof(N.RppOrderStats) == 56
    assert L.rpp_order_check_options(1, 1) == N.RPP_OK
    assert L.rpp_order_check_options(0, 1) == N.RPP_UNSUPPORTED_CONFIG
    assert L.rpp_order_check_options(1, 0) == N.RPP_UNSUPPORTED_CONFIG
    for bad in ((0, 16), (16, 0)):
        with pytest.raises(UnsupportedConfiguration):
            O.host_order_nilsimsa(np.zeros((2, 32), np.uint8), [1, 1], max_children=bad[0], max_cluster_size=bad[1])
    B, T, S_ = O.pass_children(), O.chain_threads(), O.chain_stage_rows()
    assert B % 64 == 0 and T % 64 == 0 and S_ > T
    # the sizes around B, T and the LDS capacity in the committed file were built for these kernels
    assert kat["params"] == {"split_pass_children": B, "chain_threads": T, "chain_stage_rows": S_}
    assert L.rpp_order_split_workspace_bytes(0) == 0 and L.rpp_order_chain_workspace_bytes(10**6) == 0
    assert L.rpp_order_split_workspace_bytes(1000) >= 1000 * (32 + 256 * 4 + 4)
    # device entry points check their arguments before they touch the device
    assert L.rpp_order_split_batch(None, 0, None, None, None, 1, 1, 0, 128, None, None, None, 0, None) == \
        N.RPP_UNSUPPORTED_CONFIG
    assert L.rpp_order_split_batch(None, 0, None, None, None, 1, 1, 4, 128, None, None, None, 0, None) == \
        N.RPP_INVALID_ARGUMENT
    assert L.rpp_order_chain_batch(None, 0, None, None, None, 1, None, None) == N.RPP_INVALID_ARGUMENT
    assert L.rpp_order_split_batch(None, 0, None, None, None, 0, 0, 4, 128, None, None, None, 0, None) == N.RPP_OK
    with pytest.raises(ValueError):
        O.host_order_nilsimsa(np.zeros((2, 32), np.uint8), [1, 1], index=[0, 0])
    with pytest.raises(ValueError):
        O.host_order_nilsimsa(np.zeros((2, 32), np.uint8), [1, 1], index=[2])


def test_word_order_is_the_reference_array():
    """A digest row read as four little-endian words is the reference's array: its hexdigest prints w3 first."""
    d = S.host_hash(b"abcdefgh")
    w = O.as_words(np.frombuffer(d, np.uint8))[0]
    assert "".join(f"{int(x):016x}" for x in w[::-1]) == S.hexdigest(np.frombuffer(d, np.uint8))
    assert S.hexdigest(np.frombuffer(d, np.uint8)) == "14c8118000000000030800000004042004189020001308014088003280000078"


@pytest.mark.parametrize("name", names(KAT.get("order", [])))
def test_host_order_equals_model(kat, name):
    c = next(c for c in kat["order"] if c["name"] == name)
    bits, sizes, rank = table(kat, c["table"])
    index = K.unpack(c["index"])
    out, st = O.host_order_nilsimsa(bits, sizes, rank, np.array(index, dtype=np.uint32), c["max_children"],
                                    c["max_cluster_size"], return_stats=True)
    assert out.tolist() == K.unpack(c["order"])
    assert st == c["stats"]
    before, after = c["total_distance"]
    assert O.total_distance(bits, index) == before and O.total_distance(bits, out) == after


@pytest.mark.parametrize("name", names(KAT.get("split", [])))
def test_host_split_equals_model(kat, name):
    c = next(c for c in kat["split"] if c["name"] == name)
    bits, _, _ = table(kat, c["table"])
    child, nch = O.host_split(bits, K.unpack(c["index"]), c["max_children"], c["max_distance"])
    assert child.tolist() == K.unpack(c["child"]) and nch == c["nchildren"]


@pytest.mark.parametrize("name", names(KAT.get("chain", [])))
def test_host_chain_equals_model(kat, name):
    c = next(c for c in kat["chain"] if c["name"] == name)
    bits, _, _ = table(kat, c["table"])
    to = None if c["to"] is None else K.unpack(c["to"])
    assert O.host_chain(bits, K.unpack(c["from"]), to).tolist() == K.unpack(c["perm"])


def test_rank_none_is_identity_and_subset_ignores_the_rest(kat):
    bits, sizes, _ = table(kat, "mix")
    n = bits.shape[0]
    a = O.host_order_nilsimsa(bits, sizes)
    b = O.host_order_nilsimsa(bits, sizes, np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    assert a.tolist() == b.tolist() and sorted(a.tolist()) == list(range(n))
    idx = np.arange(0, n, 3, dtype=np.uint32)
    other = bits.copy()
    other[1::3] ^= np.uint64(0x5555)  # elements outside the index do not matter
    assert O.host_order_nilsimsa(bits, sizes, None, idx).tolist() == O.host_order_nilsimsa(other, sizes, None, idx).tolist()
