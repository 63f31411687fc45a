"""GPU tests of the nilsimsa fragment ordering: order_nilsimsa and the two kernels of the order group against the
committed answers of the Python model (tests/golden/order_kat.json), and against the library's host restatement
where the model is too slow.  Everything is an equality: the algorithm is deterministic."""

import base64
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from dwarfs_amd import ordering as O
from dwarfs_amd import similarity as S

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
from make_order_kat import unpack  # noqa: E402

KAT = json.loads((GOLDEN / "order_kat.json").read_text())
for _group in ("order", "split", "chain"):  # id lists are packed in the file
    for _c in KAT[_group]:
        for _key in ("index", "order", "child", "from", "to", "perm"):
            if _c.get(_key) is not None:
                _c[_key] = unpack(_c[_key])
        if _group == "chain" and _c["to"] is None:
            _c["to"] = _c["from"]
FLIPS = (0, 1, 2, 3, 8, 20, 60)


def names(cases):
    return [c["name"] for c in cases]


def case(group, name):
    return next(c for c in KAT[group] if c["name"] == name)


_tables = {}


def table(name):
    if name not in _tables:
        t = KAT["tables"][name]
        bits = np.frombuffer(base64.b64decode(t["digests"]), "<u8").reshape(-1, 4).astype(np.uint64)
        sizes = np.array(t["size_choices"], np.uint64)[np.frombuffer(t["sizes"].encode(), np.uint8) - ord("0")]
        _tables[name] = (bits, sizes, np.array(unpack(t["rank"]), np.uint32))
    return _tables[name]


def families(seed, n):
    """The family mix at size: a random base digest with f random bits flipped per member, f from FLIPS, families
    of 1 .. 400 members so that tight ones outlast several levels; sizes from a few values, a shuffled rank."""
    rng = np.random.default_rng(seed)
    rows = []
    total = 0
    while total < n:
        m = min(int(rng.choice((1, 2, 3, 5, 8, 12, 40, 100, 400))), n - total)
        f = int(rng.choice(FLIPS))
        base = rng.integers(0, 2, 256, dtype=np.uint8)
        member = np.repeat(base[None, :], m, axis=0)
        if f:
            where = np.argsort(rng.random((m, 256)), axis=1)[:, :f]
            np.put_along_axis(member, where, 1 - np.take_along_axis(member, where, axis=1), axis=1)
        rows.append(member)
        total += m
    bits = np.packbits(np.concatenate(rows), axis=1, bitorder="little").view("<u8").astype(np.uint64)
    mix = rng.permutation(n)
    return bits[mix], rng.choice(np.array([1, 4096, 4096, 65536], np.uint64), n), rng.permutation(n).astype(np.uint32)


@pytest.mark.parametrize("name", names(KAT["order"]))
def test_order_equals_model(name):
    c = case("order", name)
    bits, sizes, rank = table(c["table"])
    out = O.order_nilsimsa(bits, sizes, rank, np.array(c["index"], np.uint32), c["max_children"], c["max_cluster_size"])
    assert out.dtype == np.uint32 and out.tolist() == c["order"]


@pytest.mark.parametrize("name", [n for n in names(KAT["order"]) if n.startswith(("max_children", "root_at"))])
def test_root_split_equals_model(name):
    """rpp_order_split_batch alone on the root of a whole-order case: the model's child of every visited element."""
    c = case("order", name)
    bits, sizes, rank = table(c["table"])
    idx = np.array(c["index"], np.uint32)
    b = bits[idx]
    visit = idx[np.lexsort((rank[idx], b[:, 3], b[:, 2], b[:, 1], b[:, 0]))]
    visit = visit[np.concatenate(([True], (bits[visit][1:] != bits[visit][:-1]).any(axis=1)))]
    child, nch = O.split_batch(O.device_bits(bits), visit, [0, visit.size], c["max_children"], 128)
    assert child.tolist() == c["root_child"] and nch.tolist() == [max(c["root_child"]) + 1]


@pytest.mark.parametrize("name", names(KAT["split"]))
def test_split_equals_model(name):
    c = case("split", name)
    bits, _, _ = table(c["table"])
    child, nch = O.split_batch(O.device_bits(bits), c["index"], [0, len(c["index"])], c["max_children"], c["max_distance"])
    assert child.tolist() == c["child"] and nch.tolist() == [c["nchildren"]]


def test_split_nodes_of_one_launch_are_independent():
    """The wide cases as three nodes of one launch, an empty node between them."""
    cs = [case("split", f"wide_B{d:+d}") for d in (-1, 0, 1)]
    bits, _, _ = table("spread")
    index = np.concatenate([cs[0]["index"], cs[1]["index"], cs[2]["index"]]).astype(np.uint32)
    cut = np.cumsum([0, len(cs[0]["index"]), 0, len(cs[1]["index"]), len(cs[2]["index"])])
    child, nch = O.split_batch(O.device_bits(bits), index, cut, 16384, 64)
    assert child.tolist() == cs[0]["child"] + cs[1]["child"] + cs[2]["child"]
    assert nch.tolist() == [cs[0]["nchildren"], 0, cs[1]["nchildren"], cs[2]["nchildren"]]


def test_chains_equal_model():
    """Every chain case (leaf and to != from, lengths around the pass width and the LDS capacity) in one launch,
    and each length class alone."""
    bits_a, _, _ = table("spread")
    bits_b, _, _ = table("chain_edges")
    bits = np.concatenate([bits_a, bits_b])
    d_bits = O.device_bits(bits)
    frm, to, seg, want = [], [], [0], []
    for c in KAT["chain"]:
        shift = bits_a.shape[0] if c["table"] == "chain_edges" else 0
        frm += [i + shift for i in c["from"]]
        to += [i + shift for i in c["to"]]
        seg.append(len(frm))
        want += c["perm"]
    assert O.chain_batch(d_bits, frm, to, seg).tolist() == want
    for c in KAT["chain"]:
        if c["from"] == c["to"] and c["table"] == "spread":
            assert O.chain_batch(d_bits, c["from"], None, [0, len(c["from"])]).tolist() == c["perm"], c["name"]


@pytest.mark.parametrize("options", [(256, 256), (16, 64)])
def test_large_equals_host(options):
    bits, sizes, rank = families(options[0], 20000)
    want, st = O.host_order_nilsimsa(bits, sizes, rank, None, *options, return_stats=True)
    assert st["depth"] >= 4 and st["leaves"] >= 50, st
    got = O.order_nilsimsa(bits, sizes, rank, None, *options)
    assert np.array_equal(got, want)
    if options == (16, 64):  # two calls on the same input: no dependence on scheduling
        assert np.array_equal(O.order_nilsimsa(bits, sizes, rank, None, *options), got)


def test_files_to_order():
    """similarity_hashes -> order_nilsimsa: about 200 small files, edited copies of a few bases."""
    rng = np.random.default_rng(7)
    bases = [rng.integers(0, 256, int(s), dtype=np.uint8) for s in (3000, 5000, 8000, 1200, 6000)]
    files = []
    for i in range(200):
        f = bases[i % len(bases)].copy()
        for _ in range(int(rng.integers(0, 6))):
            at = int(rng.integers(0, f.size - 64))
            f[at:at + int(rng.integers(1, 64))] = rng.integers(0, 256, dtype=np.uint8)
        files.append(f[: f.size - int(rng.integers(0, 200))].tobytes())
    files += files[:5]  # exact duplicates
    h = S.similarity_hashes(files)
    assert h.has.all()
    assert h.digests[3].tobytes() == S.host_hash(files[3])
    sizes = np.array([len(f) for f in files], np.uint64)
    rank = rng.permutation(len(files)).astype(np.uint32)
    got = O.order_nilsimsa(h.digests, sizes, rank, None, 4, 8)
    assert np.array_equal(got, O.host_order_nilsimsa(h.digests, sizes, rank, None, 4, 8))
    assert sorted(got.tolist()) == list(range(len(files)))
    assert O.total_distance(h.digests, got) <= O.total_distance(h.digests, np.arange(len(files)))
    assert np.array_equal(O.order_nilsimsa(h.digests, sizes, rank, None, 4, 8), got)
