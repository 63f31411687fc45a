"""GPU tests of duplicate-file detection (rpp_xxh3_128_batch ... rpp_file_dedup_batch and their Python / C++
layers).  Every comparison is for equality: digests against tests/golden/filehash_kat.json (XXH3-128 from the
xxhash module, in DwarFS's byte order) and section_kat.json (XXH3-64, SHA-512/256); grouping against a Python
dict; the scanner's decision against dwarfs_amd.dedup.scanner_model."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from dwarfs_amd import _native as N
from dwarfs_amd import dedup as D
from dwarfs_amd import section as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_filehash_kat as FK  # noqa: E402
import make_section_kat as K  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "filehash_kat.json").read_text())


@pytest.fixture(scope="module")
def section_kat():
    return json.loads((GOLDEN / "section_kat.json").read_text())


@pytest.fixture(scope="module")
def messages(kat):
    """The synthetic messages' bytes, regenerated once."""
    return [K.message_bytes(m) for m in kat["messages"]]


@pytest.fixture(scope="module")
def scenario(kat):
    """The dedup scenario's files, regenerated once, with the model's decision."""
    files = [FK.dedup_file_bytes(s) for s in kat["dedup_files"]]
    first, hashed = D.scanner_model(files)
    return files, first, hashed


def _rows(hexes, width):
    return np.frombuffer(bytes.fromhex("".join(hexes)), np.uint8).reshape(-1, width)


def _split(s, width):
    return [s[i:i + width] for i in range(0, len(s), width)]


def _place(chunks, misalign, spare=16):
    """Chunks laid into one buffer, chunk i starting at a 16-byte boundary + misalign(i); returns the buffer
    (with `spare` bytes behind the last chunk) and the offsets."""
    offs, at = [], 0
    for i, c in enumerate(chunks):
        at = (at + 15) // 16 * 16 + misalign(i)
        offs.append(at)
        at += len(c)
    buf = np.zeros(at + spare, np.uint8)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = np.frombuffer(c, np.uint8)
    return buf, offs


def _bad_rows(got, want):
    return np.nonzero((got != want).any(axis=1))[0]


def test_xxh3_128_all_lengths_one_batch(kat, messages):
    buf, offs = _place(messages, lambda i: (5 * i) % 16)
    d = torch.from_numpy(buf).to(DEV)
    sizes = [len(m) for m in messages]
    assert len(sizes) == 320
    got = S.xxh3_128_batch(d, offs, sizes).cpu().numpy()
    want = _rows([m["xxh3_128"] for m in kat["messages"]], 16)
    bad = _bad_rows(got, want)
    assert len(bad) == 0, [(sizes[i], got[i].tobytes().hex(), kat["messages"][i]["xxh3_128"]) for i in bad[:8]]


def test_xxh3_128_prefixes_and_payload_misalignments(kat, messages):
    """Every message behind prefixes of 0, 1, 16, 24, 47 and 64 bytes, its payload at each misalignment 0..15,
    in one batch; against the stored digests of the concatenations."""
    n = len(messages)
    plens = kat["prefix_lengths"]
    assert plens == [0, 1, 16, 24, 47, 64]
    copies = [m for mis in range(16) for m in messages]
    buf, offs = _place(copies, lambda i: i // n)
    d = torch.from_numpy(buf).to(DEV)
    rows = np.stack([np.frombuffer(K.prefix_bytes(i), np.uint8) for i in range(n)])
    m_off, m_size, m_row, m_plen, want = [], [], [], [], []
    for p in plens:
        w = _split(kat["prefixed"][str(p)]["xxh3_128"], 32)
        for mis in range(16):
            for i in range(n):
                assert offs[mis * n + i] % 16 == mis
                m_off.append(offs[mis * n + i])
                m_size.append(len(messages[i]))
                m_row.append(i)
                m_plen.append(p)
                want.append(w[i])
    d_rows = torch.from_numpy(rows[np.array(m_row)]).to(DEV)
    d_plen = torch.tensor(m_plen, dtype=torch.int32, device=DEV)
    got = S.xxh3_128_batch(d, m_off, m_size, d_rows, d_plen).cpu().numpy()
    bad = _bad_rows(got, _rows(want, 16))
    assert len(bad) == 0, [(m_plen[i], m_off[i] % 16, m_size[i]) for i in bad[:8]]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_xxh3_128_small_batches(kat, messages, n):
    """Few messages: the lane-per-message kernel spreads them over waves; short and long ones mixed."""
    pick = [(37 * k + 11) % 320 for k in range(n)]
    pick[0] = 318 if n > 1 else 250  # (a long message in every batch)
    buf, offs = _place([messages[i] for i in pick], lambda i: (3 * i + 1) % 16)
    got = S.xxh3_128_batch(torch.from_numpy(buf).to(DEV), offs, [len(messages[i]) for i in pick]).cpu().numpy()
    want = _rows([kat["messages"][i]["xxh3_128"] for i in pick], 16)
    bad = _bad_rows(got, want)
    assert len(bad) == 0, [(pick[i], len(messages[pick[i]])) for i in bad[:8]]


def test_three_algorithms(kat, section_kat, messages):
    buf, offs = _place(messages, lambda i: (7 * i + 2) % 16)
    d = torch.from_numpy(buf).to(DEV)
    sizes = [len(m) for m in messages]
    want = {
        "xxh3-128": _rows([m["xxh3_128"] for m in kat["messages"]], 16),
        # (stored as the 64-bit value in hex; DwarFS's digest is its 8 little-endian bytes)
        "xxh3-64": np.array([int(m["xxh3_64"], 16) for m in section_kat["messages"]], "<u8").view(np.uint8).reshape(-1, 8),
        "sha512-256": _rows([m["sha512_256"] for m in section_kat["messages"]], 32),
    }
    for algo, rows in want.items():
        got = D.file_hash_batch(d, offs, sizes, algo)
        assert tuple(got.shape) == rows.shape
        bad = _bad_rows(got.cpu().numpy(), rows)
        assert len(bad) == 0, (algo, [sizes[i] for i in bad[:8]])
    hello = kat["hello"]["text"].encode()
    d = torch.from_numpy(np.frombuffer(hello, np.uint8).copy()).to(DEV)
    got = D.file_hash_batch(d, [0], [len(hello)])  # (the default algorithm is the writer's: xxh3-128)
    assert got.cpu().numpy().tobytes().hex().upper() == "9553D72C8403DB7750DD474484F21D53"
    with pytest.raises(ValueError, match="md5"):
        D.file_hash_batch(d, [0], [len(hello)], "md5")
    with pytest.raises(ValueError, match="crc32"):
        D.find_duplicates([b"a"], "crc32")


@pytest.mark.parametrize("algo", ["xxh3-64", "xxh3-128", "sha512-256"])
def test_select_mask(kat, section_kat, messages, algo):
    """Unselected messages keep the sentinel; the buffer ends exactly where the last selected message ends, at
    the end of its allocation."""
    key = {"xxh3-64": "xxh3_64", "xxh3-128": "xxh3_128", "sha512-256": "sha512_256"}[algo]
    src = kat if algo == "xxh3-128" else section_kat
    width = len(src["messages"][0][key]) // 2
    last = 316  # 65537 bytes: a long message that ends on the allocation's last byte
    order = [i for i in range(320) if i != last] + [last]
    assert len(messages[last]) == 65537
    buf, offs = _place([messages[i] for i in order], lambda i: (5 * i) % 16, spare=0)
    assert offs[-1] + len(messages[last]) == len(buf)
    d = torch.from_numpy(buf).to(DEV)
    sizes = [len(messages[i]) for i in order]
    select = np.array([1 if (k % 3 != 1 or k == len(order) - 1) else 0 for k in range(len(order))], np.uint8)
    out = torch.full((len(order), width), 0xA5, dtype=torch.uint8, device=DEV)
    got = D.file_hash_batch(d, offs, sizes, algo, select=select, out=out).cpu().numpy()
    for k, i in enumerate(order):
        h = src["messages"][i][key]
        if select[k]:
            want = bytes.fromhex(h)[::-1] if algo == "xxh3-64" else bytes.fromhex(h)
            assert got[k].tobytes() == want, (k, i)
        else:
            assert got[k].tobytes() == b"\xa5" * width, (k, i)


def _dict_first(keys, select=None):
    seen, first, count = {}, [], {}
    for b, k in enumerate(keys):
        if select is not None and not select[b]:
            first.append(b)
            continue
        first.append(seen.setdefault(k, b))
        count[k] = count.get(k, 0) + 1
    multi = [1 if (select is None or select[b]) and count[k] > 1 else 0 for b, k in enumerate(keys)]
    return first, multi


def _group(sizes, digests=None, select=None):
    d = torch.from_numpy(np.ascontiguousarray(digests)).to(DEV) if digests is not None else None
    first, multi = D.group_first(np.asarray(sizes, np.int64), d, select, device=DEV)
    return first.cpu().tolist(), multi.cpu().tolist()


def test_group_tiny_and_uniform():
    assert _group([5]) == ([0], [0])
    assert _group([7] * 300) == ([0] * 300, [1] * 300)
    assert _group(list(range(300))) == (list(range(300)), [0] * 300)
    dig = np.arange(32, dtype=np.uint8).reshape(1, 32)
    assert _group([5], dig) == ([0], [0])
    assert _group([9] * 70, np.repeat(dig, 70, axis=0)) == ([0] * 70, [1] * 70)


@pytest.mark.parametrize("width", [0, 8, 16, 32])
def test_group_5000_keys_over_1000_values(width):
    rng = np.random.default_rng(100 + width)
    n, nvals = 5000, 1000
    # (with a digest, few sizes: the digest must tell the values apart)
    val_sizes = rng.integers(0, 40, nvals) if width else rng.choice(2**40, nvals, replace=False)
    val_dig = rng.integers(0, 256, (nvals, max(width, 1)), dtype=np.uint8)[:, :width]
    which = np.concatenate([np.arange(nvals), rng.integers(0, nvals, n - nvals)])
    rng.shuffle(which)
    sizes, dig = val_sizes[which], val_dig[which]
    keys = [(int(s), d.tobytes()) for s, d in zip(sizes, dig)]
    want = _dict_first(keys)
    got = _group(sizes, dig if width else None)
    assert got == want
    assert _group(sizes, dig if width else None) == got  # the same input twice: the same output
    select = (rng.integers(0, 4, n) != 0).astype(np.uint8)  # a mask with gaps
    assert _group(sizes, dig if width else None, select) == _dict_first(keys, select)


def test_group_keys_do_not_merge_across_size_or_digest():
    dig = np.zeros((6, 16), np.uint8)
    dig[3:, 15] = 1  # (differs in the last digest byte only)
    # equal digests, different sizes; equal sizes, different digests
    assert _group([1, 2, 1, 1, 2, 1], dig) == ([0, 1, 0, 3, 4, 3], [1, 0, 1, 1, 0, 1])
    dig32 = np.zeros((4, 32), np.uint8)
    dig32[1, 31], dig32[2, 0], dig32[3, 31] = 1, 1, 1
    assert _group([4, 4, 4, 4], dig32) == ([0, 1, 2, 1], [0, 1, 0, 1])
    # sizes that differ in their high half only
    assert _group([1, 1 + 2**32, 1, 1 + 2**32, 2**32]) == ([0, 1, 0, 1, 4], [1, 1, 1, 1, 0])


def test_group_long_probe_runs():
    """Keys that all start at one slot of the table (found with the rpp_group_start_slot hook): the probe runs
    grow to the number of distinct keys; the duplicates among them still meet in one slot."""
    n = 512
    slots = N.lib().rpp_group_workspace_bytes(n) // 4
    assert slots == 1024
    target = slots - 3  # (the runs wrap around the table's end)
    crowd = []
    size = 0
    while len(crowd) < 256:
        if D.group_start_slot(size, b"", n) == target:
            crowd.append(size)
        size += 1
    rng = np.random.default_rng(9)
    sizes = np.array(crowd + [crowd[i] for i in rng.integers(0, 256, 256)], np.int64)
    rng.shuffle(sizes)
    want = _dict_first([(int(s), b"") for s in sizes])
    assert _group(sizes) == want
    # the same with a digest: 16-byte digests crafted onto one start slot
    digs, k = [], 0
    while len(digs) < 64:
        cand = np.array([k, 3 * k + 1], "<u8").view(np.uint8).tobytes()
        if D.group_start_slot(77, cand, n) == 5:
            digs.append(cand)
        k += 1
    which = np.concatenate([np.arange(64), rng.integers(0, 64, n - 64)])
    rng.shuffle(which)
    dig = np.stack([np.frombuffer(digs[i], np.uint8) for i in which])
    assert _group([77] * n, dig) == _dict_first([(77, digs[i]) for i in which])


def _check_against_model(res, kat, scenario):
    files, first, hashed = scenario
    assert res.hashed.tolist() == hashed
    assert res.first.tolist() == first
    for i, f in enumerate(kat["dedup_files"]):
        assert res.hexdigest(i) == (f["xxh3_128"] if hashed[i] else None), i


def test_find_duplicates_scenario(kat, scenario):
    files, first, hashed = scenario
    assert 0 < sum(hashed) < len(files) and any(f != i for i, f in enumerate(first))
    res = D.find_duplicates(files)
    assert res.algo == "xxh3-128" and res.digests.shape == (len(files), 16)
    _check_against_model(res, kat, scenario)
    # the other algorithms decide the same
    for algo, width in (("xxh3-64", 8), ("sha512-256", 32)):
        res = D.find_duplicates(files[:11], algo)
        want_first, want_hashed = D.scanner_model(files[:11])
        assert res.digests.shape == (11, width)
        assert (res.first.tolist(), res.hashed.tolist()) == (want_first, want_hashed)
    empty = D.find_duplicates([])
    assert empty.first.tolist() == [] and empty.hashed.tolist() == []


def _scenario_on_device(files):
    buf, offs = _place(files, lambda i: (11 * i + 3) % 16)
    d_off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    d_sz = torch.tensor([len(f) for f in files], dtype=torch.int64, device=DEV)
    return torch.from_numpy(buf).to(DEV), d_off, d_sz


def test_find_duplicates_device_form_unaligned_files(kat, scenario):
    data, d_off, d_sz = _scenario_on_device(scenario[0])
    _check_against_model(D.find_duplicates_device(data, d_off, d_sz).cpu(), kat, scenario)


def test_dedup_graph_capture(kat, scenario):
    """One rpp_file_dedup_batch call captured in a graph and replayed twice."""
    data, d_off, d_sz = _scenario_on_device(scenario[0])
    out = D.find_duplicates_device(data, d_off, d_sz)  # (warm-up outside the capture; provides the buffers)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            D.find_duplicates_device(data, d_off, d_sz, out=out)
    results = []
    for _ in range(2):
        out.first.fill_(-1)
        out.hashed.fill_(7)
        out.digests.zero_()
        g.replay()
        torch.cuda.synchronize()
        results.append(out.cpu())
    assert results[0].first.tolist() == results[1].first.tolist()
    assert results[0].hashed.tolist() == results[1].hashed.tolist()
    assert results[0].digests.tobytes() == results[1].digests.tobytes()
    _check_against_model(results[1], kat, scenario)


def test_cpp_dedup(kat, scenario, tmp_path):
    """tests/cpp/dedup_test: ricepp_amd::find_duplicates on the same scenario, given as a file of the files'
    bytes and a table `size first hashed hexdigest` per file."""
    exe = ROOT / "tests" / "cpp" / "build" / "dedup_test"
    if not exe.exists():
        subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_dedup.sh")], check=True)
    files, first, hashed = scenario
    (tmp_path / "files.bin").write_bytes(b"".join(files))
    (tmp_path / "table.txt").write_text("".join(
        f"{len(f)} {first[i]} {hashed[i]} {kat['dedup_files'][i]['xxh3_128'] if hashed[i] else '-'}\n"
        for i, f in enumerate(files)))
    r = subprocess.run([str(exe), str(tmp_path / "files.bin"), str(tmp_path / "table.txt")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dedup_test: OK" in r.stdout
