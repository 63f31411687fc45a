"""CPU tests of the named digests (no GPU needed): exported symbols and the header, the name rules of
``rpp_digest_algo``, digest sizes, argument checks, ``rpp_digest_host`` -- the definition -- on every batch shape of
tests/digest_cases.py against tests/golden/digest_kat.bin (hashlib's digests, regenerated here), the Python layer on
CPU tensors, ``extract.file_checksums(..., device="cpu")`` against hashlib over the extracted bytes, and the host code
alone under AddressSanitizer and UBSan."""

import ctypes as C
import hashlib
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import digest_cases as DC
import extract_cases as EC
from dwarfs_amd import _native as N
from dwarfs_amd import dedup, digest
from dwarfs_amd import extract as X

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rpp_digest_algo", "rpp_digest_bytes", "rpp_digest_batch", "rpp_digest_host")


def test_library_exports_the_symbols():
    raw = C.CDLL(str(N.LIB_PATH))
    header = (ROOT / "include" / "ricepp_amd.h").read_text()
    for name in SYMBOLS:
        assert hasattr(raw, name) and name in N.EXPORTED_SYMBOLS and name + "(" in header, name
    assert N.lib().rpp_abi_version() == 1


def test_names():
    L = N.lib()
    assert len(digest.ALGORITHMS) == 16 and set(digest.ALGORITHMS) == set(DC.NEW) | set(DC.OLD)
    values = [L.rpp_digest_algo(n.encode()) for n in digest.ALGORITHMS]
    assert values == list(range(16))  # the canonical names in the enum's order, a numbering of its own
    for name in DC.NEW + ("sha512-256",):  # OpenSSL's names in any letter case
        want = L.rpp_digest_algo(name.encode())
        assert L.rpp_digest_algo(name.upper().encode()) == want, name
        assert L.rpp_digest_algo(name.title().encode()) == want, name
    assert L.rpp_digest_algo(b"SHA256") == L.rpp_digest_algo(b"sha256") == digest.ALGORITHMS.index("sha256")
    assert L.rpp_digest_algo(b"BLAKE2b512") == digest.ALGORITHMS.index("blake2b512")
    for bad in (b"XXH3-64", b"Xxh3-128", b"xxh3-128 ", b"", b"sha", b"sha2566", b"sha-256", b"shake128", b"shake256",
                b"ripemd160", b"sm3", b"whirlpool", b"md5-sha1", b"md5 ", b" md5", b"crc32"):
        assert L.rpp_digest_algo(bad) < 0, bad
    assert L.rpp_digest_algo(None) < 0
    # the older group is as it was
    assert L.rpp_file_hash_algo(b"md5") < 0 and L.rpp_file_hash_digest_bytes(3) == 0
    assert dedup.ALGORITHMS == ("xxh3-64", "xxh3-128", "sha512-256")


def test_digest_sizes():
    L = N.lib()
    for name in DC.NEW:
        assert L.rpp_digest_bytes(L.rpp_digest_algo(name.encode())) == DC.WIDTH[name] == digest.digest_bytes(name)
        assert DC.WIDTH[name] == hashlib.new(DC.MK.ALGORITHMS[name][0]).digest_size
    assert [digest.digest_bytes(n) for n in DC.OLD] == [8, 16, 32]
    assert [L.rpp_digest_bytes(a) for a in (-1, 16, 17, 1 << 20)] == [0, 0, 0, 0]
    with pytest.raises(ValueError, match=r"unknown digest algorithm 'crc32' \(known: md5, sha1, .*sha512-256\)"):
        digest.digest_bytes("crc32")


def test_argument_checks_without_gpu():
    L, null, fake = N.lib(), C.c_void_p(0), C.c_void_p(0x1000)
    for a in range(16):
        assert L.rpp_digest_batch(a, null, null, null, null, 0, null, null) == N.RPP_OK  # nothing to do
        # a null pointer with work to do is refused before anything is launched (pointers that are never followed)
        assert L.rpp_digest_batch(a, null, fake, fake, null, 1, fake, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_digest_batch(a, fake, null, fake, null, 1, fake, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_digest_batch(a, fake, fake, null, null, 1, fake, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_digest_batch(a, fake, fake, fake, fake, 1, null, null) == N.RPP_INVALID_ARGUMENT
    for bad in (-1, 16, 99):
        assert L.rpp_digest_batch(bad, null, null, null, null, 0, null, null) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_digest_host(bad, null, null, null, null, 0, null) == N.RPP_INVALID_ARGUMENT
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    for name in DC.NEW + ("sha512-256",):
        a = L.rpp_digest_algo(name.encode())
        assert L.rpp_digest_host(a, null, null, null, null, 0, null) == N.RPP_OK
        assert L.rpp_digest_host(a, null, p, p, null, 1, p) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_digest_host(a, p, p, p, null, 1, null) == N.RPP_INVALID_ARGUMENT
    for name in ("xxh3-64", "xxh3-128"):  # no host definition
        assert L.rpp_digest_host(L.rpp_digest_algo(name.encode()), p, p, p, null, 1, p) == N.RPP_INVALID_ARGUMENT


def test_kat_regenerates():
    """tests/golden/digest_kat.json and .bin are what make_digest_kat.py writes (which checks hashlib against the
    published vectors first), and stay under the largest fixture committed before them."""
    obj, blob = DC.MK.build()
    assert obj == DC.kat()
    assert blob == (DC.GOLDEN / "digest_kat.bin").read_bytes()
    assert hashlib.sha256(blob).hexdigest() == obj["bin_sha256"] and len(blob) == obj["bin_bytes"]
    assert len(blob) <= (DC.GOLDEN / "zstd_kat.bin").stat().st_size
    lengths = {n for n, _ in obj["messages"]}
    assert lengths >= set(range(301)) | {4095, 4096, 4097, 65539}
    for n in DC.MK.BOUNDARY:
        assert {mis for m, mis in obj["messages"] if m == n and mis} == set(range(1, 16)), n


def host_digests(name, shape, select=None):
    buf, offs, sizes = DC.place(DC.batch_shapes()[shape])
    assert buf.ctypes.data % 16 == 0
    out = DC.guarded_out(len(sizes), DC.WIDTH[name], torch)
    got = digest.digest_batch(torch.from_numpy(buf), offs, sizes, name, select=select,
                              out=out[:len(sizes) * DC.WIDTH[name]])
    assert got.data_ptr() == out.data_ptr()
    return out.numpy()


@pytest.mark.parametrize("name", DC.NEW)
def test_host_definition_on_every_shape(name):
    for shape, idx in DC.batch_shapes().items():
        want = DC.expected(name)[np.array(idx)]
        DC.check_rows(host_digests(name, shape), want, what=(name, shape))
    idx = DC.batch_shapes()["all"]
    select = DC.select_mask(len(idx))
    DC.check_rows(host_digests(name, "all", select), DC.expected(name)[np.array(idx)], select, what=(name, "select"))


def test_published_vectors_and_python_layer():
    data = torch.from_numpy(np.frombuffer(b"abc", np.uint8).copy())
    for name in DC.NEW:
        pub = DC.kat()["published"][name]
        got = digest.digest_batch(data, [0, 0, 1], [3, 0, 0], name.upper())
        assert tuple(got.shape) == (3, DC.WIDTH[name]) and got.device.type == "cpu"
        assert digest.hexdigests(got) == [pub["abc"], pub["empty"], pub["empty"]], name
    # SHA-512/256 has a host form (its IV in the shared SHA-512 rounds); XXH3 has none
    got = digest.digest_batch(data, [0], [3], "sha512-256")
    assert digest.hexdigests(got) == [hashlib.new("sha512_256", b"abc").hexdigest()]
    with pytest.raises(ValueError, match="no host definition"):
        digest.digest_batch(data, [0], [3], "xxh3-128")
    with pytest.raises(ValueError, match="unknown digest algorithm 'sha257'"):
        digest.digest_batch(data, [0], [3], "sha257")
    with pytest.raises(ValueError, match="select needs one byte per file"):
        digest.digest_batch(data, [0], [3], "md5", select=[1, 1])
    with pytest.raises(ValueError, match="out must be"):
        digest.digest_batch(data, [0], [3], "md5", out=torch.zeros(15, dtype=torch.uint8))
    assert digest.digest_batch(data, [], [], "sha1").shape == (0, 20)


def test_file_checksums_on_the_cpu():
    case = EC.holes_cases(X.tile_bytes())[0]
    flat = np.frombuffer(b"".join(case.blocks), np.uint8)
    boff, bsz = EC.block_offsets(case.blocks), [len(b) for b in case.blocks]
    files = case.files + [[], [(0, 0, 0)]]  # (and two empty files)
    table = X.FileTable.from_files(files)
    content = X.extract_files(flat, boff, bsz, table, device="cpu")
    assert [len(c) for c in content] == table.file_sizes.tolist() and 0 in table.file_sizes.tolist()
    for name, hname in (("sha256", "sha256"), ("md5", "md5")):
        want = [hashlib.new(hname, c).hexdigest() for c in content]
        for max_bytes in (X.DEFAULT_MAX_BYTES, 1000):  # one batch, several batches
            digests, status = X.file_checksums(flat, boff, bsz, table, name, max_bytes=max_bytes, device="cpu")
            assert digests.device.type == "cpu" and status.tolist() == [0] * table.nfiles
            assert X.hexdigests(digests) == want, (name, max_bytes)
        assert X.check_files(flat, boff, bsz, table, want, name, device="cpu") == []
        wrong = list(want)
        wrong[3] = want[2]
        assert X.check_files(flat, boff, bsz, table, wrong, name, device="cpu", max_bytes=1000) == [3]
    assert len(X.batches(table.file_sizes, 1000)) >= 3
    # a bad chunk: its file is marked, its digest is over zeros in the chunk's place, the others are right
    bad = EC.bad_cases()[0]
    flat = np.frombuffer(b"".join(bad.blocks), np.uint8)
    boff, bsz = EC.block_offsets(bad.blocks), [len(b) for b in bad.blocks]
    table = X.FileTable.from_files(bad.files)
    digests, status = X.file_checksums(flat, boff, bsz, table, "sha256", device="cpu")
    assert status.tolist() == [0, 0, N.RPP_BAD_CHUNK, 0, 0]
    for f in (0, 1, 3, 4):
        good = b"".join(bad.blocks[b][o:o + s] if b != EC.HOLE else bytes(s) for b, o, s in bad.files[f])
        assert digests[f].numpy().tobytes() == hashlib.sha256(good).digest()
    # (file 2 = 20 good bytes, 50 bytes of a block that does not exist, 20 good bytes)
    zeros = bad.blocks[0][0:20] + bytes(50) + bad.blocks[1][5:25]
    assert digests[2].numpy().tobytes() == hashlib.sha256(zeros).digest()
    assert X.check_files(flat, boff, bsz, table, digests, "sha256", device="cpu") == [2]
    # the names of dedup keep their route: no host form, as before; a name nobody knows is a ValueError
    with pytest.raises(ValueError, match="needs a GPU device"):
        X.file_checksums(flat, boff, bsz, table, "xxh3-128", device="cpu")
    with pytest.raises(ValueError, match="unknown digest algorithm 'crc32'"):
        X.file_checksums(flat, boff, bsz, table, "crc32", device="cpu")


def test_cpp_host_digests_under_asan_ubsan(tmp_path):
    """tests/cpp/digest_test.cpp: the host code in a program of its own, built with AddressSanitizer and UBSan:
    the published vectors, and a length sweep in exact-size heap buffers at every misalignment against digests
    passed in a file (hashlib's)."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_digest.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = []
    for name in DC.NEW:
        hname = DC.MK.ALGORITHMS[name][0]
        for n in list(range(0, 300, 7)) + [55, 56, 64, 111, 112, 128, 71, 72, 135, 136, 143, 144, 1000]:
            lines.append(f"{name} {n} {hashlib.new(hname, bytes((k * 31 + n) & 0xFF for k in range(n))).hexdigest()}\n")
    (tmp_path / "sweep.txt").write_text("".join(lines))
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "digest_test"), str(tmp_path / "sweep.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "digest_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
