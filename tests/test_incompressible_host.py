"""CPU tests of the incompressible categorizer (no GPU needed): the host restatement
(``rpp_incompressible_host_scan``, ``device="cpu"``) over the cases of tests/incompressible_cases.py.  Sizes are the
Zstandard host encoder's for each piece alone, verdicts are recomputed in Python doubles, fragment lists and stats
are compared with a plain-Python restatement of the reference's get_fragments / add_hole / result
(incompressible_cases.model_file), the asserted families with libzstd 1.4.8's recorded verdicts
(tests/golden/incompressible_kat.json), then the argument rules and the host scan alone under AddressSanitizer and
UBSan."""

import ctypes as C
import functools
import hashlib
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import incompressible_cases as IC
from dwarfs_amd import _native as N
from dwarfs_amd import categorize as CZ
from dwarfs_amd import zstd as Z
from dwarfs_amd.lz4 import SEARCH_LAZY

ROOT = Path(__file__).resolve().parent.parent
WORDS = ((0, 0), (3, 0), (3, 8 | SEARCH_LAZY))
KIB = 1024


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((ROOT / "tests" / "golden" / "incompressible_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def host_size(piece: bytes, options: int = 0, search: int = 0) -> int:
    return len(Z.host_encode(piece, options, search)[0])


def cfg_of(case, **kw):
    return CZ.IncompressibleConfig(min_input_size=case.min_input_size, block_size=case.block_size,
                                   generate_fragments=case.fragments, **kw)


def is_hole(p):
    return isinstance(p, CZ.Hole)


def expect(file, cfg):
    """The restatement's answer for a file, with the host encoder's sizes."""
    parts = CZ.IncompressibleCategorizer._parts(file)
    frags, stats = IC.model_file(parts, cfg, lambda p: host_size(p, cfg.options, cfg.search), is_hole)
    return (None if frags is None else [CZ.Fragment(*f) for f in frags]), (None if stats is None else CZ.Stats(*stats))


def test_fixture_is_of_these_inputs():
    assert kat()["version"] == "1.4.8" and [r["name"] for r in kat()["cases"]] == [c.name for c in IC.cases()]
    for rec, case in zip(kat()["cases"], IC.cases()):
        assert (rec["size"], rec["sha256"]) == (len(case.data), hashlib.sha256(case.data).hexdigest()), case.name
        assert [p["n"] for p in rec["pieces"]] == [len(p) for p in IC.pieces(case)], case.name
        assert rec["asserted"] == case.asserted


@pytest.mark.parametrize("options,search", WORDS)
def test_every_piece_is_the_encoders_size(options, search):
    for case in IC.cases():
        cfg = cfg_of(case, options=options, search=search)
        scan = CZ.scan_pieces([case.data], cfg, "cpu")
        want = [host_size(p, options, search) for p in IC.pieces(case)]
        assert scan.sizes.tolist() == want, case.name
        ns = [len(p) for p in IC.pieces(case)]
        assert scan.verdicts.tolist() == [int(float(s) >= 0.99 * float(n)) for s, n in zip(want, ns)], case.name
        assert scan.totals[0, :4].tolist() == [sum(ns), sum(want), len(ns), int(scan.verdicts.sum())], case.name
        assert scan.total_bytes == len(case.data)


def test_recorded_host_sizes():
    for rec, case in zip(kat()["cases"], IC.cases()):
        for key, options in (("host_0_0", 0), ("host_3_0", 3)):
            got = CZ.scan_pieces([case.data], cfg_of(case, options=options), "cpu").sizes.tolist()
            assert got == [p[key] for p in rec["pieces"]], (case.name, key)


def test_asserted_families_agree_with_libzstd():
    """Every piece of an asserted family: libzstd level -1 ratio outside (0.90, 1.0) (the fixture's condition), and
    this project's verdict at 0.99 is libzstd's."""
    seen = 0
    for rec, case in zip(kat()["cases"], IC.cases()):
        if not case.asserted:
            continue
        for options in (0, 3):
            scan = CZ.scan_pieces([case.data], cfg_of(case, options=options), "cpu")
            for p, verdict in zip(rec["pieces"], scan.verdicts.tolist()):
                assert not 0.90 < p["zstd_m1"] / p["n"] < 1.0, case.name
                assert verdict == p["zstd_verdict"] == int(float(p["zstd_m1"]) >= 0.99 * float(p["n"])), case.name
                seen += 1
    assert seen >= 2 * 15


def test_borderline_family_is_recorded_with_both_verdicts():
    recs = [r for r in kat()["cases"] if not r["asserted"]]
    assert {r["name"] for r in recs} >= {"borderline_far_repeat", "borderline_below_200"}
    for r in recs:
        for p in r["pieces"]:
            assert {p["zstd_verdict"], p["host_verdict"]} <= {0, 1}
    far = next(r for r in recs if r["name"] == "borderline_far_repeat")["pieces"][0]
    assert (far["zstd_verdict"], far["host_verdict"]) == (0, 1)  # the repeat lies beyond the 64 KiB window


def by_name(name):
    return next(c for c in IC.cases() if c.name == name)


def categorize(case, **kw):
    return CZ.IncompressibleCategorizer(cfg_of(case, **kw), "cpu").categorize(case.data)


def test_reference_families():
    """test/incompressible_categorizer_test.cpp with this project's data"""
    cat = CZ.IncompressibleCategorizer(device="cpu")
    assert cat.categories() == ("incompressible",)
    r = categorize(by_name("random_10000"))
    assert r.fragments == [CZ.Fragment("incompressible", 10000)] and r.stats == CZ.Stats(1, 1, 10000, 10010)
    r = categorize(by_name("text_10000"))
    assert r.fragments == [] and r.stats.incompressible_blocks == 0 and r.stats.total_in == 10000
    r = categorize(by_name("categorize_fragments"))
    assert r.fragments == [CZ.Fragment("<default>", 16384), CZ.Fragment("incompressible", 8192),
                           CZ.Fragment("<default>", 16384), CZ.Fragment("incompressible", 8192),
                           CZ.Fragment("<default>", 3072)]
    assert r.stats[:3] == (2, 7, 52224)
    assert categorize(by_name("min_input_size_999")) == CZ.FileResult(None, None)
    assert categorize(by_name("min_input_size_10000")).fragments == [CZ.Fragment("incompressible", 10000)]


def test_two_max_ratios_on_one_text():
    case, m = by_name("max_ratio_text"), kat()["max_ratio"]
    size = host_size(case.data)
    assert m["case"] == case.name and m["host_ratio"] == size / len(case.data)
    assert m["below"] == m["host_ratio"] - 0.1 and m["above"] == m["host_ratio"] + 0.1
    assert categorize(case, max_ratio=m["below"]).fragments == [CZ.Fragment("incompressible", len(case.data))]
    assert categorize(case, max_ratio=m["above"]).fragments == []


def hole_files():
    t, r = IC.text, IC.random_bytes
    H = CZ.Hole
    mixed = t(3 * KIB) + r(9401, 2 * KIB) + t(1 * KIB) + r(9402, 3 * KIB + 1)
    return {
        "hole_at_start": [H(4096), mixed],
        "hole_in_the_middle": [t(5000), H(100), r(9403, 5000)],
        "hole_at_end": [r(9404, 3000), H(8192)],
        "adjacent_holes": [t(2000), H(1), H(2), r(9405, 2000), H(3), H(4)],
        "only_holes": [H(1000), H(24)],
        "hole_then_default": [H(500), t(4000)],
        "data_in_two_parts": [t(1500), r(9406, 1500), H(10), mixed[:700], mixed[700:]],
        "empty_extent_between_holes": [H(300), b"", H(300), t(600)],
        "all_default": t(20 * KIB),
        "all_default_list": [t(20 * KIB)],
        "all_incompressible": r(9407, 5 * KIB),
        "empty": b"",
        "below_min_input_size": r(9408, 255),
        "below_min_with_hole": [r(9409, 100), H(100)],
        "at_min_with_hole": [r(9410, 100), H(156)],
        "exact_multiple": r(9411, 4 * KIB),
        "last_piece_one_byte": t(4 * KIB) + r(9412, 1),
    }


@pytest.mark.parametrize("fragments", (False, True))
@pytest.mark.parametrize("block_size", (1 * KIB, "1M"))
def test_fragment_lists_and_stats_against_the_restatement(fragments, block_size):
    cfg = CZ.IncompressibleConfig(block_size=block_size, generate_fragments=fragments)
    files = hole_files()
    cat = CZ.IncompressibleCategorizer(cfg, "cpu")
    got = cat.categorize_many(list(files.values()))
    for (name, file), res in zip(files.items(), got):
        assert (res.fragments, res.stats) == expect(file, cfg), name
        if res.fragments:  # result()'s check: the fragments cover the file
            parts = cat._parts(file)
            assert sum(f.size for f in res.fragments) == sum(p.size if is_hole(p) else len(p) for p in parts), name
    res = dict(zip(files, got))
    assert res["empty"] == res["below_min_input_size"] == res["below_min_with_hole"] == CZ.FileResult(None, None)
    assert res["at_min_with_hole"].fragments is not None
    # an all-default file: no fragment without the fragment list, one default fragment with it
    assert res["all_default"].fragments == ([CZ.Fragment("<default>", 20 * KIB)] if fragments else [])
    assert res["only_holes"].fragments == [CZ.Fragment("<default>", 1000), CZ.Fragment("<default>", 24)]
    assert res["hole_then_default"].fragments == [CZ.Fragment("<default>", 500), CZ.Fragment("<default>", 4000)]
    # the bytes of the files without a job are not in the buffer
    skipped = ("empty", "below_min_input_size", "below_min_with_hole")
    data_bytes = sum(len(p) for n, f in files.items() if n not in skipped for p in cat._parts(f) if not is_hole(p))
    assert cat.last_total_bytes == data_bytes


def test_all_default_with_one_piece_and_fragments_is_one_default_fragment():
    cfg = CZ.IncompressibleConfig(generate_fragments=True)
    res = CZ.IncompressibleCategorizer(cfg, "cpu").categorize(IC.text(10000))
    assert res.fragments == [CZ.Fragment("<default>", 10000)]  # (as the reference returns)
    assert CZ.IncompressibleCategorizer(CZ.IncompressibleConfig(min_input_size=0), "cpu").categorize(b"").fragments == []


def test_config_rules():
    cfg = CZ.IncompressibleConfig()
    assert (cfg.min_input_size, cfg.block_size, cfg.generate_fragments, cfg.max_ratio, cfg.options, cfg.search) == \
        (256, 1 << 20, False, 0.99, 0, 0)
    assert CZ.IncompressibleConfig(block_size="8k", min_input_size="1M").block_size == 8192
    assert CZ.IncompressibleConfig(min_input_size="2K").min_input_size == 2048
    assert CZ.IncompressibleConfig(block_size="1G").block_size == 1 << 30
    for bad in (0, (1 << 30) + 1, "2g"):
        with pytest.raises(ValueError):
            CZ.IncompressibleConfig(block_size=bad)
    for bad in ("8kb", "k", "8x", ""):
        with pytest.raises(RuntimeError):
            CZ.IncompressibleConfig(block_size=bad)
    with pytest.raises(ValueError):
        CZ.IncompressibleConfig(options=4)
    with pytest.raises(ValueError):
        CZ.IncompressibleConfig(search=3)


def test_argument_errors_of_the_abi():
    L = N.lib()
    for name in ("rpp_incompressible_workspace_bytes", "rpp_incompressible_scan_batch", "rpp_incompressible_host_scan"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(L, name)
    data = np.frombuffer(IC.text(1000), np.uint8)
    offs, szs, base = CZ.cut([1000], 256)
    out = [np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.zeros((1, 5), np.uint64), np.zeros((4, 2), np.uint64),
           np.zeros(1, np.uint32), np.zeros(4, np.int32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def host(options, search, npieces=4):
        return L.rpp_incompressible_host_scan(p(data), p(offs), p(szs), npieces, p(base), 1, 0.99, 1, options, search,
                                              *(p(a) for a in out))

    assert host(0, 0) == N.RPP_OK and out[0].tolist() == [host_size(bytes(data[o:o + 256])) for o in range(0, 1000, 256)]
    assert host(4, 0) == host(0x10, 0) == N.RPP_INVALID_ARGUMENT      # an unknown options bit
    assert host(0, 3) == host(0, 0x200) == host(0, SEARCH_LAZY) == N.RPP_INVALID_ARGUMENT  # a bad search word
    assert host(0, 0, npieces=3) == N.RPP_INVALID_ARGUMENT            # piece_base ends behind the pieces
    assert L.rpp_incompressible_host_scan(None, None, None, 0, None, 0, 0.99, 0, 0, 0, *[None] * 6) == N.RPP_OK
    # the batch call checks its arguments before it touches the device (pointers that are never followed)
    ws_bytes = L.rpp_incompressible_workspace_bytes(1000, 4, 1)
    assert ws_bytes >= L.rpp_zstd_encode_workspace_bytes(1000, 4) and ws_bytes % 16 == 0
    fake = C.c_void_p(0x1000)

    def batch(options, search, ws, npieces=4):
        return L.rpp_incompressible_scan_batch(fake, fake, fake, npieces, fake, 1, 0.99, 1, options, search, fake, fake,
                                               fake, fake, fake, fake, 1000, fake, ws, None)

    assert batch(4, 0, ws_bytes) == batch(0, 3, ws_bytes) == N.RPP_INVALID_ARGUMENT
    assert batch(0, 0, ws_bytes - 1) == N.RPP_OUTPUT_TOO_SMALL        # a workspace one byte short
    assert batch(0, 0, 0, npieces=0) == N.RPP_OK                      # no pieces: nothing to do
    assert L.rpp_incompressible_scan_batch(fake, fake, fake, 4, fake, 1, 0.99, 1, 0, 0, fake, fake, fake, fake, fake,
                                           fake, 1000, C.c_void_p(0x1008), ws_bytes, None) == N.RPP_INVALID_ARGUMENT


def test_cpp_host_scan_under_asan_ubsan():
    """tests/cpp/incompressible_test.cpp: the host scan over generated extents in a program of its own, built with
    AddressSanitizer and UBSan, with exact-size heap buffers, against rpp_zstd_host_encode_search's sizes."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_incompressible.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "incompressible_test")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "incompressible_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
