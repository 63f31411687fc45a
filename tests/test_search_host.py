"""CPU tests of the search word (no GPU needed): the host encoders under each of the eight words over the inputs of
tests/search_cases.py.  The sequences are those of the definition restated in Python (search_cases.restate);
every LZ4 block and Zstandard frame is read by the project's host decoders, by the independent readers
tests/lz4_ref.py and tests/zstd_ref.py, and by liblz4 1.9.3 and libzstd 1.4.8, whose verdict
tests/golden/search_kat.json records under the SHA-256 of the very bytes.  Then what each constructed family aims
at, the one asserted size condition, invalid words at every entry point, the Python layer, and the host
functions alone under AddressSanitizer and UBSan."""

import ctypes as C
import functools
import hashlib
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lz4_ref as LR
import search_cases as SC
import zstd_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import block_codec
from dwarfs_amd import lz4
from dwarfs_amd import zstd as Z

ROOT = Path(__file__).resolve().parent.parent
ALL_WORDS = (0,) + SC.WORDS
INVALID = (3, 5, 16, SC.LAZY, 0x200 | 2, 0x1000 | 8, 1 << 31)


@functools.lru_cache(maxsize=None)
def kat():
    return json.loads((ROOT / "tests" / "golden" / "search_kat.json").read_text())


@functools.lru_cache(maxsize=None)
def encoded(fmt, search):
    """[(name, input, bytes, flag)] per format ("lz4", "zstd0", "zstd3") and search word, computed once"""
    if fmt == "lz4":
        return [(name, data, *lz4.host_encode(data, search)) for name, data in SC.inputs()]
    return [(name, data, *Z.host_encode(data, int(fmt[4:]), search)) for name, data in SC.inputs()]


@functools.lru_cache(maxsize=None)
def restated(search):
    """{name: [(position, length, offset)]} by the Python restatement"""
    return {name: SC.restate(data, search) for name, data in SC.inputs()}


def lz4_sequences(block):
    return [(s.out_at + s.literals, s.match, s.offset) for s in LR.walk(block) if s.offset is not None]


@pytest.mark.parametrize("search", ALL_WORDS)
def test_host_sequences_are_the_definitions(search):
    want = restated(search)
    for name, data, block, _ in encoded("lz4", search):
        assert lz4_sequences(block) == want[name], name
        assert all(1 <= off <= 65535 for _, _, off in want[name]), name
    # the Zstandard encoder is handed the same sequences: per chunk, in a frame without repeat codes
    for name, data, frame, _ in encoded("zstd0", search):
        blocks = SC.AC.blocks(frame)
        for i, b in enumerate(blocks):
            if b.kind != 2:
                continue
            cs, got, at = i * SC.CHUNK, [], i * SC.CHUNK
            for ll, ml, ov in b.sequences:
                got.append((at + ll, ml, ov - 3))
                at += ll + ml
            assert got == [s for s in want[name] if cs <= s[0] < cs + SC.CHUNK], (name, i)


def test_depth_1_is_search_0():
    for fmt in ("lz4", "zstd0", "zstd3"):
        assert [c[2:] for c in encoded(fmt, 1)] == [c[2:] for c in encoded(fmt, 0)], fmt
    for name, data, block, flag in encoded("lz4", 0):
        assert (block, flag) == lz4.host_encode(data), name  # ... and search 0 is the old entry point
    for name, data, frame, flag in encoded("zstd3", 0):
        assert (frame, flag) == Z.host_encode(data, 3), name


@pytest.mark.parametrize("search", ALL_WORDS)
def test_three_readers_and_the_recorded_verdict(search):
    records = kat()["cases"]
    assert kat()["versions"] == {"lz4": "1.9.3", "zstd": "1.4.8"} and tuple(kat()["words"]) == ALL_WORDS
    assert [r["name"] for r in records] == [name for name, _ in SC.inputs()]
    at = ALL_WORDS.index(search)
    for fmt in ("lz4", "zstd0", "zstd3"):
        total = 0
        for rec, (name, data, enc, flag) in zip(records, encoded(fmt, search)):
            n = len(data)
            assert rec["size"] == n and rec[fmt]["sizes"][at] == len(enc), (fmt, name)
            assert rec[fmt]["decoded"] == n, (fmt, name)  # the library decoded the pinned bytes to the input
            if fmt == "lz4":
                assert LR.decode(enc, n) == data, name
                LR.check_end_rules(enc, n)
                assert lz4.host_decode(enc, n) == (N.RPP_OK, data), name
                assert len(enc) <= lz4.bound(n) and flag == (4 + len(enc) >= n), name
            else:
                assert R.decode(enc) == data, (fmt, name)
                assert Z.host_decode(enc, n) == (N.RPP_OK, data), (fmt, name)
                assert len(enc) <= Z.bound(n) and flag == (len(enc) >= n), (fmt, name)
            total += len(enc)
        assert kat()["totals"][str(search)][fmt]["all"] == total, fmt


def test_the_pinned_bytes():
    """The fixture holds one SHA-256 per input and format, over the results of the nine words one behind the
    other: the bytes that liblz4 and libzstd decoded when it was written."""
    for fmt in ("lz4", "zstd0", "zstd3"):
        for i, rec in enumerate(kat()["cases"]):
            joined = b"".join(encoded(fmt, w)[i][2] for w in ALL_WORDS)
            assert rec[fmt]["sha256"] == hashlib.sha256(joined).hexdigest(), (fmt, rec["name"])


def test_constructed_totals():
    """The one size condition: over the constructed inputs, each built around a longer match that the
    one-candidate search cannot see, depth 8 with LAZY is smaller in total than search 0."""
    first = len(SC.AC.inputs())
    for fmt in ("lz4", "zstd3"):
        deep = sum(len(c[2]) for c in encoded(fmt, 8 | SC.LAZY)[first:])
        greedy = sum(len(c[2]) for c in encoded(fmt, 0)[first:])
        assert deep < greedy, (fmt, deep, greedy)
        assert kat()["totals"]["264"][fmt]["constructed"] == deep and kat()["totals"]["0"][fmt]["constructed"] == greedy


def taken(name, search):
    """{position: (length, offset)} of an input's sequences under a word"""
    return {p: (ln, off) for p, ln, off in restated(search)[name]}


def test_depth_families_reach_what_they_aim_at():
    SC.constructed()
    found = 0
    for name, aim in SC.AIMS.items():
        for search in SC.WORDS:
            depth, seqs = search & ~SC.LAZY, taken(name, search)
            if "first_depth" in aim:  # the source is the first_depth-th newest entry of its bucket
                for p in aim["at"]:
                    if depth >= aim["first_depth"]:
                        assert seqs[p][0] >= 40, (name, search, p)
                        found += 1
                    else:
                        assert p not in seqs or seqs[p][0] <= 7, (name, search, p)
            if "missed_by" in aim:  # that many newer entries: found from the next depth on
                for p in aim["at"]:
                    assert (seqs.get(p, (0, 0))[0] >= 40) == (depth > aim["missed_by"]), (name, search, p)
    assert found == 6 * (6 + 4 + 2 + 4)  # 6 units per input; the words of depth 2, 4 and 8 up, and 4 up again
    # the collisions of colliding_words hold other words: never a match, only a lost place in the bucket
    for search in (1, 2):
        assert not any(p in taken("colliding_words", search) for p in SC.AIMS["colliding_words"]["at"])


def test_lazy_families_reach_what_they_aim_at():
    SC.constructed()
    for search in SC.WORDS:
        lazy = bool(search & SC.LAZY)
        for name in ("climb_1", "climb_3", "climb_into_next_step", "climb_to_step_end"):
            aim = SC.AIMS[name]
            p, seqs, scores = aim["at"], taken(name, search), {}
            SC.restate(dict(SC.inputs())[name], search, scores)
            assert p % SC.STEP == aim["lane"]
            # every position of the climb that lies in the query's step scores one more than the one before
            inside = min(aim["steps"], SC.STEP - 1 - aim["lane"])
            if lazy:  # (without LAZY the positions behind the match taken are never scored)
                assert [scores[p + j][1] for j in range(inside + 1)] == [SC.CLIMB_BASE + j for j in range(inside + 1)]
                assert seqs[p + inside][0] == SC.CLIMB_BASE + inside and not any(p + j in seqs for j in range(inside))
            else:
                assert seqs[p][0] == SC.CLIMB_BASE, (name, search)
        # scores of CAP on both neighbours: the first one is taken whole
        p = SC.AIMS["cap_both"]["at"]
        scores = {}
        SC.restate(dict(SC.inputs())["cap_both"], search, scores)
        assert taken("cap_both", search)[p] == (80, p - 21) and scores[p][1] == SC.CAP
        if lazy:
            assert scores[p + 1][1] == SC.CAP
    assert SC.AIMS["climb_into_next_step"]["lane"] == SC.STEP - 1  # the better neighbour lies in the next step


def test_ties_limits_and_far_offsets():
    SC.constructed()
    for search in SC.WORDS:
        for name in ("tie", "tie_at_cap"):
            aim = SC.AIMS[name]
            assert taken(name, search)[aim["at"]] == (aim["length"], aim["offset"]), (name, search)
        assert taken("ends_at_limit", search)[266] == (25, 128)  # cut 5 bytes before the end; the nearer of two
        far = taken("far_offsets", search)
        assert far[3 * SC.CHUNK - 4] == (4, 65532)  # the window's first position, cut at the chunk's end
        assert 3 * SC.CHUNK - 104 not in far and 3 * SC.CHUNK - 304 not in far  # 65535 and 65536 back: no candidates
        assert max(off for _, off in far.values()) == 65532
        # 64 equal hashes in a step (zeros), two groups of 32 (a period of 2).  The first run ends at 400 and its
        # positions from 384 on were inserted last, so the second run, at 500, meets the bucket's depth-th newest
        # entry as its longest candidate: 396 back to 389 (zeros), 396 back to 382 in steps of 2 (period 2, where
        # the next position's candidates start at 395 and reach one byte further)
        depth, lazy = search & ~SC.LAZY, bool(search & SC.LAZY)
        zeros, period = taken("zeros_then_zeros", search), taken("period_2_then_period_2", search)
        assert restated(search)["zeros_then_zeros"][0] == (64, 336, 1)
        assert restated(search)["period_2_then_period_2"][0] == (64, 336, 2)
        assert zeros[500] == (3 + depth, 103 + depth), (search, zeros)
        if depth == 8:  # (only 7 of them hold the word: the eighth entry, from the run's second step, spans the run)
            assert period[500] == (40, 374), (search, period)
        elif lazy:
            assert 500 not in period and period[501] == (3 + 2 * depth, 104 + 2 * depth), (search, period)
        else:
            assert period[500] == (2 + 2 * depth, 102 + 2 * depth), (search, period)
    for n in (0, 1, 12):
        assert all(restated(s)[f"repeats_{n}"] == [] for s in SC.WORDS)
    assert {name: len(d) for name, d in SC.constructed()}["repeats_66313"] == 2 * SC.CHUNK + 777


def test_invalid_words_at_every_entry_point():
    L = N.lib()
    src = np.frombuffer(b"abcdefghabcdefghabcdefgh", np.uint8)
    out = np.zeros(256, np.uint8)
    n = C.c_uint64()
    for bad in INVALID:
        assert L.rpp_lz4_host_encode_search(src.ctypes.data_as(C.c_void_p), len(src), bad,
                                            out.ctypes.data_as(C.c_void_p), 256, C.byref(n),
                                            None) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_zstd_host_encode_search(src.ctypes.data_as(C.c_void_p), len(src), 0, bad,
                                             out.ctypes.data_as(C.c_void_p), 256, C.byref(n),
                                             None) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_lz4_encode_batch_search(None, None, None, 0, bad, None, None, None, None, None, 0, None, 0,
                                             None) == N.RPP_INVALID_ARGUMENT
        assert L.rpp_zstd_encode_batch_search(None, None, None, 0, 3, bad, None, None, None, None, None, 0, None, 0,
                                              None) == N.RPP_INVALID_ARGUMENT
        with pytest.raises(Exception):
            lz4.host_encode(b"abcdefgh", bad)
        with pytest.raises(Exception):
            Z.host_encode(b"abcdefgh", 0, bad)
        with pytest.raises(ValueError):
            lz4.Lz4BlockCompressor(device="cpu", search=bad)
        with pytest.raises(ValueError):
            Z.ZstdBlockCompressor(device="cpu", search=bad)
    for good in ALL_WORDS:
        assert L.rpp_lz4_encode_batch_search(None, None, None, 0, good, None, None, None, None, None, 0, None, 0,
                                             None) == N.RPP_OK
        assert L.rpp_zstd_encode_batch_search(None, None, None, 0, 3, good, None, None, None, None, None, 0, None, 0,
                                              None) == N.RPP_OK
    assert L.rpp_zstd_encode_batch_search(None, None, None, 0, 4, 8, None, None, None, None, None, 0, None, 0,
                                          None) == N.RPP_INVALID_ARGUMENT  # the options word keeps its own check
    assert lz4.SEARCH_LAZY == Z.SEARCH_LAZY == N.RPP_SEARCH_LAZY == 0x100


def test_python_layer_on_the_cpu():
    by_name = dict(SC.inputs())
    names = ("older_is_longer_8", "climb_3", "repeats_32769", "records_600")
    for search in ALL_WORDS:
        comp = lz4.Lz4BlockCompressor(9, "cpu", search)
        assert comp.describe() == "lz4hc [level=9]" and comp.clone().search == search
        zcomp = Z.ZstdBlockCompressor(device="cpu", options=3, search=search)
        assert zcomp.describe() == "zstd [level=22]" and zcomp.clone().search == search and zcomp.clone().options == 3
        for name in names:
            data = by_name[name]
            payload = comp.clone().compress(data)
            assert payload == lz4.frame_header(len(data)) + lz4.host_encode(data, search)[0], name
            assert lz4.decompress(payload, "cpu") == data, name
            frame = zcomp.clone().compress(data)
            assert frame == Z.host_encode(data, 3, search)[0] and Z.decompress(frame, "cpu") == data, name
    assert lz4.Lz4BlockCompressor(device="cpu").search == 0 and Z.ZstdBlockCompressor(device="cpu").search == 0
    # specs: depth=N and lazy=0|1 beside level, which maps to no search word
    for spec, level, search in (("lz4", None, 0), ("lz4hc", 9, 0), ("lz4hc:level=9", 9, 0), ("lz4hc:level=12", 12, 0),
                                ("lz4hc:level=9:depth=8:lazy=1", 9, 8 | SC.LAZY), ("lz4:depth=2", None, 2),
                                ("lz4:lazy=1", None, 1 | SC.LAZY), ("lz4hc:depth=4:lazy=0", 9, 4),
                                ("lz4hc:lazy=1:depth=1:level=3", 3, 1 | SC.LAZY)):
        comp = block_codec.block_compressor(spec, device="cpu")
        assert (comp.level, comp.search) == (level, search), spec
        assert comp.compress(by_name["climb_3"])[4:] == lz4.host_encode(by_name["climb_3"], search)[0], spec
    for spec, level, search in (("zstd", 22, 0), ("zstd:level=3", 3, 0), ("zstd:level=3:depth=8:lazy=1", 3, 8 | SC.LAZY),
                                ("zstd:depth=4", 22, 4), ("zstd:lazy=1", 22, 1 | SC.LAZY)):
        comp = Z.block_compressor(spec, "cpu")
        assert (comp.level, comp.search, comp.options) == (level, search, 0), spec
        assert comp.compress(by_name["climb_3"]) == Z.host_encode(by_name["climb_3"], 0, search)[0], spec
    for spec, name, what in (("lz4hc:depth=3", "lz4hc", "depth=3"), ("lz4:depth=16", "lz4", "depth=16"),
                             ("lz4hc:level=9:lazy=2", "lz4hc", "lazy=2"), ("lz4:depth", "lz4", "depth"),
                             ("lz4:level=3:depth=2", "lz4", "level=3"), ("null:depth=2", "null", "depth=2")):
        with pytest.raises(RuntimeError, match=f"^invalid option\\(s\\) for {name}: {what}$"):
            block_codec.block_compressor(spec, device="cpu")
    for spec, what in (("zstd:depth=3", "depth=3"), ("zstd:lazy=yes", "lazy=yes"), ("zstd:level=3:depth=0", "depth=0")):
        with pytest.raises(RuntimeError, match=f"^invalid option\\(s\\) for zstd: {what}$"):
            Z.block_compressor(spec, "cpu")


def test_cpp_host_encoders_under_asan_ubsan(tmp_path):
    """tests/cpp/search_test.cpp: host encode under every word, then host decode, of every input in a program of
    its own, built with AddressSanitizer and UBSan, with exact-size heap buffers."""
    r = subprocess.run(["bash", str(ROOT / "tests" / "cpp" / "build_search.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = tmp_path / "search_vectors.bin"
    with open(vec, "wb") as f:
        for i, (_, data) in enumerate(SC.inputs()):
            sizes = [len(encoded(fmt, w)[i][2]) for w in ALL_WORDS for fmt in ("lz4", "zstd3")]
            f.write(np.array([len(data)] + sizes, "<i8").tobytes() + data)
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "build" / "search_test"), str(vec)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "search_test: OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
