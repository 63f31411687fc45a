"""CPU differential tests against the reference itself: oracle/_ref/libdwarfs_ref.so is the reference's ricepp codec
and its nilsimsa, similarity and rsync hashes, compiled unmodified by oracle/ref_build.py.  The oracle
(oracle/ricepp_oracle.c), the host restatements of the C ABI and the Python models of tests/golden/ are compared
with it for equality of bytes and integers; no tolerance appears anywhere.

The tests that need the library skip only when neither it nor the reference tree is there.  The fixture tests
(tests/golden/reference_kat.json, recorded from the library) need neither and never skip."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

from dwarfs_amd import segmenter as SEG
from dwarfs_amd import similarity as SIM
from oracle import oracle as O
from oracle import reference as R

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_reference_kat as RK  # noqa: E402
import make_segment_kat as SEGK  # noqa: E402
import make_similarity_kat as SIMK  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    if not R.available():
        pytest.skip("neither oracle/_ref/libdwarfs_ref.so nor the reference tree to build it from")
    return R


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "reference_kat.json").read_text())


# ---------------------------------------------------------------- ricepp ----

def test_grid_keeps_every_axis_value():
    g = RK.grid_cases()
    assert {c["block_size"] for c in g} == {1, 2, 16, 29, 128, 511, 512}
    assert {c["streams"] for c in g} == {1, 2} and {c["big_endian"] for c in g} == {0, 1}
    assert {c["unused_lsb"] for c in g} == {0, 2, 6, 15} and {c["kind"] for c in g} == set(RK.KINDS)
    for bs in RK.BLOCK_SIZES:
        for cs in (1, 2):
            want = {n for n in (cs, bs * cs - cs, bs * cs, bs * cs + cs, 3 * bs * cs + 5 * cs) if n}
            assert {c["length"] for c in g if (c["block_size"], c["streams"]) == (bs, cs)} == want
            assert {(c["big_endian"], c["unused_lsb"]) for c in g if c["block_size"] == bs} == \
                {(b, u) for b in (0, 1) for u in (0, 2, 6, 15)}


def test_oracle_streams_equal_reference(ref):
    """Stream for stream over the grid and the single-block cases; each side decodes the other's stream; the
    worst-case sizes agree."""
    for c in RK.ricepp_cases():
        cfg, x = O.cfg(*RK.case_config(c)), RK.case_input(c)
        want = ref.encode(cfg, x)
        got = O.encode(cfg, x)
        assert got == want, c
        assert np.array_equal(O.decode(cfg, want, x.size), x), c
        assert np.array_equal(ref.decode(cfg, got, x.size), x), c
        assert O.worst_case_bytes(cfg, x.size) == ref.worst_case_bytes(cfg, x.size) >= len(want), c


def _single_block_one_stream():
    return [c for c in RK.ricepp_cases() if c["streams"] == 1 and c["length"] <= c["block_size"]]


def test_split_codes_covered_by_reference_streams(ref):
    """Read from the reference's own streams: every split code 0..15 occurs among the single-block cases, and so
    do both choices of direction -- upward with a step of the loop, and downward, which can only ever mean staying at
    the start split (see make_reference_kat.py), at start 0 (the one way to fs = 0) and at start 1."""
    codes = {}
    for c in _single_block_one_stream():
        s = ref.encode(O.cfg(*RK.case_config(c)), RK.case_input(c))
        codes.setdefault(RK.split_code(s), []).append(c["kind"])
    assert sorted(codes) == list(range(16)), sorted(codes)
    crafted = RK.crafted()
    code = {k: RK.split_code(ref.encode(O.cfg(len(v), 1, False, 0), v)) for k, v in crafted.items()}
    start = {k: RK.start_fs(RK.zigzag_deltas(v)) for k, v in crafted.items()}
    assert code["sum_zero"] == 0
    assert code["tie_no_search"] == start["tie_no_search"] + 2 == 2        # fs = start + 1: the tie goes upward
    assert code["down_at_0"] == 1 and start["down_at_0"] == 0              # fs = 0
    assert code["down_at_1"] == 2 and start["down_at_1"] == 1              # fs = start >= 1: downward, no step
    assert code["up_step_on_equal"] - 1 == start["up_step_on_equal"] + 2   # upward, and a loop step on equality
    assert code["up_equal_to_raw"] == 15 and start["up_equal_to_raw"] == 12  # 13, then 14 on equality: raw
    assert code["rice_16n_minus_2"] == 14                                  # the largest Rice block: fs = 13
    assert code["raw_tie_16n_minus_1"] == 15 and code["all_ones"] == 15
    n = 128
    assert len(ref.encode(O.cfg(n, 1, False, 0), crafted["rice_16n_minus_2"])) == (20 + 16 * n - 2 + 7) // 8
    assert len(ref.encode(O.cfg(n, 1, False, 0), crafted["raw_tie_16n_minus_1"])) == (20 + 16 * n + 7) // 8


def test_one_pixel_blocks_of_16n_minus_1_bits(ref):
    """The one Rice block that sits one bit below the raw bound `bits_used < 16 n`: a block of one pixel whose
    zigzag difference is in [8192, 12288) ties bits(12) == bits(13) == 15, goes to fs = 13 without a search and is
    Rice-coded (make_reference_kat.py).  Read from the reference's streams: code 14 at both ends of the range, as a
    second block of block size 1 and as a one-pixel tail; 8191 is Rice-coded in 14 bits, 12288 is raw."""
    for name, (bs, v) in RK.one_pixel_blocks().items():
        d = int(name.split("_")[0])
        for big in (False, True):
            cfg, x = O.cfg(bs, 1, big, 0), RK.stored(v, big, 0)
            s = ref.encode(cfg, x)
            assert RK.second_split_code(s) == (14 if d < 12288 else 15), name
            assert len(s) == 5 and O.encode(cfg, x) == s, name
            assert np.array_equal(ref.decode(cfg, s, x.size), x) and np.array_equal(O.decode(cfg, s, x.size), x)
        assert RK.zigzag_deltas(v)[-1] == d
        if 8192 <= d < 12288:
            assert RK.bits_for_fs([d], 12) == RK.bits_for_fs([d], 13) == 16 * 1 - 1
    # the payload: 15 bits for a Rice block of 16 n - 1 (the stream ends at bit 39), 14 for 8191
    assert ref.encode(O.cfg(1, 1, False, 0), RK.one_pixel_blocks()["8192_bs1"][1]) == bytes.fromhex("6400e00200")


def test_largest_rice_blocks(ref):
    """No Rice block of the reference has 16 n bits, and none of two pixels or more has 16 n - 1 (the argument is
    in make_reference_kat.py).  Scanned on second blocks, whose every difference is free (the first difference of
    a stream is always 0): random blocks of few pixels and few distinct values, where such sizes are easiest to hit,
    behind a constant first block.  The least slack is 1 bit, at n = 1 only."""
    rng = np.random.default_rng(9700)
    least = {}
    for it in range(6000):
        n = int(rng.integers(1, 9))
        hi = int(rng.integers(13, 17))
        block = rng.integers(0, 1 << hi, 3)[rng.integers(0, 3, n)].astype(np.uint16)
        v = np.concatenate((np.full(n, 100, np.uint16), block))
        code = RK.second_split_code(ref.encode(O.cfg(n, 1, False, 0), v))
        if 1 <= code <= 14:
            deltas = RK.zigzag_deltas(v[n - 1:])[1:]
            slack = 16 * n - RK.bits_for_fs(deltas, code - 1)
            least[n] = min(least.get(n, 99), slack)
    assert least[1] == 1 and all(least[n] == 2 for n in range(2, 9)), least


def test_dirty_low_bits(ref):
    """unused_lsb_count > 0 with low bits set: a release build of the reference shifts them away on the Rice path
    and writes the sample as stored on the raw path.  The oracle follows both."""
    for ulsb in (2, 6):
        for big in (False, True):
            cfg = O.cfg(128, 1, big, ulsb)
            dirt = RK.stored(np.full(300, 1, np.uint16), big, 0)  # bit 0 of the stored value
            x = RK.stored(RK.values("poisson", 300, 9710), big, ulsb) | dirt
            s = ref.encode(cfg, x)
            assert O.encode(cfg, x) == s
            assert RK.split_code(s) not in (0, 15)
            back = ref.decode(cfg, s, 300)
            assert np.array_equal(back, x & ~dirt) and np.array_equal(O.decode(cfg, s, 300), back)
            # one raw block: every stored sample comes back as it was, dirt included.  With 16 - ulsb bits a pixel
            # the differences stay below 2^(17 - ulsb): only ulsb <= 2 can reach the raw path at all.
            y = RK.stored(np.tile(np.array([0, 0xFFFF >> ulsb], np.uint16), 64), big, ulsb) | dirt[:128]
            s = ref.encode(cfg, y)
            assert O.encode(cfg, y) == s and (RK.split_code(s) == 15) == (ulsb == 2)
            if ulsb == 2:
                assert np.array_equal(ref.decode(cfg, s, 128), y) and np.array_equal(O.decode(cfg, s, 128), y)


def test_odd_length_two_streams_is_refused(ref):
    """The reference accepts an odd pixel count with two component streams (its assert is off in a release build):
    drop | stride gives stream 0 one pixel more.  But its worst-case size counts floor(n / 2) pixels per stream, so
    its own encoder overruns the buffer it allocates on incompressible input, and DwarFS never gets there
    (src/compression/ricepp.cpp:86 throws on a size that is no multiple of the component count).  The oracle and
    the product refuse such a call; what the reference does with it is pinned here all the same."""
    cfg = O.cfg(4, 2, True, 0)
    for n in (9, 11):  # 9: the last chunk has one pixel, fewer than streams; 11: three, two of them for stream 0
        x = RK.stored(RK.values("poisson", n, 9720), True, 0)
        s = ref.encode(cfg, x)
        assert np.array_equal(ref.decode(cfg, s, n), x)
        with pytest.raises(O.OracleError) as e:
            O.encode(cfg, x)
        assert e.value.status == O.INVALID_ARGUMENT
        # the first 8-pixel chunk is coded as in the even stream: decoding 8 pixels of the odd stream gives them,
        # and the odd stream is the even one (less its padding) with the tail's blocks appended
        even = ref.encode(cfg, x[:8])
        assert O.encode(cfg, x[:8]) == even and len(s) >= len(even)
        assert np.array_equal(ref.decode(cfg, s, 8), x[:8]) and np.array_equal(O.decode(cfg, s, 8), x[:8])
        assert s[:len(even) - 1] == even[:-1]
    assert ref.worst_case_bytes(cfg, 9) == ref.worst_case_bytes(cfg, 8) == O.worst_case_bytes(cfg, 8)
    # Fewer pixels than streams, the empty input among them: the reference would read input[i] for every stream,
    # past the end.  It is never called with them: this status is the driver's own (ref_driver.cpp check_defined),
    # not an answer of the reference.
    for n in (0, 1):
        with pytest.raises(O.OracleError) as e:
            ref.encode(cfg, np.zeros(n, np.uint16))
        assert e.value.status == O.INVALID_ARGUMENT


def test_unsupported_configs_agree(ref):
    x = np.arange(8, dtype=np.uint16)
    for bs, cs in ((513, 1), (128, 3), (128, 0)):
        for side in (ref, O):
            with pytest.raises(O.OracleError) as e:
                side.encode(O.cfg(bs, cs, True, 0), x)
            assert e.value.status == O.UNSUPPORTED_CONFIG
    cfg, y = O.cfg(128, 1, True, 0), RK.values("random", 300, 9740)
    for side in (ref, O):  # a stream cut in the middle: std::out_of_range
        with pytest.raises(O.OracleError) as e:
            side.decode(cfg, ref.encode(cfg, y)[:100], 300)
        assert e.value.status == O.TRUNCATED_INPUT


# ---------------------------------------------------------------- hashes ----

def _ref_digest(ref, kind, data, sizes=None):
    return ref.nilsimsa(data, sizes) if kind == "nilsimsa" else ref.similarity_digest(data, sizes)


def _model_digest(kind, data):
    return (SIMK.Nilsimsa() if kind == "nilsimsa" else SIMK.Similarity()).update(data).digest()


def test_chunk_size_is_the_one_the_lengths_surround():
    assert SIM.chunk_bytes() == RK.CHUNK


@pytest.mark.parametrize("kind", ["nilsimsa", "similarity"])
def test_hashes_equal_reference(ref, kind):
    """The host restatement on every message; the Python model on every short one and on the long random ones."""
    for spec in RK.hash_messages():
        m = RK.message_bytes(spec)
        want = _ref_digest(ref, kind, m)
        assert SIM.host_hash(m, kind) == want, spec
        if spec["length"] <= 1000 or spec["kind"] == "rng":
            assert _model_digest(kind, m) == want, spec


def test_tie_and_threshold_buffers_are_what_they_claim(ref):
    m = RK.message_bytes({"kind": "ties", "seed": RK.TIE_SEED, "length": 303})
    assert len({m[i:i + 4] for i in range(300)}) == 300
    acc = SIMK.Similarity().update(m).acc
    order = sorted(range(256), key=lambda i: (-acc[i], i))
    assert acc[order[3]] == acc[order[4]], "the fourth and fifth bucket tie: (count desc, index asc) decides"
    assert len({acc[i] for i in order[:4]}) < 4, "two of the top four tie: their order is by index"
    assert ref.similarity(m) == order[0] << 24 | order[1] << 16 | order[2] << 8 | order[3]
    t = RK.message_bytes({"kind": "threshold", "seed": RK.THRESHOLD_SEED, "length": 1000})
    nil = SIMK.Nilsimsa().update(t)
    threshold = nil.total() // 256
    at = [i for i, c in enumerate(nil.acc) if c == threshold]
    assert threshold == 31 and at, "some accumulator equals the threshold: its bit must be clear"
    d = ref.nilsimsa(t)
    assert all(not (d[i >> 3] >> (i & 7)) & 1 for i in at)
    assert all((d[i >> 3] >> (i & 7)) & 1 for i, c in enumerate(nil.acc) if c == threshold + 1)


@pytest.mark.parametrize("kind", ["nilsimsa", "similarity"])
def test_split_updates_equal_reference(ref, kind):
    """The same bytes fed in two updates, cut at every one of the first six bytes and at the chunk boundary: the
    reference's incremental path (update_slow, then update_fast) and the host state's."""
    short = RK.message_bytes({"kind": "rng", "seed": 9730, "length": 40})
    long = RK.message_bytes({"kind": "rng", "seed": 9731, "length": 2 * RK.CHUNK + 3})
    for m, cuts in ((short, range(0, 7)), (long, (RK.CHUNK - 1, RK.CHUNK, RK.CHUNK + 1))):
        whole = _ref_digest(ref, kind, m)
        for cut in cuts:
            assert _ref_digest(ref, kind, m, [cut, len(m) - cut]) == whole, cut
            assert SIM.HostState(kind).update(m[:cut]).update(m[cut:]).digest() == whole, cut
    for i in range(0, 5):  # three pieces inside the first bytes
        assert _ref_digest(ref, kind, short, [i, 1, len(short) - i - 1]) == _ref_digest(ref, kind, short)


def test_window_hashes_equal_driven_rsync_hash(ref):
    """segmenter.host_hashes and the prefix-sum model against rsync_hash driven as the segmenter drives it."""
    for c in RK.rsync_cases():
        m = RK.message_bytes(c["message"])
        cfg = SEG.SegmenterConfig(c["window_bits"], 1, c["granularity"], 1024)
        want = ref.rsync_hashes(m, cfg.window_bytes, c["granularity"])
        assert want.size == len(m) // c["granularity"] - cfg.window_frames + 1
        assert np.array_equal(SEG.host_hashes(m, cfg), want), c
        model = SEGK.hashes(m, SEGK.cfg(c["window_bits"], c["granularity"]))
        assert np.array_equal(model, want), c


def test_repeating_window_all_bytes(ref):
    """rsync_hash::repeating_window for all 256 bytes at every window length the configs give, against the
    Python model (make_segment_kat.hashes of an all-equal window, and its closed form), against rsync_hash driven
    over an all-equal window, and against the host restatement."""
    for bits in RK.RSYNC_WINDOW_BITS:
        for g in RK.RSYNC_GRANULARITIES:
            cfg = SEG.SegmenterConfig(bits, 1, g, 1024)
            L = cfg.window_bytes
            for v in range(256):
                want = ref.repeating_window(v, L)
                window = bytes([v]) * L
                assert want == ((v * L) & 0xFFFF) | (((v * L * (L + 1) // 2) & 0xFFFF) << 16), (v, L)
                assert SEGK.hashes(window, SEGK.cfg(bits, g)).tolist() == [want], (v, L)
                assert ref.rsync_hashes(window, L, g).tolist() == [want], (v, L)
                assert SEG.host_hashes(window, cfg).tolist() == [want], (v, L)
    assert SEGK.window_hash(b"\x5a" * 48) == ref.repeating_window(0x5A, 48)  # (the definition, evaluated directly)


# -------------------------------------------------------------- fixtures ----
# recorded from the library: these need neither it nor the reference tree

def test_kat_shape(kat):
    assert 35 <= len(kat["ricepp"]) <= 64 and len(kat["nilsimsa"]) == len(kat["similarity"]) >= 30
    assert len(kat["rsync"]) == 30 and len(kat["repeating_window"]) == len(RK.window_lengths())
    assert "-DNDEBUG" in kat["build_flags"] and "RICEPP_CPU_VARIANT=fallback" in kat["build_flags"]
    assert "BMI2" not in kat["build_flags"]
    assert (GOLDEN / "reference_kat.json").stat().st_size < (GOLDEN / "segment_kat.json").stat().st_size
    assert {e["kind"] for e in kat["ricepp"]} >= {"crafted:" + k for k in RK.crafted()} | \
        {"onepx:" + k for k in RK.one_pixel_blocks()}


def test_kat_is_current(ref, kat):
    """With the library at hand: the committed file is what the generator writes."""
    assert json.loads(json.dumps(RK.build())) == kat


def test_kat_ricepp_oracle(kat):
    for e in kat["ricepp"]:
        cfg, x = O.cfg(*RK.case_config(e)), RK.case_input(e)
        s = O.encode(cfg, x)
        assert RK.record(s) == {k: e[k] for k in ("size", "sha256", "head")}, e
        assert np.array_equal(O.decode(cfg, s, x.size), x)
    codes = {RK.split_code(bytes.fromhex(e["head"])) for e in kat["ricepp"] if e["streams"] == 1
             and e["length"] <= e["block_size"]}
    assert codes == set(range(16))
    second = {e["kind"]: RK.second_split_code(bytes.fromhex(e["head"])) for e in kat["ricepp"]
              if e["kind"].startswith("onepx:")}
    assert len(second) == 8 and all(c == (15 if k.startswith("onepx:12288") else 14) for k, c in second.items())


@pytest.mark.parametrize("kind", ["nilsimsa", "similarity"])
def test_kat_hashes_host_and_model(kat, kind):
    for e in kat[kind]:
        m = RK.message_bytes(e)
        want = {k: e[k] for k in ("size", "sha256", "head")}
        assert RK.record(SIM.host_hash(m, kind)) == want, e
        if e["length"] <= 1000:
            assert RK.record(_model_digest(kind, m)) == want, e
    assert {"ties", "threshold"} <= {e["kind"] for e in kat[kind]}


def test_kat_rsync_host_and_model(kat):
    for e in kat["rsync"]:
        m = RK.message_bytes(e["message"])
        cfg = SEG.SegmenterConfig(e["window_bits"], 1, e["granularity"], 1024)
        want = {k: e[k] for k in ("size", "sha256", "head")}
        h = SEG.host_hashes(m, cfg)
        assert h.size == e["count"] and RK.record(h.astype("<u4").tobytes()) == want, e
        model = SEGK.hashes(m, SEGK.cfg(e["window_bits"], e["granularity"]))
        assert RK.record(model.astype("<u4").tobytes()) == want, e
    for L, want in kat["repeating_window"].items():
        L = int(L)
        closed = [((v * L) & 0xFFFF) | (((v * L * (L + 1) // 2) & 0xFFFF) << 16) for v in range(256)]
        assert RK.record(np.array(closed, "<u4").tobytes()) == want, L
