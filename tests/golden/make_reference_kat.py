"""Writes tests/golden/reference_kat.json: outputs of the compiled reference (oracle/_ref/libdwarfs_ref.so, built
by oracle/ref_build.py from the reference's own sources) for the ricepp codec and the three scan hashes.

    python tests/golden/make_reference_kat.py

This module also holds the inputs of tests/test_reference_parity.py and tests/test_gpu_reference_parity.py: every
input is made of integer draws (`Generator.integers`) or written out, so that a recorded answer stays valid.
Each entry records the seed / kind / length (or the name of a crafted input), the size, the SHA-256 and the first
16 bytes of the reference's stream or digest; "build_flags" are the flags the library was compiled with.  `build`
asserts that the oracle (ricepp) and the host restatements (hashes) agree with the reference before it writes.

Crafted single-block inputs for the split search of compute_best_split (ricepp/include/ricepp/detail/encode.h:
43-90), with bits(fs) = n (fs + 1) + sum(delta >> fs) and start = bit_length(sum / n) - 2 (at least 0):

* bits_used == 16 n cannot exist in a Rice block, and bits_used == 16 n - 1 only in a block of one pixel.
  bits(f + 1) - bits(f) = n - sum(ceil((delta >> f) / 2)) <= n - sum(delta >> f) / 2.  If the search ended at
  f <= 13 with bits(f) >= 16 n - 1, then sum(delta >> f) >= (15 - f) n - 1 >= 2 n - 1 and the step to f + 1 costs
  at most 1/2, i.e. nothing: an ascending search goes on (`tmp > bits` continues on equality) and the downward
  choice (bits(f) < bits(f + 1)) is excluded.  That leaves the no-search tie bits(f - 1) == bits(f), which needs
  sum(ceil((delta >> (f - 1)) / 2)) == n.  With bits(f) == 16 n, sum(delta >> (f - 1)) >= 3 n and the sum of
  the halves is at least 1.5 n: impossible.  With bits(f) == 16 n - 1 it is at least (3 n - 1) / 2, which exceeds
  n for n >= 2 but not for n == 1: a one-pixel block (block size 1, or the one-pixel tail of a length of
  bs + 1) whose difference is in [8192, 12288) has start 12 and bits(12) == bits(13) == 15, goes up on the tie
  without a search and is Rice-coded with fs = 13 in 16 n - 1 bits, one below the raw bound.  `one_pixel_blocks`
  has both ends of that range, as a second block of block size 1 and as a tail, and the neighbours 8191 (14
  bits) and 12288 (bits(13) == bits(14): up to 14, raw).  For n >= 2 "rice_16n_minus_2" is the largest Rice
  block there is, and "raw_tie_16n_minus_1" has bits(13) == bits(14) == 16 n - 1, steps up on the tie and is
  stored raw.
* A descending search never takes a step: start > 0 means sum(delta) >= 2^(start + 1) n, so
  sum(ceil((delta >> (start - 1)) / 2)) > 1.5 n > n and bits(start - 1) > bits(start).  Downward is only ever
  "stay at start": "down_at_0" (start == 0, the only way to fs == 0) and "down_at_1" (start == 1).
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CHUNK = 32768  # rpp_similarity_chunk_bytes() of the kernels these lengths were laid out for

# ---------------------------------------------------------------- ricepp ----

BLOCK_SIZES = [1, 2, 16, 29, 128, 511, 512]
STREAMS = [1, 2]
ULSB = [0, 2, 6, 15]
KINDS = ["constant", "noise", "poisson", "random", "ramp"]


def lengths(bs, cs):
    out = []
    for n in (cs, bs * cs - cs, bs * cs, bs * cs + cs, 3 * bs * cs + 5 * cs):
        if n > 0 and n not in out:
            out.append(n)
    return out


def values(kind, n, seed):
    """n logical 16-bit pixel values."""
    rng = np.random.default_rng(seed)
    if kind == "constant":
        v = np.full(n, 40000 + seed % 1000, np.int64)
    elif kind == "noise":
        v = 1000 + rng.integers(-1, 2, n)
    elif kind == "poisson":  # a sum of twelve small integer draws around a pedestal
        v = 1000 + rng.integers(0, 9, (n, 12)).sum(axis=1)
    elif kind == "random":
        v = rng.integers(0, 65536, n)
    elif kind == "ramp":  # wraps 2^16 every 255 pixels
        v = 65000 + 257 * np.arange(n, dtype=np.int64)
    elif kind.startswith("lap"):  # differences uniform in [-2^k, 2^k]
        k = int(kind[3:])
        v = 30000 + np.cumsum(rng.integers(-(1 << k), (1 << k) + 1, n))
    else:
        raise ValueError(kind)
    return (v & 0xFFFF).astype(np.uint16)


def stored(v, big, ulsb):
    """Logical values as stored samples: the low 16 - ulsb bits shifted up, in the named byte order."""
    s = ((v.astype(np.uint32) & (0xFFFF >> ulsb)) << ulsb).astype(np.uint16)
    return s.byteswap() if big else s


def from_deltas(first, deltas):
    """Pixels whose zigzag differences are `deltas` (the first pixel's difference is 0 by construction)."""
    px, out = first, [first]
    for d in deltas:
        diff = (d >> 1) if d % 2 == 0 else -((d + 1) >> 1)
        px = (px + diff) & 0xFFFF
        out.append(px)
    return np.array(out, np.uint16)


def bits_for_fs(deltas, fs):
    return len(deltas) * (fs + 1) + sum(d >> fs for d in deltas)


def start_fs(deltas):
    return max(0, (sum(deltas) // len(deltas)).bit_length() - 2)


def zigzag_deltas(v):
    """The zigzag differences of one block of logical values that starts its stream."""
    v = v.astype(np.int64)
    diff = np.concatenate(([0], np.diff(v))) & 0xFFFF
    return [int((d << 1) & 0xFFFF) if d < 0x8000 else int(~(d << 1) & 0xFFFF) for d in diff]


def crafted():
    """name -> logical values of one block (block size = length, one stream)."""
    n = 128
    c = {}
    # (the first difference of a single block is always 0)
    c["sum_zero"] = from_deltas(51966, [0] * (n - 1))                       # non-zero first pixel, sum 0: code 0
    c["tie_no_search"] = from_deltas(100, [3] + [2] * (n - 2))              # start 0, bits(0) == bits(1): fs 1
    c["down_at_0"] = from_deltas(100, [1] * 40 + [0] * (n - 41))            # start 0, bits(0) < bits(1): fs 0
    c["down_at_1"] = from_deltas(100, [5] * 112 + [1] * 15)                 # start 1, bits(1) < bits(2): fs 1
    c["up_equal_to_raw"] = from_deltas(7, [30000, 0] * 63 + [30000])        # 12 -> 13 -> (equal) 14: raw
    c["up_step_on_equal"] = from_deltas(9, [1023] * (n - 2) + [2047])       # 8 -> 9 -> (equal) 10, then stops
    c["rice_16n_minus_2"] = from_deltas(11, [20000] * (n - 1))              # bits(13) = 16 n - 2 < bits(14)
    c["raw_tie_16n_minus_1"] = from_deltas(11, [20000] * (n - 2) + [24576])  # bits(13) == bits(14) == 16 n - 1
    c["all_ones"] = from_deltas(0, [65535] * (n - 1))                       # start 14 at once: raw
    d = {k: zigzag_deltas(v) for k, v in c.items()}
    # the arithmetic the names promise (of the definition above, not of any implementation)
    assert sum(d["sum_zero"]) == 0
    assert start_fs(d["tie_no_search"]) == 0 and bits_for_fs(d["tie_no_search"], 0) == bits_for_fs(d["tie_no_search"], 1)
    assert start_fs(d["down_at_0"]) == 0 and bits_for_fs(d["down_at_0"], 0) < bits_for_fs(d["down_at_0"], 1)
    assert start_fs(d["down_at_1"]) == 1 and bits_for_fs(d["down_at_1"], 1) < bits_for_fs(d["down_at_1"], 2)
    u = d["up_equal_to_raw"]
    assert start_fs(u) == 12 and bits_for_fs(u, 12) > bits_for_fs(u, 13) == bits_for_fs(u, 14) < 16 * n
    e = d["up_step_on_equal"]
    assert start_fs(e) == 8 and bits_for_fs(e, 8) > bits_for_fs(e, 9) == bits_for_fs(e, 10) < bits_for_fs(e, 11)
    r = d["rice_16n_minus_2"]
    assert start_fs(r) == 13 and bits_for_fs(r, 13) == 16 * n - 2 < bits_for_fs(r, 14) and bits_for_fs(r, 12) > 16 * n
    t = d["raw_tie_16n_minus_1"]
    assert start_fs(t) == 13 and bits_for_fs(t, 13) == bits_for_fs(t, 14) == 16 * n - 1
    assert start_fs(d["all_ones"]) == 14
    return c


def one_pixel_blocks():
    """name -> (block size, logical values): a constant first block (code 0, no payload), then one block of one
    pixel whose zigzag difference is the name's number."""
    out = {}
    for d in (8191, 8192, 12287, 12288):
        pair = from_deltas(100, [d])
        out["%d_bs1" % d] = (1, pair)
        out["%d_tail" % d] = (4, np.concatenate((np.full(4, 100, np.uint16), pair[1:])))
    return out


def second_split_code(stream: bytes) -> int:
    """The split code of the second block of a one-stream stream whose first block has code 0 (and so no payload):
    bits 20..23, the high nibble of byte 2."""
    assert stream[2] & 15 == 0
    return stream[2] >> 4


COVERAGE = [("lap%d" % k, 9100 + k) for k in range(0, 15)]  # single blocks of 128 whose best split rises with k
COVERAGE += [("lap4", 9200), ("lap8", 9200)]  # (codes 5 and 9, which the rising set steps over)


def case(bs, cs, big, ulsb, kind, seed, length):
    return {"block_size": bs, "streams": cs, "big_endian": int(big), "unused_lsb": ulsb, "kind": kind, "seed": seed,
            "length": length}


def single_block_cases():
    """One block, one stream, clean 16-bit values: the crafted inputs and the coverage set, in both byte orders."""
    out = []
    for i, (name, v) in enumerate(crafted().items()):
        out.append(case(len(v), 1, i % 2, 0, "crafted:" + name, 0, len(v)))
    for i, (kind, seed) in enumerate(COVERAGE):
        out.append(case(128, 1, i % 2, 0, kind, seed, 128))
    return out


def grid_cases():
    """Every block size, stream count and length, all five data kinds at each; byte order and unused LSB count
    rotate (five kinds against eight combinations: every combination meets every block size)."""
    out, i = [], 0
    for bs in BLOCK_SIZES:
        for cs in STREAMS:
            for n in lengths(bs, cs):
                for kind in KINDS:
                    out.append(case(bs, cs, i % 2, ULSB[(i // 2) % 4], kind, 9000 + i, n))
                    i += 1
    return out


def one_pixel_cases():
    return [case(bs, 1, big, 0, "onepx:" + name, 0, len(v)) for name, (bs, v) in one_pixel_blocks().items()
            for big in (0, 1)]


def ricepp_cases():
    return single_block_cases() + one_pixel_cases() + grid_cases()


_CRAFTED = None


def case_input(c) -> np.ndarray:
    """The stored samples of a case."""
    global _CRAFTED
    if c["kind"].startswith("crafted:"):
        if _CRAFTED is None:
            _CRAFTED = crafted()
        v = _CRAFTED[c["kind"][8:]]
    elif c["kind"].startswith("onepx:"):
        v = one_pixel_blocks()[c["kind"][6:]][1]
    else:
        v = values(c["kind"], c["length"], c["seed"])
    return stored(v, c["big_endian"], c["unused_lsb"])


def case_config(c):
    return (c["block_size"], c["streams"], bool(c["big_endian"]), c["unused_lsb"])


def split_code(stream: bytes) -> int:
    """The 4-bit split code of the first block of a one-stream stream: the writer fills a 64-bit word from bit 0
    and stores it little endian (bitstream_writer.h:125-145), so after the 16-bit first value the code is the low
    nibble of byte 2."""
    return stream[2] & 15


# ---------------------------------------------------------------- hashes ----

HASH_LENGTHS = list(range(10)) + [31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
HASH_KINDS = ["rng", "zero", "ff", "period2"]


def hash_messages():
    specs = []
    for k, kind in enumerate(HASH_KINDS):
        specs += [{"kind": kind, "seed": 9300 + 100 * k + i, "length": n} for i, n in enumerate(HASH_LENGTHS)]
    specs.append({"kind": "ties", "seed": TIE_SEED, "length": 303})
    specs.append({"kind": "threshold", "seed": THRESHOLD_SEED, "length": 1000})
    return specs


TIE_SEED = 9501        # 303 random bytes: 300 four-byte substrings whose bucket counts tie around rank four
THRESHOLD_SEED = 9502  # 1000 random bytes: some nilsimsa accumulator equals the threshold (8 * 1000 - 28) // 256


def message_bytes(spec) -> bytes:
    n, kind = spec["length"], spec["kind"]
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    if kind == "period2":
        return (b"\xa5\x3c" * (n // 2 + 1))[:n]
    return np.random.default_rng(spec["seed"]).integers(0, 256, n, dtype=np.uint8).tobytes()


RSYNC_WINDOW_BITS = [3, 4, 12]
RSYNC_GRANULARITIES = [1, 2, 3, 6, 7, 64]
RSYNC_KINDS = ["rng", "ff", "period2"]


def rsync_cases():
    out, i = [], 0
    for bits in RSYNC_WINDOW_BITS:
        W = 1 << bits
        for g in RSYNC_GRANULARITIES:
            for kind in RSYNC_KINDS:
                for frames in (W, W + 1, 3 * W + 5):
                    out.append({"window_bits": bits, "granularity": g,
                                "message": {"kind": kind, "seed": 9600 + i, "length": frames * g}})
                    i += 1
    return out


def window_lengths():
    return sorted({(1 << b) * g for b in RSYNC_WINDOW_BITS for g in RSYNC_GRANULARITIES})


# ------------------------------------------------------------------ file ----

def record(data: bytes) -> dict:
    return {"size": len(data), "sha256": hashlib.sha256(data).hexdigest(), "head": data[:16].hex()}


def kat_ricepp_cases():
    grid = grid_cases()
    return single_block_cases() + one_pixel_cases() + grid[3::20]


def kat_hash_messages():
    m = hash_messages()
    return [s for s in m if s["kind"] in ("rng", "ties", "threshold")] + \
        [s for s in m if s["kind"] != "rng" and s["length"] in (3, 4, 5, 33, CHUNK + 1)][:11]


def kat_rsync_cases():
    return rsync_cases()[1::5][:30]


def build():
    from dwarfs_amd import segmenter as SEG
    from dwarfs_amd import similarity as SIM
    from oracle import oracle as O
    from oracle import reference as R

    kat = {"build_flags": R.build_flags(), "ricepp": [], "nilsimsa": [], "similarity": [], "rsync": []}
    for c in kat_ricepp_cases():
        x, cfg = case_input(c), O.cfg(*case_config(c))
        stream = R.encode(cfg, x)
        assert O.encode(cfg, x) == stream, c
        assert np.array_equal(R.decode(cfg, stream, x.size), x), c
        kat["ricepp"].append(dict(c, **record(stream)))
    for s in kat_hash_messages():
        m = message_bytes(s)
        nil, sim = R.nilsimsa(m), R.similarity_digest(m)
        assert SIM.host_hash(m, "nilsimsa") == nil and SIM.host_hash(m, "similarity") == sim, s
        kat["nilsimsa"].append(dict(s, **record(nil)))
        kat["similarity"].append(dict(s, **record(sim)))
    for c in kat_rsync_cases():
        m = message_bytes(c["message"])
        cfg = SEG.SegmenterConfig(c["window_bits"], 1, c["granularity"], 1024)
        h = R.rsync_hashes(m, cfg.window_bytes, c["granularity"])
        assert np.array_equal(SEG.host_hashes(m, cfg), h), c
        kat["rsync"].append(dict(c, count=int(h.size), **record(h.astype("<u4").tobytes())))
    kat["repeating_window"] = {str(L): record(np.array([R.repeating_window(v, L) for v in range(256)],
                                                        "<u4").tobytes()) for L in window_lengths()}
    return kat


def main():
    kat = build()
    (HERE / "reference_kat.json").write_text(json.dumps(kat, indent=0, separators=(",", ":")) + "\n")
    print({k: len(v) for k, v in kat.items() if not isinstance(v, str)})


if __name__ == "__main__":
    main()
