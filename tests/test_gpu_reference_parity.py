"""GPU tests against the reference itself (oracle/_ref/libdwarfs_ref.so, see tests/test_reference_parity.py) and
against what was recorded from it (tests/golden/reference_kat.json).  Every comparison is for equality.  The kernels
are compared with the reference's bytes directly -- not with the oracle or the host restatements, which the CPU
tests pin separately.  The library tests skip only where neither the library nor the reference tree is; the
fixture tests never do."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from dwarfs_amd import codec
from dwarfs_amd import segmenter as SEG
from dwarfs_amd import similarity as SIM
from oracle import oracle as O
from oracle import reference as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_reference_kat as RK  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def ref():
    if not R.available():
        pytest.skip("neither oracle/_ref/libdwarfs_ref.so nor the reference tree to build it from")
    return R


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "reference_kat.json").read_text())


def _by_config(cases):
    groups = {}
    for c in cases:
        groups.setdefault(RK.case_config(c), []).append(c)
    return groups


def _codec_cfg(key) -> codec.CodecConfig:
    bs, cs, big, ulsb = key
    return codec.CodecConfig(bs, cs, "big" if big else "little", ulsb)


def _encode_group(key, inputs):
    """One encode launch over all inputs of a config: the streams, block for block."""
    n = [x.size for x in inputs]
    off = np.concatenate(([0], np.cumsum(n)[:-1]))
    d = torch.from_numpy(np.concatenate(inputs).view(np.int16)).to(DEV)
    enc = codec.encode_batch(_codec_cfg(key), d, off, n)
    torch.cuda.synchronize()
    enc.check()
    data, sizes = enc.data.cpu().numpy(), enc.sizes.cpu().numpy()
    return [data[o:o + s].tobytes() for o, s in zip(enc.offsets, sizes)]


def _decode_group(key, streams, n):
    """One decode launch over all streams of a config: the samples of each."""
    off = np.concatenate(([0], np.cumsum([(len(s) + 15) // 16 * 16 for s in streams])[:-1]))
    blob = np.zeros(int(off[-1]) + len(streams[-1]) + 16, np.uint8)
    for o, s in zip(off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, np.uint8)
    out, st = codec.decode_batch(_codec_cfg(key), torch.from_numpy(blob).to(DEV), off, [len(s) for s in streams], n)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0, st
    flat = out.cpu().numpy().view(np.uint16)
    starts = np.concatenate(([0], np.cumsum(n)))
    return [flat[starts[i]:starts[i + 1]] for i in range(len(n))]


def _dirty_cases():
    """unused_lsb_count > 0 with low bits set, Rice-coded and (for 2 unused bits) raw: see the CPU test."""
    out = {}
    for ulsb in (2, 6):
        for big in (False, True):
            dirt = RK.stored(np.full(300, 1, np.uint16), big, 0)
            out[(128, 1, big, ulsb)] = [RK.stored(RK.values("poisson", 300, 9710), big, ulsb) | dirt,
                                        RK.stored(np.tile(np.array([0, 0xFFFF >> ulsb], np.uint16), 64), big, ulsb)
                                        | dirt[:128]]
    return out


def test_encode_equals_reference_streams(ref):
    """codec.encode_batch against the reference's bytes over the grid, the crafted split cases, the one-pixel blocks
    of 16 n - 1 bits (and their neighbours) and the dirty-low-bit inputs: one batch per config, all data kinds mixed
    in it; the worst-case sizes agree for every case."""
    groups = {k: [RK.case_input(c) for c in v] for k, v in _by_config(RK.ricepp_cases()).items()}
    for k, v in _dirty_cases().items():
        groups.setdefault(k, []).extend(v)
    assert len(groups) >= 60 and {(1, 1, False, 0), (1, 1, True, 0), (4, 1, False, 0), (4, 1, True, 0)} <= set(groups)
    for key, inputs in groups.items():
        cfg = O.cfg(*key)
        got = _encode_group(key, inputs)
        for x, s in zip(inputs, got):
            assert s == ref.encode(cfg, x), (key, x.size)
            assert codec.worst_case_encoded_bytes(_codec_cfg(key), x.size) == ref.worst_case_bytes(cfg, x.size)


def test_decode_of_reference_streams(ref):
    """codec.decode_batch of streams written by the reference returns what the reference's decoder returns (the
    input, but for dirty low bits that a Rice block does not carry)."""
    groups = {k: [RK.case_input(c) for c in v] for k, v in _by_config(RK.ricepp_cases()).items()}
    dirty = _dirty_cases()
    for k, v in dirty.items():
        groups.setdefault(k, []).extend(v)
    for key, inputs in groups.items():
        cfg = O.cfg(*key)
        streams = [ref.encode(cfg, x) for x in inputs]
        got = _decode_group(key, streams, [x.size for x in inputs])
        for x, s, y in zip(inputs, streams, got):
            if key in dirty:
                assert np.array_equal(y, ref.decode(cfg, s, x.size)), (key, x.size)
            else:
                assert np.array_equal(y, x), (key, x.size)


def test_odd_length_two_streams_is_refused():
    """The reference's release build accepts it; the product refuses it, as the oracle does (the CPU test says why)."""
    x = RK.stored(RK.values("poisson", 11, 9720), True, 0)
    with pytest.raises(codec.CodecError):
        codec.create_encoder(_codec_cfg((4, 2, True, 0)), DEV).encode(x)


@pytest.mark.parametrize("kind", ["nilsimsa", "similarity"])
def test_similarity_digests_equal_reference(ref, kind):
    """Every hash message, the tie and threshold buffers among them, in one batch call, and the long ones again
    each as a lone message."""
    msgs = [RK.message_bytes(s) for s in RK.hash_messages()]
    want = [ref.nilsimsa(m) if kind == "nilsimsa" else ref.similarity_digest(m) for m in msgs]
    got = SIM.similarity_hashes(msgs, kind, device=DEV)
    assert got.has.tolist() == [1] * len(msgs)
    for i, m in enumerate(msgs):
        assert got.digests[i].tobytes() == want[i], RK.hash_messages()[i]
    for i, m in enumerate(msgs):
        if len(m) >= RK.CHUNK - 1 or RK.hash_messages()[i]["kind"] in ("ties", "threshold"):
            lone = SIM.similarity_hashes([m], kind, device=DEV)
            assert lone.digests[0].tobytes() == want[i], RK.hash_messages()[i]


def _dev(b: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b) + b"\x3c" * 16, np.uint8).copy()).to(DEV)


def _window_hashes(cases):
    """segmenter.window_hashes of every case, one batch per config: uint32 arrays in the order of `cases`."""
    out = [None] * len(cases)
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["window_bits"], c["granularity"]), []).append(i)
    for (bits, g), idx in groups.items():
        cfg = SEG.SegmenterConfig(bits, 1, g, 1024)
        msgs = [RK.message_bytes(cases[i]["message"]) for i in idx]
        starts = np.concatenate(([0], np.cumsum([len(m) for m in msgs])[:-1])) + 3
        hashes, hs = SEG.window_hashes(_dev(b"\xc3" * 3 + b"".join(msgs)), starts, [len(m) // g for m in msgs], cfg)
        flat = hashes.cpu().numpy().view(np.uint32)
        for j, i in enumerate(idx):
            out[i] = flat[hs[j]:hs[j + 1]]
    return out


def test_window_hashes_equal_driven_rsync_hash(ref):
    cases = RK.rsync_cases()
    for c, h in zip(cases, _window_hashes(cases)):
        L = (1 << c["window_bits"]) * c["granularity"]
        assert np.array_equal(h, ref.rsync_hashes(RK.message_bytes(c["message"]), L, c["granularity"])), c


@pytest.mark.parametrize("bits,g", [(3, 1), (4, 7), (12, 1), (12, 6)])
def test_index_of_repeating_windows(bits, g):
    """Blocks of two windows of one byte value, all 256 values in a batch: the first all-equal window is entered
    with the hash that rsync_hash::repeating_window gives, the later ones are not entered."""
    cfg = SEG.SegmenterConfig(bits, 1, g, 1 << 14)
    W, L = cfg.window_frames, cfg.window_bytes
    blocks = [bytes([v]) * (2 * L) for v in range(256)]
    idx = SEG.BlockIndex.build(_dev(b"".join(blocks)), [2 * L * v for v in range(256)], [2 * W] * 256, cfg)
    closed = [((v * L) & 0xFFFF) | (((v * L * (L + 1) // 2) & 0xFFFF) << 16) for v in range(256)]
    want = [R.repeating_window(v, L) for v in range(256)] if R.available() else closed
    assert want == closed
    for v in range(256):
        h, off, entered = idx.slots(v)
        assert off.tolist() == [0, W // 2, W] and h.tolist() == [want[v]] * 3 and entered.tolist() == [1, 0, 0], v


# -------------------------------------------------------------- fixtures ----

def test_kat_ricepp_encode_and_decode(kat):
    """The kernels against the recorded reference streams alone: encode gives the recorded size, SHA-256 and head;
    decoding the encoder's stream (which is then the reference's) gives the input."""
    for key, entries in _by_config(kat["ricepp"]).items():
        inputs = [RK.case_input(e) for e in entries]
        got = _encode_group(key, inputs)
        for e, s in zip(entries, got):
            assert RK.record(s) == {k: e[k] for k in ("size", "sha256", "head")}, e
        back = _decode_group(key, got, [x.size for x in inputs])
        for e, x, y in zip(entries, inputs, back):
            assert np.array_equal(x, y), e


@pytest.mark.parametrize("kind", ["nilsimsa", "similarity"])
def test_kat_similarity(kat, kind):
    msgs = [RK.message_bytes(e) for e in kat[kind]]
    got = SIM.similarity_hashes(msgs, kind, device=DEV)
    for i, e in enumerate(kat[kind]):
        assert RK.record(got.digests[i].tobytes()) == {k: e[k] for k in ("size", "sha256", "head")}, e


def test_kat_window_hashes(kat):
    for e, h in zip(kat["rsync"], _window_hashes(kat["rsync"])):
        assert h.size == e["count"]
        assert RK.record(h.astype("<u4").tobytes()) == {k: e[k] for k in ("size", "sha256", "head")}, e
