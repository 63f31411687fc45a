"""The FLAC encoder (rpp_flac_encode_kernel) held to a rule-by-rule model on inputs built for its decisions.

flac_enc_cases.py aims one input at each choice the planner makes -- wasted bits, constant, verbatim, the fixed
order, the legal residual range, the partition order and its caps, the Rice parameters and the 4/5-bit switch,
the four stereo assignments and their ties, every header field -- and test_flac_encode_model_host.py proves on
the CPU that each input meets its aim under the model (flac_enc_model.py).  Here:

* levels 0, 1 and 2 (integer from samples to bytes): the GPU's stream equals the model's, byte for byte, for
  every case, through compress_many in both orders and, for the block-size edges, through compress;
* levels 3, 5, 8 and 5 exhaustive (float window, coefficients not predicted): every subframe that is not LPC is
  the model's plan at that level's partition cap; every LPC subframe obeys the level's order limit, the automatic
  precision, and, given the coefficients and shift it carries, has exactly the Rice plan the model gives the
  residuals they imply, and is strictly shorter than the model's plan without LPC; a stereo pair is no longer
  than the model's best pair without LPC; every stream decodes to its input under the RFC reader;
* one direct rpp_flac_encode_batch call into a buffer of 0xA5 writes nothing past the total it reports.

Every comparison is for equality or an integer inequality.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import flac_enc_cases as K
import flac_enc_model as M
import flac_ref as R
from dwarfs_amd import _native as N
from dwarfs_amd import flac as FL
from dwarfs_amd.pcm import PcmSampleEndianness as E, PcmSamplePadding as Pd, PcmSampleSignedness as S
from test_gpu_flac import ar_audio, meta, pcm_bytes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_pcm, _model = {}, {}


def ar_case():
    """One frame of test_gpu_flac.ar_audio: all-pole audio a linear predictor codes and fixed predictors do not."""
    return K.Case("ar_audio_16", 1, 16, ar_audio(1, 4096, 16).astype(np.int64), ("lpc", None))


def as_int32(samples):
    return (np.asarray(samples, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def item(case):
    """(PCM bytes, metadata) of the case: little-endian signed samples of ceil(bits / 8) bytes."""
    nbytes = (case.bits + 7) // 8
    if case.name not in _pcm:
        if case.bits in (8, 16, 32):
            _pcm[case.name] = case.samples.astype(f"<i{nbytes}").tobytes()
        elif case.bits == 24:
            raw = case.samples.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
            _pcm[case.name] = np.ascontiguousarray(raw).tobytes()
        else:   # 10, 12 and 20 bits: the package's own packing of padded samples (test_pcm.py covers it)
            _pcm[case.name] = pcm_bytes(as_int32(case.samples), E.Little, S.Signed, Pd.Msb, nbytes, case.bits)
    return _pcm[case.name], meta(E.Little, S.Signed, Pd.Msb, case.channels, nbytes, case.bits)


def model(case, max_po):
    if (case.name, max_po) not in _model:
        _model[case.name, max_po] = M.encode(case.samples, case.channels, case.bits, max_po)
    return _model[case.name, max_po]


def stream_of(block: bytes) -> bytes:
    return FL.FlacBlockDecompressor(block).stream


def explain(case, got: bytes, want) -> str:
    """The first frame at which ``got`` leaves the model's stream, and both parsed plans."""
    if got[:42] != want.stream[:42]:
        return f"{case.name}: stream headers differ: {got[:42].hex()} / {want.stream[:42].hex()}"
    for number, (pos, n) in enumerate(want.frames):
        if got[pos:pos + n] != want.stream[pos:pos + n]:
            break
    else:
        return f"{case.name}: {len(got)} bytes, model {len(want.stream)}"
    try:
        plans = []
        f = R.frame_at(got, pos, case.channels, case.bits, plans=plans)
        seen = f"assignment {f.assignment}, {f.length} bytes, {plans}"
    except (R.FlacError, IndexError) as e:
        seen = f"does not parse: {e}"
    return (f"{case.name} {case.aim}: frame {number} at byte {pos} differs\n  GPU:   {seen}\n"
            f"  model: assignment {want.plans[number][0]}, {n} bytes, {want.plans[number][1]}")


def compare(cases, streams, max_po):
    wrong = [explain(c, s, model(c, max_po)) for c, s in zip(cases, streams) if s != model(c, max_po).stream]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ from the model:\n" + "\n".join(wrong[:6])


@pytest.mark.parametrize("level", [0, 1, 2])
def test_fixed_levels_write_the_models_bytes(level):
    """All cases in one compress_many, and once more in reversed order (a frame's slot and its neighbours in the
    launch change, its bytes must not)."""
    comp = FL.FlacBlockCompressor(level)
    for cases in (K.CASES, K.CASES[::-1]):
        blocks = comp.compress_many([item(c) for c in cases])
        compare(cases, [stream_of(b) for b in blocks], M.LEVEL_MAX_PO[level])


@pytest.mark.parametrize("level", [0, 1, 2])
def test_block_size_edges_one_block_at_a_time(level):
    """rpp_flac_encode_ex on its own for every block-size edge: frames of 1 to 4096 samples, one and two frames."""
    comp = FL.FlacBlockCompressor(level)
    cases = [K.BY_NAME[n] for n in K.EDGE_NAMES]
    assert len(cases) == 20
    compare(cases, [stream_of(comp.compress(*item(c))) for c in cases], M.LEVEL_MAX_PO[level])


def test_frame_numbers_past_2048():
    """2050 frames of 8-bit mono, audio in the last four: the coded frame number grows to two bytes at 128 and to
    three at 2048.  Every frame is compared."""
    case = K.frame_number_case()
    want = M.encode(case.samples, case.channels, case.bits, M.LEVEL_MAX_PO[0])
    got = stream_of(FL.FlacBlockCompressor(0).compress(*item(case)))
    assert len(want.frames) == 2050
    assert got == want.stream, explain(case, got, want)


def check_lpc_level(case, stream, level):
    """The claims of the module docstring for one stream of a level with LPC; returns the kinds it saw."""
    max_po, max_lpc = M.LEVEL_MAX_PO[level], M.LEVEL_MAX_LPC[level]
    want = model(case, max_po)
    assert stream[:42] == want.stream[:42]
    frames, plans = R.walk_plans(stream)
    assert len(frames) == len(want.frames) and all(f.crc8_ok and f.crc16_ok for f in frames)
    kinds = set()
    for number, (f, subs) in enumerate(zip(frames, plans)):
        where = (case.name, level, number)
        coded = K.coded_sources(case, f.assignment, number)
        assert len(coded) == len(subs), where
        if case.channels == 2 and case.bits < 32:
            assert f.assignment in (1, 8, 9, 10), where
            assert sum(p.bits for p in subs) <= sum(p.bits for p in want.plans[number][1]), where
        else:
            assert f.assignment == case.channels - 1, where
        for p, (src, width) in zip(subs, coded):
            kinds.add(p.kind)
            plain = M.plan_subframe(src, width, max_po)
            if p.kind != "lpc":
                assert (p.kind, p.order, p.wasted, p.partition_order, p.method, p.params, p.bits) == \
                       (plain.kind, plain.order, plain.wasted, plain.partition_order, plain.method, plain.params,
                        plain.bits), (where, p, plain)
                continue
            bs, b = f.blocksize, width - p.wasted
            assert 1 <= p.order <= max_lpc and p.order < bs, (where, p)
            assert p.wasted == M.wasted_bits(src, width), (where, p)
            assert p.precision == M.lpc_precision(b, bs) and 0 <= p.shift <= 15, (where, p)
            assert all(-(1 << (p.precision - 1)) <= c < 1 << (p.precision - 1) for c in p.coefs), (where, p)
            res = M.lpc_residuals(src >> p.wasted, p.coefs, p.shift)
            rice = M.rice_plan_of(res, p.order, bs, max_po)
            assert rice is not None, (where, "an LPC residual outside the legal range")
            po, method, ks, rbits = rice
            assert (p.partition_order, p.method, p.params) == (po, method, ks), (where, p, rice)
            assert p.bits == 8 + p.wasted + p.order * b + 4 + 5 + p.order * p.precision + rbits, (where, p, rice)
            assert p.bits < plain.bits, (where, p, plain)
    assert R.decode(stream) == case.samples.tolist(), (case.name, level)
    return kinds


@pytest.mark.parametrize("level,exhaustive", [(3, False), (5, False), (8, False), (5, True)])
def test_lpc_levels_against_the_model(level, exhaustive):
    ar = ar_case()
    cases = K.CASES + [ar]
    blocks = FL.FlacBlockCompressor(level, exhaustive).compress_many([item(c) for c in cases])
    seen = {}
    for c, b in zip(cases, blocks):
        seen[c.name] = check_lpc_level(c, stream_of(b), level)
    # the LPC branch of the check ran: the all-pole input is coded by a linear predictor
    assert "lpc" in seen[ar.name], seen[ar.name]
    # and so did the other: noise, silence and polynomials stay with what the model chose
    assert seen["verbatim_16"] == {"verbatim"} and seen["all_zero"] == {"constant"}


def test_batch_encode_writes_nothing_past_its_total():
    """One direct rpp_flac_encode_batch call with the output buffer filled with 0xA5: blocks of different shapes,
    the reported offsets are the model's stream lengths, and every byte past the total is untouched."""
    names = ["bs_1", "bs_257", "bs_4097", "stereo_mid_side_16", "format_3ch_24bit", "verbatim_32", "k_outlier_runs",
             "res32_min_at_order_0", "format_8ch_12bit", "all_zero"]
    cases = [K.BY_NAME[n] for n in names]
    level = 2
    nb = len(cases)
    n = np.array([c.samples.size // c.channels for c in cases], np.uint64)
    ch = np.array([c.channels for c in cases], np.uint32)
    bp = np.array([c.bits for c in cases], np.uint32)
    vals = n * ch
    in_off = np.zeros(nb, np.uint64)
    in_off[1:] = np.cumsum(vals)[:-1]
    x = torch.from_numpy(np.concatenate([as_int32(c.samples) for c in cases])).to(DEV)
    L = N.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    frames = int(sum((int(v) + 4095) // 4096 for v in n))
    bound = max(int(L.rpp_flac_frame_bound(int(c), int(b))) for c, b in zip(ch, bp))
    guard = 4096
    out = torch.full((frames * bound + 64 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(nb + 1, dtype=torch.int64, device=DEV)
    ws_bytes = int(L.rpp_flac_encode_batch_workspace_bytes(nb, P(n), P(ch), P(bp)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream(DEV)
    st = L.rpp_flac_encode_batch(C.c_void_p(x.data_ptr()), nb, P(in_off), P(n), P(ch), P(bp), level, 0,
                                 C.c_void_p(out.data_ptr()), C.c_void_p(offs.data_ptr()), C.c_void_p(ws.data_ptr()),
                                 ws_bytes, C.c_void_p(s.cuda_stream))
    assert st == N.RPP_OK
    o = offs.cpu().numpy()
    host = out.cpu().numpy()
    want = [model(c, M.LEVEL_MAX_PO[level]).stream[42:] for c in cases]
    assert o.tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    total = int(o[-1])
    assert host[:total].tobytes() == b"".join(want)
    assert total < host.size - guard and bool((host[total:] == 0xA5).all())
