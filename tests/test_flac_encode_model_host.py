"""The FLAC encoder's model (flac_enc_model.py) and its inputs (flac_enc_cases.py) on the CPU.

test_gpu_flac_encode_constructed.py holds the GPU encoder to the model's bytes; here the model is held to the
format and to itself.  For every case at levels 0, 2 and 5 (fixed predictors only: level 5 lends its partition
cap) the model's stream parses under the independent RFC 9639 reader (flac_ref.py), decodes to the input under
that reader and under the CPU restatement (oracle/flac_oracle.c), the plans read back from the stream are the
plans the model intended, every plan's ``bits`` is the written subframe's length, and the case's aim holds: a
case that misses the decision it exists for fails here, not silently on the GPU.
"""

import numpy as np
import pytest

import flac_build as B
import flac_enc_cases as K
import flac_enc_model as M
import flac_ref as R
from oracle import flac as F

NAMES = [c.name for c in K.CASES]
_enc = {}


def encoded(case, level):
    key = (case.name, level)
    if key not in _enc:
        _enc[key] = M.encode(case.samples, case.channels, case.bits, M.LEVEL_MAX_PO[level])
    return _enc[key]


def as_int32(samples):
    return (np.asarray(samples, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def same_plan(read: R.SubframePlan, meant: M.Plan) -> bool:
    return (read.kind, read.order, read.wasted, read.partition_order, read.method, read.params, read.bits) == \
           (meant.kind, meant.order, meant.wasted, meant.partition_order, meant.method, meant.params, meant.bits)


def check_stream(case, e, decode=True):
    info = R.parse_streaminfo(e.stream)
    n = case.samples.size // case.channels
    assert (info.min_blocksize, info.max_blocksize, info.sample_rate) == (M.BLOCK, M.BLOCK, 48000)
    assert (info.channels, info.bits, info.total_samples, info.frames_at) == (case.channels, case.bits, n, 42)
    frames, plans = R.walk_plans(e.stream, info)
    assert [(f.pos, f.length) for f in frames] == e.frames
    assert all(f.crc8_ok and f.crc16_ok and not f.variable for f in frames)
    assert [f.blocksize for f in frames] == [min(M.BLOCK, n - at) for at in range(0, n, M.BLOCK)]
    assert [f.size_code for f in frames] == [B.SIZE_CODES.get(case.bits, 0)] * len(frames)
    for f, read, (code, meant) in zip(frames, plans, e.plans):
        assert f.assignment == code and len(read) == len(meant)
        assert all(same_plan(a, b) for a, b in zip(read, meant)), (f.coded, read, meant)
    if decode:
        assert R.decode(e.stream) == case.samples.tolist()
    status, y, ch, b = F.decode(e.stream, case.samples.size)
    assert status == F.OK and (ch, b) == (case.channels, case.bits)
    assert np.array_equal(y, as_int32(case.samples))


def test_the_case_list_covers_the_issue():
    kinds = {c.aim[0] for c in K.CASES}
    assert kinds >= {"blocksize", "order", "order_tie", "po_by_level", "po_order4", "k_all", "k_method", "unary_run",
                     "wasted", "constant_wasted", "kind", "assignment_strict", "assignment_tie", "assignment",
                     "side_25_bits", "orders_illegal", "res_extreme", "res_min_skipped", "format"}
    assert [c.aim[1] for c in K.CASES if c.aim[0] == "blocksize"] == list(K.EDGE_SIZES)
    assert sorted(c.aim[1] for c in K.CASES if c.aim[0] == "order") == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    for bits in (16, 24):
        strict = {c.aim[1] for c in K.CASES if c.aim[0] == "assignment_strict" and c.bits == bits}
        assert strict == {1, 8, 9, 10}
    assert {c.channels for c in K.CASES} >= {1, 2, 3, 8} and {c.bits for c in K.CASES} >= {8, 10, 12, 16, 20, 24, 32}
    assert all(c.samples.size // c.channels <= 2 * M.BLOCK for c in K.CASES)


def test_level_tables_and_header_codes():
    assert M.LEVEL_MAX_PO == (3, 3, 3, 4, 4, 5, 5, 5, 5) and M.LEVEL_MAX_LPC == (0, 0, 0, 6, 8, 8, 8, 12, 12)
    assert [M.bs_code(n) for n in (1, 192, 255, 256, 257, 576, 1152, 2304, 4608, 4096, 4095, 512, 32768, 65536)] == \
           [6, 1, 6, 8, 7, 2, 3, 4, 5, 12, 7, 9, 15, 7]
    assert [M.lpc_precision(b, n) for b, n in ((8, 4096), (12, 64), (15, 4096), (16, 192), (16, 193), (16, 4096),
                                               (16, 4609), (17, 384), (24, 1152), (24, 4096), (33, 4096))] == \
           [6, 8, 9, 7, 8, 12, 13, 13, 14, 15, 15]
    assert M.rice_plan_of([0, -(1 << 31)], 0, 2, 0) is None and M.rice_plan_of([0, 1 << 31], 0, 2, 0) is None
    assert M.rice_plan_of([0, -(1 << 31) + 1, (1 << 31) - 1, 0], 0, 4, 0) == (0, 1, (30,), 6 + 5 + 2 * 31 + 2 * 34)


@pytest.mark.parametrize("name", NAMES)
def test_case_at_every_level(name):
    case = K.BY_NAME[name]
    levels = K.LEVELS + ((4,) if case.aim[0].startswith("po_") else ())
    enc = {level: encoded(case, level) for level in levels}
    K.check_aim(case, enc)
    for level in levels:
        check_stream(case, enc[level])
    assert enc[0].stream == encoded(case, 1).stream == enc[2].stream  # levels 0-2 differ in nothing the encoder uses


def test_frame_numbers_past_2048():
    """2050 frames: one- , two- and three-byte coded numbers.  (The reader's sample-keeping decode is left to the
    small cases: here every frame is walked, its plan compared, and the restatement decodes all of it.)"""
    case = K.frame_number_case()
    e = M.encode(case.samples, case.channels, case.bits, M.LEVEL_MAX_PO[0])
    K.check_aim(case, {0: e})
    check_stream(case, e, decode=False)
    lens = {n: len(B.utf8(n)) for n in (0, 127, 128, 2047, 2048, 2049)}
    assert lens == {0: 1, 127: 1, 128: 2, 2047: 2, 2048: 3, 2049: 3}
    for n, want in lens.items():
        pos = e.frames[n][0]
        h = R.parse_header(e.stream, pos)
        assert h.coded == n and h.length == 4 + want + 1


def test_reader_refuses_a_residual_of_the_most_negative_value():
    """RFC 9639 section 9.2.7.3: a residual of -2^31 is not allowed.  A hand-built fixed order-0 subframe that
    carries it (the writer asked to allow it) is refused by walk and by decode; one step inside the range passes."""
    def built(value):
        x = [7, value, -3] + [1, -1] * 7 + [0]
        f = B.frame(18, [B.fixed(0, x, B.Residual(1, 0, (29,)))], 32, bs_code=6, allow_wide=True)
        return B.stream(1, 32, [f]).data, x
    good, x = built(-(1 << 31) + 1)
    assert R.decode(good) == x and len(R.walk_frames(good)) == 1
    bad, _ = built(-(1 << 31))
    for reader in (R.decode, R.walk_frames, R.walk_plans):
        with pytest.raises(R.FlacError, match="9.2.7.3"):
            reader(bad)
    # at order 1: samples that fit, a difference that does not
    x = [1 << 30, -(1 << 30)] + [-(1 << 30)] * 14
    f = B.frame(16, [B.fixed(1, x, B.Residual(1, 0, (28,)))], 32, bs_code=6, allow_wide=True)
    with pytest.raises(R.FlacError, match="9.2.7.3"):
        R.decode(B.stream(1, 32, [f]).data)


def test_walk_plans_reads_an_lpc_subframe():
    x = [3, -4, 9, 2, -7, 5, 0, 1] * 4
    res = B.Residual(0, 1, (3, 2))
    f = B.frame(32, [B.lpc(2, 7, 4, (21, -9), x, res, wasted=0), B.constant([40] * 32, 3)], 16, bs_code=6)
    frames, plans = R.walk_plans(B.stream(2, 16, [f]).data)
    a, b = plans[0]
    assert (a.kind, a.order, a.partition_order, a.method, a.params) == ("lpc", 2, 1, 0, (3, 2))
    assert (a.precision, a.shift, a.coefs) == (7, 4, (21, -9))
    assert (b.kind, b.wasted, b.bits) == ("constant", 3, 8 + 3 + 13)
    m = f.marks[0]
    assert a.bits == m.end - m.start and frames[0].crc16_ok
