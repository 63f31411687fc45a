"""Inputs for the FLAC encoder, each aimed at one of its decisions (test_flac_encode_model_host.py,
test_gpu_flac_encode_constructed.py).

A case is (name, channels, bits, samples, aim): interleaved samples of one or two 4096-sample frames and the
feature of the plan (flac_enc_model.py) the case exists for.  ``check_aim`` asserts that the model's own plan has
that feature, so a case that drifts off its aim fails on the CPU instead of passing vacuously on the GPU.
Block sizes are per channel.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

import flac_enc_model as M

LEVELS = (0, 2, 5)  # the partition caps 3, 3 and 5 (level 4's cap of 4 is run for the partition cases)


class Case(NamedTuple):
    name: str
    channels: int
    bits: int
    samples: np.ndarray  # interleaved, int64
    aim: tuple


CASES: list = []
EDGE_SIZES = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 192, 255, 256, 257, 576, 1152, 4095, 4096, 4097, 8192)


def rng(seed):
    return np.random.default_rng(seed)


def add(name, channels, bits, samples, aim):
    x = np.asarray(samples, dtype=np.int64)
    if x.ndim == 2:  # [sample, channel]
        assert x.shape[1] == channels
        x = x.reshape(-1)
    assert x.size and x.size % channels == 0 and x.size // channels <= 2 * M.BLOCK, name
    assert -(1 << (bits - 1)) <= int(x.min()) and int(x.max()) < 1 << (bits - 1), name
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, channels, bits, x, aim))


def noise(r, n, amp):
    """Uniform in [-amp, amp]."""
    return r.integers(-amp, amp + 1, n)


# ---- block-size edges: orders below the block size, pomax 0, the named size codes, the 8/16-bit size field ----
for _n in EDGE_SIZES:
    _r = rng(100 + _n)
    add(f"bs_{_n}", 1, 16, 1000 + np.cumsum(noise(_r, _n, 20)) + noise(_r, _n, 2), ("blocksize", _n))


# ---- each fixed order the winner: a polynomial of degree d - 1 plus noise of +-2 ----
# The (d-1)-th difference of the polynomial is the constant _LEAD[d], about twice the deviation of the noise's
# d-th difference, so order d - 1 pays for it at every sample and order d + 1 only roughens the noise.
_LEAD = (0, 1000, 8, 14, 24)


def binom_poly(n, d, centre):
    """lead * C(i - centre, d - 1): integer valued, (d-1)-th difference = lead."""
    i = np.arange(n, dtype=np.int64) - centre
    if d == 0:
        return np.zeros(n, np.int64)
    p = np.ones(n, dtype=object)
    for j in range(d - 1):
        p = p * (i.astype(object) - j)
    for j in range(2, d):
        p = p // j
    return (p * _LEAD[d]).astype(np.int64)


def spline(n, seg, lead):
    """A piecewise cubic: third difference +lead, -lead, -lead, +lead over segments of ``seg`` samples, so the
    value grows only linearly with the length (one cubic with a third difference of 24 leaves 32 bits after
    about 1500 samples); its fourth difference is zero except at the knots."""
    d3 = np.repeat(np.tile([1, -1, -1, 1], n // (4 * seg) + 1), seg)[:n] * lead
    return np.cumsum(np.cumsum(np.cumsum(d3)))


for _d in range(5):
    add(f"order_{_d}_bs64", 1, 24, binom_poly(64, _d, 32) + noise(rng(200 + _d), 64, 2), ("order", _d))
    _p = spline(4096, 128, _LEAD[4]) if _d == 4 else binom_poly(4096, _d, 2048)
    add(f"order_{_d}_bs4096", 1, 32, _p + noise(rng(210 + _d), 4096, 2), ("order", _d))


def _order_tie():
    """32 small samples whose orders 0 and 1 have the same sum of |residual|, below every other order's."""
    for seed in range(10000):
        x = rng(seed).integers(-3, 4, 32)
        s = [int(np.abs(M.fixed_residuals(x, o)).sum()) for o in range(5)]
        if s[0] == s[1] and s[0] < min(s[2:]):
            return x
    raise AssertionError("no tie found")


add("order_tie_0_1", 1, 16, _order_tie(), ("order_tie", (0, 1)))


# ---- partition order ----
def stepped(r, n, seg, amps):
    a = np.repeat(r.choice(amps, n // seg + 1), seg)[:n]
    return (r.random(n) * 2 - 1) * a


_AMPS = (3, 40, 700, 9000)
add("po_steps_128", 1, 16, np.rint(stepped(rng(300), 4096, 128, _AMPS)), ("po_by_level", {2: 3, 4: 4, 5: 5}))
add("po_flat", 1, 16, noise(rng(301), 4096, 48), ("po_by_level", {2: 0, 4: 0, 5: 0}))
# (bs >> po) > order binds: bs 64 and order 4 allow po 3 (8 > 4) but not 4; bs 32 allows only po 2
for _n, _po in ((64, {2: 3, 4: 3, 5: 3}), (32, {2: 2, 4: 2, 5: 2})):
    _x = binom_poly(_n, 4, _n // 2) * 100 + np.rint(stepped(rng(302 + _n), _n, 4, (2, 150)))
    add(f"po_order4_bs{_n}", 1, 32, _x, ("po_order4", _po))


# ---- Rice parameters ----
add("k_zero", 1, 16, rng(400).choice([0, 0, 0, 0, 1, -1], 4096), ("k_all", 0))
add("k_14_only", 1, 24, noise(rng(401), 4096, 24000), ("k_method", ((14,), 0)))
add("k_14_and_15", 1, 24, np.concatenate([noise(rng(402), 2048, 24000), noise(rng(403), 2048, 48000)]),
    ("k_method", ((14, 15), 1)))
# one partition of samples of magnitude 2^30 and more (folded: 2^31 and more, log2 = 31), the rest quiet
_r = rng(404)
_x = noise(_r, 4096, 30)
_x[:512] = ((1 << 30) + _r.integers(1, 1000, 512)) * _r.choice([-1, 1], 512)
add("k_clamp_30", 1, 32, _x, ("k_method", ((30,), 1)))
# a quiet block with outliers whose unary runs are hundreds of zeros: the last sample of a 64-sample row, the
# first of the next, and one inside a row (with 128-sample partitions, level 5, two outliers share a partition
# and raise its parameter: the runs are shorter there, still longer than two 32-bit words)
_x = noise(rng(405), 4096, 2)
_x[[63, 64, 1000, 4095]] = (1200, -1500, 900, -1100)
add("k_outlier_runs", 1, 16, _x, ("unary_run", {0: 200, 2: 200, 5: 64}))


# ---- wasted bits ----
for _w in (1, 3):
    add(f"wasted_{_w}", 1, 16, noise(rng(500 + _w), 2000, 900) << _w | (1 << _w), ("wasted", (_w,)))
add("wasted_bps_minus_1", 1, 16, rng(503).choice([0, -32768], 1000), ("wasted", (15,)))
_x = np.stack([noise(rng(504), 1500, 8000) << 2, noise(rng(505), 1500, 32000) | 1], axis=1)
_x[0, 0] = 4
add("wasted_one_channel", 2, 16, _x, ("wasted", (2, 0)))
_x = np.zeros(1000, np.int64)
_x[100] = 96
add("wasted_all_zero_but_one", 1, 16, _x, ("wasted", (5,)))
add("wasted_constant", 1, 16, np.full(700, 80), ("constant_wasted", 4))
add("all_zero", 1, 16, np.zeros(4096 + 9, np.int64), ("constant_wasted", 0))


# ---- verbatim wins: uniform noise over the whole range ----
for _b in (8, 16, 32):
    add(f"verbatim_{_b}", 1, _b, rng(600 + _b).integers(-(1 << (_b - 1)), 1 << (_b - 1), 4096), ("kind", "verbatim"))


# ---- stereo ----
def smooth(n, amp, period, phase=0.0):
    return np.rint(amp * np.sin(2 * np.pi * np.arange(n) / period + phase)).astype(np.int64)


for _b, _s in ((16, 1), (24, 256)):
    _n = 4096
    _r = rng(700 + _b)
    _d1, _d2 = noise(_r, _n, 200 * _s), noise(_r, _n, 200 * _s)
    _big = smooth(_n, 8000 * _s, 400)
    # independent: uncorrelated noise, right a quarter of left's amplitude (side and mid both carry left's)
    add(f"stereo_independent_{_b}", 2, _b, np.stack([noise(_r, _n, 3000 * _s), noise(_r, _n, 750 * _s)], 1),
        ("assignment_strict", 1))
    # left/side: left smooth (order 2 removes it), right = left + white noise: side is the noise at order 0,
    # right and mid need order 2, which roughens the noise
    add(f"stereo_left_side_{_b}", 2, _b, np.stack([_big, _big + _d1], 1), ("assignment_strict", 8))
    add(f"stereo_side_right_{_b}", 2, _b, np.stack([_big + _d1, _big], 1), ("assignment_strict", 9))
    # mid/side: both channels the smooth part plus their own noise: mid halves the noise, side drops the smooth part
    add(f"stereo_mid_side_{_b}", 2, _b, np.stack([_big + _d1, _big + _d2], 1), ("assignment_strict", 10))
    # left == right: side is constant zero, mid equals left: three totals tie, left/side comes first
    add(f"stereo_equal_{_b}", 2, _b, np.stack([_big + _d1, _big + _d1], 1), ("assignment_tie", (8, (8, 9, 10))))
    # left silent, right in pairs (v, -v): side = -right has right's residual magnitudes partition by partition,
    # so independent and left/side tie exactly, and independent comes first
    _v = noise(_r, _n // 2, 900 * _s) | 1
    _pairs = np.stack([_v, -_v], 1).reshape(-1)
    add(f"stereo_tie_{_b}", 2, _b, np.stack([np.zeros(_n, np.int64), _pairs], 1), ("assignment_tie", (1, (1, 8))))
_x = smooth(3000, 1 << 29, 500) + noise(rng(720), 3000, 1000)
add("stereo_32_never_decorrelated", 2, 32, np.stack([_x, _x], 1), ("assignment", 1))
_x = rng(721).integers(-(1 << 23) + 1, 1 << 23, 4096)
_x[:2] = ((1 << 23) - 1, -(1 << 23) + 1)
add("stereo_24_opposite_full_scale", 2, 24, np.stack([_x, -_x], 1), ("side_25_bits", 10))


# ---- 32-bit mono: the residual limits ----
_FS = (1 << 31) - 1
_x = noise(rng(800), 4096, 50)
_x[1000:1008] = [_FS, -_FS] * 4
add("res32_alternating_full_scale", 1, 32, _x, ("orders_illegal", (0, (1, 2, 3, 4))))
_r = rng(801)
_x = _r.integers(-(1 << 29), 1 << 29, 4096)
_x[2000] = _FS
add("res32_max_at_order_0", 1, 32, _x, ("res_extreme", (0, _FS)))
_x = _r.integers(-(1 << 29), 1 << 29, 4096)
_x[1999:2002] = (1 << 28, -(1 << 31), 1 << 28)
add("res32_min_at_order_0", 1, 32, _x, ("res_min_skipped", 0))
# a walk of small steps at +2^30 that drops to -2^30 in one step of exactly -2^31 (the steps around it are -5,
# so the second difference stays legal)
_steps = noise(rng(802), 4096, 40)
_steps[0] = 0
_steps[1999:2002] = (-5, 0, -5)
_x = (1 << 30) + np.cumsum(_steps)
_x[2000:] += -(1 << 31) - (_x[2000] - _x[1999])
add("res32_min_at_order_1", 1, 32, _x, ("res_min_skipped", 1))


# ---- formats ----
def tone(r, n, channels, bits):
    amp = (1 << (bits - 2)) - 1
    cols = [smooth(n, amp, 90 + 37 * c, c) + noise(r, n, max(1, amp >> 6)) for c in range(channels)]
    return np.stack(cols, 1)


for _c, _b, _n in ((3, 8, 700), (8, 12, 300), (1, 20, 900), (2, 20, 900), (8, 16, 520), (1, 10, 800), (2, 10, 800),
                   (3, 32, 600), (3, 24, 4096 + 50), (2, 12, 333), (1, 24, 100)):
    add(f"format_{_c}ch_{_b}bit", _c, _b, tone(rng(900 + 10 * _c + _b), _n, _c, _b), ("format", (_c, _b)))

BY_NAME = {c.name: c for c in CASES}
EDGE_NAMES = [f"bs_{n}" for n in EDGE_SIZES]


def frame_number_case() -> Case:
    """Mono 8-bit silence with audio in frames 2046-2049: 2050 frames, the coded number takes a third byte
    from 2048 on (and a second from 128).  About 8 MiB of samples; built on demand."""
    x = np.zeros(2050 * M.BLOCK, np.int64)
    at = 2046 * M.BLOCK
    x[at:] = smooth(4 * M.BLOCK, 90, 300) + noise(rng(1000), 4 * M.BLOCK, 3)
    return Case("frame_numbers_2050", 1, 8, x, ("frames", 2050))


# ---- the aims ----
def sources_of(case: Case, frame: int = 0):
    """Per-channel arrays of one frame, and for stereo below 32 bits the four sources and their widths."""
    x = case.samples.reshape(-1, case.channels)[frame * M.BLOCK:(frame + 1) * M.BLOCK]
    chans = [x[:, c] for c in range(case.channels)]
    if case.channels == 2 and case.bits < 32:
        return list(M.stereo_sources(*chans)), [case.bits, case.bits, case.bits + 1, case.bits]
    return chans, [case.bits] * case.channels


def coded_sources(case: Case, assignment: int, frame: int = 0):
    """[(samples, width)] of the frame's subframes in stream order under ``assignment``."""
    src, widths = sources_of(case, frame)
    if case.channels == 2 and case.bits < 32:
        pair = dict(M.STEREO_ORDER)[assignment]
        return [(src[i], widths[i]) for i in pair]
    return list(zip(src, widths))


def check_aim(case: Case, enc: dict):
    """``enc``: level -> flac_enc_model.Encoded of the case (at least LEVELS; 4 as well for po_by_level)."""
    kind, want = case.aim
    for level, e in enc.items():
        code0, plans0 = e.plans[0]
        p = plans0[0]
        src, widths = sources_of(case)
        max_po = M.LEVEL_MAX_PO[level]
        if kind == "blocksize":
            sizes = [min(M.BLOCK, want - at) for at in range(0, want, M.BLOCK)]
            assert len(e.plans) == len(sizes) and case.samples.size == want
            last = e.plans[-1][1][0]
            assert last.order < sizes[-1] and (last.kind == "constant") == (sizes[-1] == 1)
            if sizes[-1] >= 16:
                assert last.kind == "fixed", (want, last)
        elif kind == "order":
            assert p.kind == "fixed" and p.order == want, p
        elif kind == "order_tie":
            s = [int(np.abs(M.fixed_residuals(src[0], o)).sum()) for o in range(5)]
            assert s[want[0]] == s[want[1]] == min(s) and p.kind == "fixed" and p.order == want[0], (s, p)
        elif kind == "po_by_level":
            if level in want:
                assert p.kind == "fixed" and p.partition_order == want[level], (level, p)
        elif kind == "po_order4":
            if level in want:
                assert p.kind == "fixed" and p.order == 4 and p.partition_order == want[level], (level, p)
                if level == 5:  # the cap allows more: only the first partition's length holds it back
                    assert want[level] < max_po and (src[0].size >> (want[level] + 1)) <= 4
        elif kind == "k_all":
            assert p.kind == "fixed" and set(p.params) == {want} and p.method == 0, p
        elif kind == "k_method":
            ks, method = want
            assert p.kind == "fixed" and set(ks) <= set(p.params) and max(p.params) == max(ks), p
            assert p.method == method
        elif kind == "unary_run":
            assert p.kind == "fixed"
            res = np.concatenate([np.zeros(p.order, np.int64), M.fixed_residuals(src[0] >> p.wasted, p.order)])
            u = np.where(res >= 0, 2 * res, -2 * res - 1)
            per = u.size >> p.partition_order
            runs = np.array([int(v) >> p.params[i // per] for i, v in enumerate(u)])
            long = np.flatnonzero(runs >= want[level])
            assert {63, 64} <= set(long.tolist()) and any(i % 64 not in (0, 63) for i in long), long
        elif kind == "wasted":
            assert tuple(q.wasted for q in plans0) == want and code0 == len(want) - 1, (code0, plans0)
            assert all(q.kind != "constant" for q in plans0)
        elif kind == "constant_wasted":
            assert all(pl[1][0].kind == "constant" and pl[1][0].wasted == want for pl in e.plans)
        elif kind == "kind":
            assert p.kind == want, p
        elif kind in ("assignment_strict", "assignment_tie", "side_25_bits"):
            bits = [M.plan_subframe(s, w, max_po).bits for s, w in zip(src, widths)]
            totals = {c: bits[a] + bits[b] for c, (a, b) in M.STEREO_ORDER}
            if kind == "assignment_strict":
                assert code0 == want and all(totals[want] < t for c, t in totals.items() if c != want), totals
            elif kind == "assignment_tie":
                code, tied = want
                assert code0 == code and len({totals[c] for c in tied}) == 1, totals
                assert all(totals[code] < t for c, t in totals.items() if c not in tied), totals
            else:
                assert code0 == want and int(np.abs(src[2]).max()) >= 1 << 23  # (past 24 bits)
                assert plans0[1].wasted == 1
        elif kind == "assignment":
            assert code0 == want
        elif kind == "orders_illegal":
            order, bad = want
            assert p.kind == "fixed" and p.order == order
            assert not any(M.legal(M.fixed_residuals(src[0], o)) for o in bad)
        elif kind == "res_extreme":
            order, value = want
            assert p.kind == "fixed" and p.order == order
            assert int(M.fixed_residuals(src[0], order).max()) == value
        elif kind == "res_min_skipped":
            # order `want` has the smallest sum of |residual| and holds a residual of exactly -2^31: it is skipped;
            # with that one residual one step inside the range it would be taken, and would beat verbatim
            s = [int(np.abs(M.fixed_residuals(src[0], o)).sum()) for o in range(5)]
            r = M.fixed_residuals(src[0], want)
            assert s[want] == min(s) and int(r.min()) == -(1 << 31) and int(r.max()) <= M.RES_MAX
            assert not (p.kind == "fixed" and p.order == want), p
            eased = r.copy()
            eased[eased == -(1 << 31)] += 1
            po, method, ks, rbits = M.rice_plan_of(eased, want, src[0].size, max_po)
            assert 8 + want * case.bits + rbits < 8 + case.bits * src[0].size
        elif kind == "format":
            assert (case.channels, case.bits) == want and len(plans0) == case.channels
            assert any(q.kind == "fixed" for q in plans0)
        elif kind == "frames":
            assert len(e.plans) == want
            assert all(pl[1][0].kind == "constant" for pl in e.plans[:2046])
            assert all(pl[1][0].kind == "fixed" for pl in e.plans[2046:])
        else:
            raise AssertionError(f"unknown aim {kind}")
