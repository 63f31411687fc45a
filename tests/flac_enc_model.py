"""The FLAC encoder's choices restated in plain Python/numpy, for the tests only.

Written from the rules the encoder documents (the header comment of dwarfs_amd/csrc/flac_kernels.hip) and from
RFC 9639, not from the kernel's data structures: whole-array integer arithmetic in int64 (a 32-bit sample's
fourth difference needs 36 bits, a 25-bit side value less) and Python ints for the sums.  Without LPC (libFLAC's
levels 0-2, or any level's partition cap with ``lpc`` left out) every step from samples to bytes is integer, so
``encode`` gives the exact stream the encoder must write.  From level 3 the encoder's tukey window runs in float
and its coefficients are not predicted here; ``rice_plan_of`` and ``lpc_residuals`` pin what follows the
coefficients read back from a stream.

The rules:

* a subframe: wasted bits = the trailing zeros of the OR of its samples (at most sbps - 1); constant when all
  samples are equal; else verbatim is the bar, and the fixed order 0..4 (below the block size, every residual
  legal) with the smallest sum of |residual| (ties: the lower order) replaces it when strictly cheaper;
* a legal residual r has -2^31 < r <= 2^31 - 1 (RFC 9639 section 9.2.7.3 excludes the most negative value);
* the Rice plan: partition orders 0..min(cap, pomax) with 2^po dividing the block and a first partition longer
  than the predictor order; per partition k = min(floor(log2(sum // count)), 30), 0 for a zero mean; a code
  costs (u >> k) + 1 + k; 5-bit parameters as soon as one k exceeds 14; fewest bits, ties to the lower order;
* two channels below 32 bits: the cheapest of left/right, left/side, side/right, mid/side, ties in that order.

The bytes come from the field-by-field writer (flac_build.py); this file only decides.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

import flac_build as B

BLOCK = 4096  # samples per frame and channel (libFLAC's level-5 block size; the encoder uses it at every level)
RATE_CODE = 10  # 48 kHz
MAX_PO = 5  # the project's cap on the partition order

# libFLAC's presets -0 .. -8: -r (max Rice partition order, capped at MAX_PO) and -l (max LPC order)
LEVEL_MAX_PO = tuple(min(v, MAX_PO) for v in (3, 3, 3, 4, 4, 5, 6, 6, 6))
LEVEL_MAX_LPC = (0, 0, 0, 6, 8, 8, 8, 12, 12)

RES_MIN, RES_MAX = -(1 << 31) + 1, (1 << 31) - 1

ASSIGNMENTS = {1: None, 8: "left_side", 9: "right_side", 10: "mid_side"}


def lpc_precision(bps: int, bs: int) -> int:
    """libFLAC's automatic coefficient precision (qlp_coeff_precision 0), capped at the 15 bits the format
    holds: by the sample depth below 16 bits, by the block size from there."""
    if bps < 16:
        p = max(5, 2 + bps // 2)
    elif bps == 16:
        p = next((v for lim, v in ((192, 7), (384, 8), (576, 9), (1152, 10), (2304, 11), (4608, 12)) if bs <= lim), 13)
    else:
        p = 13 if bs <= 384 else 14 if bs <= 1152 else 15
    return min(p, 15)


def bs_code(bs: int) -> int:
    """The block-size code: a named size where there is one, else the 8-bit field up to 256, else the 16-bit."""
    if bs == 192:
        return 1
    for c in range(2, 6):
        if bs == 576 << (c - 2):
            return c
    for c in range(8, 16):
        if bs == 256 << (c - 8):
            return c
    return 6 if bs <= 256 else 7


class Plan(NamedTuple):
    kind: str             # "constant", "verbatim", "fixed"
    wasted: int
    order: int
    partition_order: int
    method: int
    params: tuple         # k per partition
    bits: int             # the whole subframe


def _ctz(v: int) -> int:
    return (v & -v).bit_length() - 1


def legal(res) -> bool:
    res = np.asarray(res, dtype=np.int64)
    return bool(res.size == 0 or (int(res.min()) >= RES_MIN and int(res.max()) <= RES_MAX))


def rice_plan_of(residuals, order: int, bs: int, max_po: int):
    """(partition order, method, (k, ...), bits) of the bs - order residuals of a predictor of ``order``; bits
    counts the residual section from its 6-bit header.  None when a residual is not legal."""
    res = np.asarray(residuals, dtype=np.int64)
    assert res.size == bs - order and 0 <= order < bs
    if not legal(res):
        return None
    u = np.where(res >= 0, 2 * res, -2 * res - 1)
    padded = np.concatenate([np.zeros(order, np.int64), u])  # (the warm-up samples: no code, taken out below)
    pomax = 0
    while pomax < max_po and bs % (2 << pomax) == 0 and (bs >> (pomax + 1)) > order:
        pomax += 1
    best = None
    for po in range(pomax + 1):
        parts = padded.reshape(1 << po, bs >> po)
        ks, codes = [], 0
        for p, row in enumerate(parts):
            skip = order if p == 0 else 0
            mean = int(row.sum()) // (row.size - skip)
            k = min(mean.bit_length() - 1, 30) if mean else 0
            ks.append(k)
            codes += int((row[skip:] >> k).sum()) + (row.size - skip) * (1 + k)
        method = 1 if max(ks) > 14 else 0
        total = 6 + (1 << po) * (5 if method else 4) + codes
        if best is None or total < best[3]:
            best = (po, method, tuple(ks), total)
    return best


def fixed_residuals(s, order: int):
    """The order-th backward difference of s from sample ``order`` on (RFC 9639 section 9.2.5)."""
    return np.diff(np.asarray(s, dtype=np.int64), n=order)


def lpc_residuals(s, coefs, shift: int):
    """sample - (sum coefs[j] * s[i - 1 - j] >> shift) from sample len(coefs) on (section 9.2.6).  In int64:
    up to 32 products of a 15-bit coefficient and a 33-bit sample stay below 2^53."""
    s = np.asarray(s, dtype=np.int64)
    o, n = len(coefs), s.size
    assert all(-(1 << 14) <= int(c) < 1 << 14 for c in coefs) and int(np.abs(s).max()) <= 1 << 32 and o <= 32
    pred = np.zeros(n - o, np.int64)
    for j, c in enumerate(coefs):
        pred += int(c) * s[o - 1 - j:n - 1 - j]
    return s[o:] - (pred >> shift)


def wasted_bits(samples, sbps: int) -> int:
    orv = int(np.bitwise_or.reduce(np.asarray(samples, dtype=np.int64)))
    return min(_ctz(orv), sbps - 1) if orv else 0


def plan_subframe(samples, sbps: int, max_po: int) -> Plan:
    """The cheapest constant, verbatim or fixed subframe of ``samples`` (``sbps`` bits each)."""
    x = np.asarray(samples, dtype=np.int64)
    bs = x.size
    wasted = wasted_bits(x, sbps)
    b = sbps - wasted
    head = 8 + wasted  # the type byte and the unary count of wasted bits
    if int(x.min()) == int(x.max()):
        return Plan("constant", wasted, 0, 0, 0, (), head + b)
    plan = Plan("verbatim", wasted, 0, 0, 0, (), head + b * bs)
    s = x >> wasted
    order, fewest = None, None
    for o in range(min(5, bs)):
        r = fixed_residuals(s, o)
        if not legal(r):
            continue
        total = int(np.abs(r).sum())
        if fewest is None or total < fewest:
            order, fewest = o, total
    if order is not None:
        po, method, ks, rbits = rice_plan_of(fixed_residuals(s, order), order, bs, max_po)
        bits = head + order * b + rbits
        if bits < plan.bits:
            plan = Plan("fixed", wasted, order, po, method, ks, bits)
    return plan


def stereo_sources(left, right):
    """left, right, side = left - right (one bit wider), mid = (left + right) >> 1."""
    l, r = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    return l, r, l - r, (l + r) >> 1


# per assignment code: the two coded sources (indexes into stereo_sources) in stream order
STEREO_ORDER = ((1, (0, 1)), (8, (0, 2)), (9, (2, 1)), (10, (3, 2)))


def plan_frame(channels, bps: int, max_po: int):
    """(assignment code, [(plan, samples, sbps)] in stream order) for one frame's per-channel sample arrays."""
    if len(channels) == 2 and bps < 32:
        src = stereo_sources(*channels)
        plans = [plan_subframe(s, bps + (1 if i == 2 else 0), max_po) for i, s in enumerate(src)]
        best = None
        for code, (a, b) in STEREO_ORDER:
            total = plans[a].bits + plans[b].bits
            if best is None or total < best[0]:
                best = (total, code, (a, b))
        _, code, pair = best
        return code, [(plans[i], src[i], bps + (1 if i == 2 else 0)) for i in pair]
    return len(channels) - 1, [(plan_subframe(c, bps, max_po), np.asarray(c, dtype=np.int64), bps) for c in channels]


def subframe_of(plan: Plan, samples) -> B.Sub:
    s = [int(v) for v in samples]
    if plan.kind == "constant":
        return B.constant(s, plan.wasted)
    if plan.kind == "verbatim":
        return B.verbatim(s, plan.wasted)
    return B.fixed(plan.order, s, B.Residual(plan.method, plan.partition_order, plan.params), plan.wasted)


def write_frame(number: int, bps: int, assignment: int, subs) -> bytes:
    """The frame's bytes: header (fixed blocking, 48 kHz, the block-size code of bs_code, sample-size code 0
    for a depth the table lacks, the UTF-8 coded number, CRC-8), subframes, zero padding, CRC-16.  ``subs``:
    plan_frame's list.  Every plan's ``bits`` must be what the writer lays down."""
    bs = len(subs[0][1])
    f = B.frame(bs, [subframe_of(p, s) for p, s, _ in subs], bps, bs_code=bs_code(bs), rate_code=RATE_CODE,
                size_code=B.SIZE_CODES.get(bps, 0), assignment=ASSIGNMENTS[assignment] if len(subs) == 2 else None,
                number=number)
    for (p, _, _), m in zip(subs, f.marks):
        assert m.end - m.start == p.bits, (p, m.end - m.start)
    return f.data


def stream_header(channels: int, bps: int, total: int) -> bytes:
    """fLaC and the STREAMINFO the project writes: block sizes 4096..4096, frame sizes unknown, 48 kHz, no MD5."""
    v = (BLOCK << 128) | (BLOCK << 112) | (48000 << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(18, "big") + bytes(16)


class Encoded(NamedTuple):
    stream: bytes
    frames: list   # (byte position in stream, byte length)
    plans: list    # per frame (assignment code, [Plan per subframe in stream order])


def encode(samples, channels: int, bps: int, max_po: int) -> Encoded:
    """The stream of interleaved ``samples`` with fixed predictors only and partition orders up to ``max_po``."""
    x = np.asarray(samples, dtype=np.int64).reshape(-1, channels)
    out = bytearray(stream_header(channels, bps, x.shape[0]))
    frames, plans = [], []
    for number, at in enumerate(range(0, x.shape[0], BLOCK)):
        block = x[at:at + BLOCK]
        code, subs = plan_frame([block[:, c] for c in range(channels)], bps, max_po)
        data = write_frame(number, bps, code, subs)
        frames.append((len(out), len(data)))
        plans.append((code, [p for p, _, _ in subs]))
        out += data
    return Encoded(bytes(out), frames, plans)
