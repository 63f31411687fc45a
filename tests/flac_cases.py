"""The constructed FLAC cases, shared by the CPU and the GPU tests (test_flac_constructed_host.py,
test_gpu_flac_constructed.py).  Every stream is written field by field by flac_build.py.

The geometry cases aim at constants of the wave decoder (dwarfs_amd/csrc/flac_kernels.hip); they are restated
here once, and ``wave_model`` replays the decoder's window and round bookkeeping over the writer's recorded bit
positions, so that a case can assert which path it takes.  Bit positions count from the first frame's first
byte: the decoder's input starts there and is copied to an aligned buffer, so those are the kernel's positions.
"""

from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field

import flac_build as B

SEG_BITS = 32   # a lane's segment: `ss = ((pos >> 5) + lane) << 5`, flac_kernels.hip:1261
LANES = 64      # segments per round: kWave, flac_kernels.hip:62, used at :1260
FWIN = 512      # kFWin, LDS window words, flac_kernels.hip:1155
FLOOK = 64      # kFLook, words a round keeps past its lane segments, flac_kernels.hip:1156
WAVE_LDS = 144 * 1024  # kFlacWaveLds, flac_kernels.hip:65: 4 * (FWIN + 2) + 4 * channels * max_bs must fit


@dataclass
class Case:
    name: str
    family: str
    build: object            # bits -> B.Stream
    widths: tuple = (16, 32)
    check: object = None     # (stream, bits) -> None: the geometry assertions
    direct_only: bool = False  # block-size range too wide for the block decompressor's plan (see family p)
    wide: str = ""           # family h under allow_wide: "ok" (both CPU readers decode it) or "min" (a residual of
                             # -2^31: flac_ref.py refuses it by section 9.2.7.3, the restatement decodes it)


CASES: list = []
REFUSED: list = []


def case(name, family, widths=(16, 32), check=None, **kw):
    def deco(fn):
        CASES.append(Case(name, family, fn, tuple(widths), check, **kw))
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def built(name: str, bits: int) -> B.Stream:
    c = BY_NAME[name]
    return c.build(bits)


def ids(cases):
    return [(c.name, b) for c in cases for b in c.widths]


# ---- a model of the wave decoder's window and rounds over recorded positions ----

class Win:
    """win_cover (flac_kernels.hip:1174): the window holds words [W, W + FWIN)."""

    def __init__(self):
        self.W, self.reloads = None, []

    def cover(self, bit, words):
        wi = bit >> 5
        if self.W is not None and wi >= self.W and wi + words <= self.W + FWIN:
            return
        self.W = wi
        self.reloads.append(bit)


@dataclass
class Round:
    part: int
    pos: int        # where the round starts
    W: int          # the window's first word during the round
    first: int      # index of the round's first code in the subframe
    count: int      # codes taken
    reloaded: bool
    last: bool      # the partition ends in this round
    end_at_exit: bool = False  # ... and its last code is the last start in its lane's segment (r == cnt)
    tot_eq_need: bool = False  # ... and no later start lies in the round's 64 segments (tot == need)


@dataclass
class Model:
    rounds: list = field(default_factory=list)
    redo: bool = False
    redo_code: int = -1


def wave_model(st: B.Stream, fi=0, si=0) -> Model:
    """wave_subframe / wave_rice (flac_kernels.hip:1256-1334, :1345-1419) over a mono frame at byte 0 whose
    subframe is a fixed or LPC one without wasted bits: the header fields' ubits, then per partition the parameter
    and the rounds.  A needed code whose closing 1 bit lies outside the window hands the frame to the lane decoder."""
    assert fi == 0 and si == 0 and st.channels == 1
    m = st.marks[0][0]
    w, out = Win(), Model()
    w.cover(m.start, 2)
    ci = 0
    for p, ((ps, pe), first) in enumerate(zip(m.parts, m.first)):
        w.cover(ps, 2)
        ncodes = sum(1 for a, _ in m.codes[ci:] if a < pe and a >= first) if pe > first else 0
        codes = m.codes[ci:ci + ncodes]
        what, k = m.params[p]
        if what == "esc":
            width = k
            for j0 in range(0, ncodes, LANES):
                w.cover(first + j0 * width, (LANES * width + 31) // 32 + 2)
            ci += ncodes
            continue
        done, pos = 0, first
        while done < ncodes:
            before = len(w.reloads)
            w.cover(pos, LANES + FLOOK)
            lim = SEG_BITS * ((pos >> 5) + LANES)
            take = [c for c in codes[done:] if c[0] < lim]
            # next_one (:1189) looks for a code's closing 1 bit, k + 1 bits before its end, inside the window
            for j, (a, e) in enumerate(take):
                if e - 1 - k >= SEG_BITS * (w.W + FWIN):
                    out.redo, out.redo_code = True, ci + done + j
                    out.rounds.append(Round(p, pos, w.W, ci + done, len(take), len(w.reloads) > before, False))
                    return out
            last = done + len(take) == ncodes
            r = Round(p, pos, w.W, ci + done, len(take), len(w.reloads) > before, last)
            if last:
                a, e = take[-1]
                r.end_at_exit = e >= SEG_BITS * ((a >> 5) + 1)
                r.tot_eq_need = e >= lim
            out.rounds.append(r)
            done += len(take)
            pos = take[-1][1]
        ci += ncodes
    return out


# ---- helpers ----

def plan(dist, lo, hi):
    """Code lengths in [lo, hi] that add up to ``dist`` (None: impossible)."""
    n = max(1, -(-dist // hi))
    while n * lo <= dist:
        if dist <= n * hi:
            base, extra = divmod(dist - n * lo, n)
            return [lo + base + (1 if i < extra else 0) for i in range(n)]
        n += 1
    return None


def code(length, k, salt=0):
    """The residual whose Rice code of parameter k is ``length`` bits long."""
    q = length - 1 - k
    assert q >= 0
    low = (salt * 0x9E37 + 0x51) & ((1 << k) - 1)
    return B.unfold((q << k) | low)


def first_code(bs_code, pbits=4, number=0):
    """Bit at which the first code of a mono frame's fixed subframe (no wasted bits, order 0) starts: header,
    8 subframe header bits, 2 + 4 residual header bits, the parameter."""
    extra = {6: 1, 7: 2}.get(bs_code, 0)
    return 8 * (4 + len(B.utf8(number)) + extra + 1) + 8 + 6 + pbits


def next_boundary(at, lo, hi, after=1):
    """(lengths, boundary): the nearest word boundary at least ``after`` words ahead of ``at`` that codes of
    lo..hi bits reach exactly."""
    m = (at >> 5) + after
    while True:
        ls = plan(SEG_BITS * m - at, lo, hi)
        if ls:
            return ls, SEG_BITS * m
        m += 1


def mono_rice(bits, lengths, k, method=0, po=0, params=None, bs_code=7):
    """A mono stream of one frame: fixed order 0, Rice codes of the given lengths (residuals equal samples)."""
    res = [code(n, k if params is None else params[(i * (1 << po)) // len(lengths)], i) for i, n in enumerate(lengths)]
    r = B.Residual(method, po, tuple(params) if params else (k,))
    f = B.frame(len(res), [B.fixed(0, res, r)], bits, bs_code=bs_code)
    return B.stream(1, bits, [f])


def qmax(k, bits=16):
    """The longest unary run at parameter k whose residual still fits a 16-bit sample."""
    return ((1 << 16) - 1) >> k


def rng(seed):
    return random.Random(seed)


def smooth(n, seed, amp=90):
    r, v, out = rng(seed), 0, []
    for _ in range(n):
        v = max(-amp, min(amp, v + r.randrange(-7, 8)))
        out.append(v)
    return out


def auto_res(values, bs, order, po=0):
    """A Residual whose per-partition parameter keeps every unary run short (a rule, not a search)."""
    per, params, at, big = bs >> po, [], 0, 0
    for p in range(1 << po):
        n = per - (order if p == 0 else 0)
        mag = max([B.fold(v) for v in values[at:at + n]] or [0])
        params.append(max(0, mag.bit_length() - 3))
        big = max(big, params[-1])
        at += n
    return B.Residual(1 if big > 14 else 0, po, tuple(params))


def with_res(kind, order, samples, po=0, wasted=0, **lpc):
    """A fixed or LPC subframe with auto_res residual coding."""
    s = [v >> wasted for v in samples]
    sub = B.Sub(kind, s, order=order, **lpc)
    res = auto_res(B.residuals_of(sub, s), len(s), order, po)
    if kind == "fixed":
        return B.fixed(order, samples, res, wasted)
    return B.lpc(order, lpc["precision"], lpc["shift"], lpc["coefs"], samples, res, wasted)


def bs_code_for(bs):
    for c in (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 6, 7):
        try:
            B.blocksize_field(bs, c)
            return c
        except ValueError:
            pass
    raise ValueError(bs)


def word_aligned(pos):
    return pos % SEG_BITS == 0


# ---- a. a code on a segment boundary ----

def _a(k):
    def build(bits):
        lo, hi = k + 1, k + 1 + min(qmax(k), 40)
        at = first_code(7)
        l1, b1 = next_boundary(at, lo, hi)
        l2, b2 = next_boundary(b1, lo, hi)       # the code after b1 starts on it; the last of l2 ends on b2
        lengths = l1 + l2 + [lo + (i % (hi - lo + 1)) for i in range(7)]
        lengths += [lo] * (48 - len(lengths))
        return mono_rice(bits, lengths, k)

    def check(st, bits):
        m = st.marks[0][0]
        assert m.first[0] == first_code(7)
        starts = [a for a, _ in m.codes]
        ends = [e for _, e in m.codes]
        on = [i for i, a in enumerate(starts) if word_aligned(a)]
        assert len(on) >= 2 and on[0] > 0          # code on[0] starts at bit 32 * m ...
        assert word_aligned(ends[on[0] - 1])       # ... which is where the code before it ends
        assert any(not word_aligned(a) for a in starts)
        assert not wave_model(st).redo
    return build, check


for _k in (0, 1, 4, 14):
    _b, _c = _a(_k)
    CASES.append(Case(f"a_boundary_k{_k}", "a", _b, (16, 32), _c))


# ---- b. a code that covers whole lane segments ----

def _b_case(nseg):
    k = 3

    def build(bits):
        at = first_code(7)
        b1 = SEG_BITS * ((at >> 5) + 3)
        l1 = plan(b1 - 12 - at, k + 1, 24)           # the long code starts 12 bits before a boundary ...
        long = 12 + SEG_BITS * nseg + 9              # ... covers nseg whole words and ends 9 bits into the next
        lengths = l1 + [long] + [5, 9, 4, 17, 6]
        lengths += [k + 2] * (64 - len(lengths))
        return mono_rice(bits, lengths, k)

    def check(st, bits):
        m = st.marks[0][0]
        covers = [(e >> 5) - ((a + 31) >> 5) for a, e in m.codes]
        assert max(covers) == nseg and sorted(covers)[-2] <= 0
        a, e = m.codes[covers.index(nseg)]
        assert e - a > SEG_BITS and not word_aligned(a) and not word_aligned(e)
        assert not wave_model(st).redo               # inside the first window: the wave decoder keeps it
    return build, check


for _n in (2, 3, 63):
    _b, _c = _b_case(_n)
    CASES.append(Case(f"b_long_{_n}seg", "b", _b, (16, 32), _c))


# ---- c. a unary run around the look-ahead ----

C_K = 3  # 6144 << 3 = 49152: the residual 24576 fits 16 bits


def _c_case(run, late):
    """late: the run starts at the last bit of lane 63's segment in a round that begins FWIN - LANES - FLOOK
    words into the window, where the look-ahead is exactly FLOOK words; else in the frame's first round."""
    def build(bits):
        at = first_code(7)
        if late:
            l1, b1 = next_boundary(at, C_K + 1, 28)
            W = (8 * 8) >> 5                          # the window is loaded at the frame header's end
            words = W + (FWIN - LANES - FLOOK) + LANES - 1 - (b1 >> 5)
            lengths = l1 + [32] * words + [31]        # 32-bit codes up to lane 63's word, 31 bits of it
        else:
            lengths = [7, 5]
        lengths += [run + 1 + C_K] + [6, 4, 11, 5]
        lengths += [C_K + 2] * (512 - len(lengths))
        return mono_rice(bits, lengths, C_K)

    def check(st, bits):
        m = st.marks[0][0]
        runs = [e - a - 1 - C_K for a, e in m.codes]
        i = runs.index(run)
        assert max(runs) == run and sorted(runs)[-2] < 32
        mod = wave_model(st)
        a, e = m.codes[i]
        if late:
            r = mod.rounds[-1] if mod.redo else next(r for r in mod.rounds if r.first <= i < r.first + r.count)
            assert (r.pos >> 5) == r.W + FWIN - LANES - FLOOK and not r.reloaded
            assert a == SEG_BITS * ((r.pos >> 5) + LANES) - 1       # last bit of lane 63's segment
            inside = a + run < SEG_BITS * (r.W + FWIN)              # the closing 1 bit is in the window
            assert inside == (run <= FLOOK * SEG_BITS)
            assert mod.redo == (not inside) and (not mod.redo or mod.redo_code == i)
        else:
            assert a - m.first[0] < FLOOK * SEG_BITS and not mod.redo
    return build, check


for _run, _late in ((2047, True), (2048, True), (2049, True), (3 * 2048, True), (2049, False), (3 * 2048, False)):
    _b, _c = _c_case(_run, _late)
    CASES.append(Case(f"c_run_{_run}_{'late' if _late else 'first_round'}", "c", _b, (16, 32), _c))


# ---- d. partition end and lane exit ----

def _d_case(kind):
    k = 2

    def build(bits):
        at = first_code(7)
        full = SEG_BITS * ((at >> 5) + LANES)         # the end of lane 63's segment in the first round
        if kind == "one_round":                        # tot == need, r == cnt, endp = X
            l0 = plan(full - at, k + 1, 20)
        elif kind == "second_round_one_code":
            l0 = plan(full - at, k + 1, 20) + [9]
        elif kind == "exit_mid_round":                 # ends on a word boundary, lanes after it parse on
            l0 = plan(SEG_BITS * ((at >> 5) + 10) - at, k + 1, 20)
        elif kind == "exit_long_last":                 # the last code starts in a word and ends past it
            l0 = plan(SEG_BITS * ((at >> 5) + 10) - 7 - at, k + 1, 20) + [7 + 13]
        else:                                          # "mask": ends inside a word, the lane parses on in it
            l0 = plan(SEG_BITS * ((at >> 5) + 10) - at, k + 1, 20) + [11]
        n = len(l0)
        lengths = l0 + [k + 1 + (i % 5) for i in range(n)]
        return mono_rice(bits, lengths, k, po=1, params=(k, k))

    def check(st, bits):
        m = st.marks[0][0]
        n = len(m.codes) // 2
        mod = wave_model(st)
        assert not mod.redo
        r0 = [r for r in mod.rounds if r.part == 0]
        a, e = m.codes[n - 1]
        assert e == m.parts[0][1]
        if kind == "one_round":
            assert len(r0) == 1 and r0[0].tot_eq_need and r0[0].end_at_exit and word_aligned(e)
            assert e == SEG_BITS * ((m.first[0] >> 5) + LANES)
        elif kind == "second_round_one_code":
            assert [r.count for r in r0] == [n - 1, 1] and word_aligned(a)
        elif kind == "exit_mid_round":
            assert len(r0) == 1 and r0[0].end_at_exit and not r0[0].tot_eq_need and word_aligned(e)
        elif kind == "exit_long_last":
            assert len(r0) == 1 and r0[0].end_at_exit and not r0[0].tot_eq_need and not word_aligned(e)
            assert (e >> 5) == (a >> 5) + 1
        else:
            assert len(r0) == 1 and not r0[0].end_at_exit and (a >> 5) == ((e - 1) >> 5) == (e >> 5)
    return build, check


for _kind in ("one_round", "second_round_one_code", "exit_mid_round", "exit_long_last", "mask"):
    _b, _c = _d_case(_kind)
    CASES.append(Case(f"d_{_kind}", "d", _b, (16, 32), _c))


# ---- e. partition sizes ----

def _e_case(bs, po, order):
    def build(bits):
        x = smooth(bs, bs + po + order, 300)
        f = B.frame(bs, [with_res("fixed", order, x, po)], bits, bs_code=bs_code_for(bs))
        return B.stream(1, bits, [f])

    def check(st, bits):
        m = st.marks[0][0]
        per = bs >> po
        counts, ci = [], 0
        for ps, pe in m.parts:
            n = sum(1 for a, _ in m.codes[ci:] if a < pe)
            counts.append(n)
            ci += n
        assert counts == [per - order] + [per] * ((1 << po) - 1) and sum(counts) == bs - order
        if per == order:
            assert m.parts[0][1] == m.first[0]        # the first partition: a parameter and no code
    return build, check


for _bs, _po, _o in ((16, 0, 0), (64, 0, 1), (64, 0, 0), (65, 0, 0), (4096, 0, 0), (256, 8, 1), (4096, 8, 16 - 12),
                     (4096, 8, 0)):
    _b, _c = _e_case(_bs, _po, _o)
    CASES.append(Case(f"e_bs{_bs}_po{_po}_o{_o}", "e", _b, (16, 32), _c))


def _e16_build(bits):
    """Block size 4096, partition order 8, LPC order 16 = 4096 >> 8: the first partition holds no residual."""
    x = smooth(4096, 77, 200)
    coefs = (3, -2, 1, 0, 1, -1, 0, 2, -1, 0, 1, 0, -1, 1, 0, -1)
    f = B.frame(4096, [with_res("lpc", 16, x, 8, precision=4, shift=2, coefs=coefs)], bits, bs_code=12)
    return B.stream(1, bits, [f])


def _e16_check(st, bits):
    m = st.marks[0][0]
    assert len(m.parts) == 256 and m.parts[0][1] == m.first[0] and len(m.codes) == 4096 - 16


CASES.append(Case("e_bs4096_po8_lpc16", "e", _e16_build, (16, 32), _e16_check))


# ---- f. the extreme parameters ----

@case("f_k0_throughout", "f")
def _f_k0(bits):
    r = rng(5)
    x = [r.choice((0, 0, 0, -1, 1, -2, 2, 3, -9)) for _ in range(192)]
    return B.stream(1, bits, [B.frame(192, [B.fixed(0, x, B.Residual(0, 2, (0, 0, 0, 0)))], bits, bs_code=1)])


def _f5(k):
    def build(bits):
        r = rng(k)
        lim = min(1 << 31, 6 << k)
        x = [r.randrange(-lim, lim) for _ in range(64)]
        x[3], x[4] = lim - 1, -lim + 1
        return B.stream(1, bits, [B.frame(64, [B.fixed(0, x, B.Residual(1, 1, (k, k)))], bits, bs_code=6)])
    return build


for _k in (15, 16, 30):
    CASES.append(Case(f"f_rice2_k{_k}", "f", _f5(_k), (32,)))


# ---- g. escape partitions ----

def _g_width(width, wasted=0):
    def build(bits):
        r = rng(width)
        lim = 1 << (width - 1) if width else 0
        x = [(r.randrange(-lim, lim) if lim else 0) << wasted for _ in range(80)]
        if lim:
            x[0], x[1] = (lim - 1) << wasted, -lim << wasted
        res = B.Residual(0, 0, (("esc", width),))
        return B.stream(1, bits, [B.frame(80, [B.fixed(0, x, res, wasted)], bits, bs_code=6)])
    return build


for _w in (0, 1, 15):
    CASES.append(Case(f"g_escape_w{_w}", "g", _g_width(_w)))
CASES.append(Case("g_escape_w31", "g", _g_width(31), (32,)))
CASES.append(Case("g_escape_w31_wasted1", "g", _g_width(31, 1), (32,)))   # 32 - wasted
CASES.append(Case("g_escape_w14_wasted2", "g", _g_width(14, 2), (16,)))   # 16 - wasted


def _g_between(aligned):
    k = 2

    def build(bits):
        at = first_code(7)
        target = SEG_BITS * ((at >> 5) + 6) - 9 + (0 if aligned else 13)   # 4-bit escape code + 5-bit width
        l0 = plan(target - at, k + 1, 20)
        n = len(l0)
        r = rng(n)
        x = [code(v, k, i) for i, v in enumerate(l0)] + [r.randrange(-256, 256) for _ in range(n)]
        x += [code(k + 1 + i % 6, k, i) for i in range(2 * n)]
        res = B.Residual(0, 2, (k, ("esc", 9), k, k))
        return B.stream(1, bits, [B.frame(4 * n, [B.fixed(0, x, res)], bits, bs_code=7)])

    def check(st, bits):
        m = st.marks[0][0]
        assert m.first[1] - m.parts[1][0] == 9 and word_aligned(m.first[1]) == aligned
        assert not wave_model(st).redo
    return build, check


for _al in (True, False):
    _b, _c = _g_between(_al)
    CASES.append(Case(f"g_escape_between_{'aligned' if _al else 'unaligned'}", "g", _b, (16, 32), _c))


# ---- h. the widest residuals ----

def _h32(value, allow):
    def build(bits):
        right = [0] * 16
        side = [5, -3, value] + [0, 1, -1] * 4 + [2]
        if value == 1 << 31:
            right[2] = -1
        left = [s + r for s, r in zip(side, right)]
        subs = [B.verbatim(left), B.fixed(0, side, B.Residual(1, 0, (30,)))]
        f = B.frame(16, subs, 32, bs_code=6, assignment="left_side", allow_wide=allow)
        return B.stream(2, 32, [f])
    return build


def _h16(value, allow):
    """A 17-bit side channel under an LPC predictor of order 2, coefficients -2^14, shift 0: after two side
    samples of +-65535 the prediction is -+(2^31 - 32768)."""
    def build(bits):
        sg = 1 if value > 0 else -1
        third = value - sg * ((1 << 31) - 32768)
        side = [sg * 65535, sg * 65535, third] + [0] * 13
        edge = 32767 if sg > 0 else -32768          # side +-65535 is edge - (the other edge)
        left = [edge, edge, max(-32768, min(32767, third))] + [0] * 13
        sub = B.lpc(2, 15, 0, (-(1 << 14), -(1 << 14)), side, B.Residual(1, 0, (28,)))
        f = B.frame(16, [B.verbatim(left), sub], 16, bs_code=6, assignment="left_side", allow_wide=allow)
        st = B.stream(2, 16, [f])
        assert value in B.residuals_of(sub, side)
        return st
    return build


CASES.append(Case("h_res_max_32", "h", _h32((1 << 31) - 1, False), (32,)))
CASES.append(Case("h_res_min_32", "h", _h32(-(1 << 31), True), (32,), wide="min"))
CASES.append(Case("h_res_over_32", "h", _h32(1 << 31, True), (32,), wide="ok"))
CASES.append(Case("h_res_max_16", "h", _h16((1 << 31) - 1, False), (16,)))
CASES.append(Case("h_res_min_16", "h", _h16(-(1 << 31), True), (16,), wide="min"))
CASES.append(Case("h_res_over_16", "h", _h16(1 << 31, True), (16,), wide="ok"))


# ---- i. a window reload inside a partition ----

def _i_build(bits):
    k, r = 3, rng(12)
    lengths = [r.choice((4, 5, 5, 6, 7, 9, 13, 33, 40)) for _ in range(4096)]
    return mono_rice(bits, lengths, k, bs_code=12)


def _i_check(st, bits):
    m = st.marks[0][0]
    assert m.parts[0][1] - m.parts[0][0] > FWIN * SEG_BITS
    mod = wave_model(st)
    assert not mod.redo
    re = [r for r in mod.rounds if r.reloaded and r.first > 0]
    assert re and all(r.part == 0 for r in re)
    old_end = SEG_BITS * (mod.rounds[0].W + FWIN)
    assert any(a < old_end < e for a, e in m.codes)            # a code straddles the old window's end
    assert any(not word_aligned(r.pos) for r in re)            # ... and a reload starts inside a word


CASES.append(Case("i_reload_in_partition", "i", _i_build, (16, 32), _i_check))


# ---- j. fixed predictors ----

def _j_short(order):
    def build(bits):
        x = smooth(16 + order, order, 1 << (bits - 2))
        f0 = B.frame(16, [with_res("fixed", order, x[:16])], bits, bs_code=6, number=0)
        f1 = B.frame(order, [B.fixed(order, x[16:], B.Residual(0, 0, (0,)))], bits, bs_code=6, number=1)
        return B.stream(1, bits, [f0, f1])

    def check(st, bits):
        m = st.marks[1][0]
        assert not m.codes and m.parts[0][1] == m.first[0]
    return build, check


for _o in (1, 2, 3, 4):   # (a block of 0 samples does not exist: order 0 has no such case)
    _b, _c = _j_short(_o)
    CASES.append(Case(f"j_fixed{_o}_blocksize_is_order", "j", _b, (16, 32), _c))


def full_scale_alternating(bits, order, n=40):
    """+-A alternating with the largest A <= 2^(bits-1) whose order-``order`` residuals keep the 32-bit rule."""
    def resid(a):
        x = [(-a if i & 1 else a - 1) for i in range(n)]
        return x, B.residuals_of(B.Sub("fixed", x, order=order), x)
    lo, hi = 1, 1 << (bits - 1)
    if all(abs(v) < 1 << 31 for v in resid(hi)[1]):
        return resid(hi)[0], hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if all(abs(v) < 1 << 31 for v in resid(mid)[1]):
            lo = mid
        else:
            hi = mid
    return resid(lo)[0], lo


def _j_full(order):
    def build(bits):
        x, a = full_scale_alternating(bits, order)
        return B.stream(1, bits, [B.frame(40, [with_res("fixed", order, x)], bits, bs_code=6)])

    def check(st, bits):
        x, a = full_scale_alternating(bits, order)
        res = B.residuals_of(B.Sub("fixed", x, order=order), x)
        assert max(abs(v) for v in res) < 1 << 31
        assert bits == 32 or a == 1 << (bits - 1)
        if a < 1 << (bits - 1):   # scaled down: one step larger breaks the rule
            big = [(-(a + 1) if i & 1 else a) for i in range(40)]
            assert max(abs(v) for v in B.residuals_of(B.Sub("fixed", big, order=order), big)) >= 1 << 31
    return build, check


for _o in range(5):
    _b, _c = _j_full(_o)
    CASES.append(Case(f"j_fixed{_o}_full_scale", "j", _b, (16, 32), _c))


# ---- k. LPC ----

def _k_case(order, precision, shift, coefs, amp):
    def build(bits):
        x = smooth(96, order * 31 + precision, amp)
        sub = with_res("lpc", order, x, 1, precision=precision, shift=shift, coefs=coefs)
        return B.stream(1, bits, [B.frame(96, [sub], bits, bs_code=6)])
    return build


P15 = (1 << 14) - 1
CASES.append(Case("k_lpc_o1_p1_s0", "k", _k_case(1, 1, 0, (-1,), 3000)))
CASES.append(Case("k_lpc_o2_p1_s15", "k", _k_case(2, 1, 15, (-1, 0), 3000)))
CASES.append(Case("k_lpc_o2_p15_s15", "k", _k_case(2, 15, 15, (P15, -(1 << 14)), 3000)))
CASES.append(Case("k_lpc_o31_p15_s0", "k", _k_case(31, 15, 0, tuple((P15, -P15, -(1 << 14))[j % 3] for j in range(31)),
                                                   900)))
CASES.append(Case("k_lpc_o32_p15_s15", "k", _k_case(32, 15, 15, tuple((P15, -(1 << 14))[j & 1] for j in range(32)),
                                                    3000)))
CASES.append(Case("k_lpc_o32_p2_s0", "k", _k_case(32, 2, 0, tuple((1, -2, -1, 0)[j % 4] for j in range(32)), 200)))


def _k_acc_parts():
    left = [-(1 << 31)] * 24
    right = [(1 << 31) - 1 - (i % 3) for i in range(24)]
    side = [a - b for a, b in zip(left, right)]
    return left, side, (P15, P15, P15)


def _k_acc_build(bits):
    """A 33-bit side channel near -(2^32 - 1) under three coefficients of 2^14 - 1, shift 15: the sum is about
    -1.5 * 2^47, negative with a remainder under the shift."""
    left, side, coefs = _k_acc_parts()
    sub = with_res("lpc", 3, side, 0, precision=15, shift=15, coefs=coefs)
    return B.stream(2, 32, [B.frame(24, [B.constant(left), sub], 32, bs_code=6, assignment="left_side")])


def _k_acc_check(st, bits):
    left, side, coefs = _k_acc_parts()
    accs = [sum(c * side[i - 1 - j] for j, c in enumerate(coefs)) for i in range(3, 24)]
    assert all(a < -(1 << 47) for a in accs) and any(a % (1 << 15) for a in accs)
    assert any((a >> 15) != -((-a) >> 15) for a in accs)   # floor differs from truncation


CASES.append(Case("k_lpc_sum_beyond_2_47", "k", _k_acc_build, (32,), _k_acc_check))


# ---- l. wasted bits ----

def _l_case(wfn, name):
    def build(bits):
        w = wfn(bits)
        b = bits - w
        lim = 1 << (b - 1)
        r = rng(w)
        base = [max(-lim, min(lim - 1, v)) for v in smooth(48, w, min(lim, 200))]
        if b > 1:
            base[5] |= 1                        # the lowest kept bit is set somewhere: exactly w wasted bits
        else:
            base = [r.choice((-1, 0)) for _ in range(48)]
        x = [v << w for v in base]
        c = [(-lim) << w] * 48
        subs = [B.constant(c, w), B.verbatim(x, w), with_res("fixed", min(2, 0 if b < 3 else 2), x, 0, w),
                with_res("lpc", 2, x, 0, w, precision=3, shift=1, coefs=(2, -1))]
        return B.stream(4, bits, [B.frame(48, subs, bits, bs_code=6)])
    return build


for _name, _fn in (("1", lambda b: 1), ("bps_minus_2", lambda b: b - 2), ("bps_minus_1", lambda b: b - 1)):
    CASES.append(Case(f"l_wasted_{_name}", "l", _l_case(_fn, _name)))


def _l_side(wfn):
    def build(bits):
        w = wfn(bits)
        unit = 1 << w
        top = (1 << bits) - 1
        pick = [v for v in (-2 * unit, -unit, 0, unit) if abs(v) <= top] if w < bits else [0]
        r = rng(w + bits)
        side = [r.choice(pick) for _ in range(32)]
        lo = -(1 << (bits - 1))
        left = [lo + s if s >= 0 else lo for s in side]   # right = left - side stays in range
        f = B.frame(32, [B.verbatim(left), B.verbatim(side, w)], bits, bs_code=6, assignment="left_side")
        return B.stream(2, bits, [f])
    return build


for _name, _fn in (("1", lambda b: 1), ("bps_minus_1", lambda b: b - 1), ("bps", lambda b: b)):
    CASES.append(Case(f"l_wasted_side_{_name}", "l", _l_side(_fn)))


# ---- m. channel assignments ----

def _m_case(assignment, bits):
    def build(_):
        lim = 1 << (bits - 1)
        r = rng(bits)
        left = [lim - 1, -lim, lim - 1, -lim, 0, 1, -1, 7] + [r.randrange(-lim, lim) for _ in range(24)]
        right = [-lim, lim - 1, lim - 1, -lim, 1, 0, -2, 4] + [r.randrange(-lim, lim) for _ in range(24)]
        side = [a - b for a, b in zip(left, right)]
        assert side[0] == (1 << bits) - 1 and side[1] == -((1 << bits) - 1)
        assert any(s & 1 for s in side) and any(not s & 1 for s in side)
        if assignment == "left_side":
            subs = [B.verbatim(left), B.verbatim(side)]
        elif assignment == "right_side":
            subs = [B.verbatim(side), B.verbatim(right)]
        elif assignment == "mid_side":
            subs = [B.verbatim([(a + b) >> 1 for a, b in zip(left, right)]), B.verbatim(side)]
        else:
            subs = [B.verbatim(left), B.verbatim(right)]
        f = B.frame(32, subs, bits, bs_code=6, assignment=assignment)
        st = B.stream(2, bits, [f])
        assert st.samples == [v for pair in zip(left, right) for v in pair]
        return st
    return build


for _bits in (8, 16, 24, 32):
    for _as in (None, "left_side", "right_side", "mid_side"):
        CASES.append(Case(f"m_{_as or 'independent'}_{_bits}", "m", _m_case(_as, _bits), (_bits,)))


@case("m_eight_kinds", "m")
def _m8(bits):
    xs = [smooth(64, 40 + c, 100) for c in range(8)]
    xs[0] = [-77] * 64
    subs = [B.constant(xs[0]), B.verbatim(xs[1]), with_res("fixed", 0, xs[2]), with_res("fixed", 1, xs[3], 2),
            with_res("fixed", 3, xs[4]), with_res("fixed", 4, xs[5], 1),
            with_res("lpc", 1, xs[6], 0, precision=5, shift=3, coefs=(7,)),
            with_res("lpc", 9, xs[7], 1, precision=6, shift=4, coefs=(20, -9, 3, 1, 0, -1, 2, 0, 1))]
    return B.stream(8, bits, [B.frame(64, subs, bits, bs_code=6)])


# ---- n. header codes ----

N_BLOCKS = [(1, 192), (2, 576), (3, 1152), (4, 2304), (5, 4608), (6, 16), (6, 17), (6, 255), (6, 256), (7, 257),
            (7, 65535)] + [(c, 256 << (c - 8)) for c in range(8, 16)]


def _n_bs(code, bs, rate_code, size0):
    def build(bits):
        x = smooth(min(bs, 300), bs, 100)
        x = (x * (bs // len(x) + 1))[:bs]
        sub = B.verbatim(x) if bs <= 4608 else B.constant([-(1 << (bits - 1))] * bs)
        f = B.frame(bs, [sub], bits, bs_code=code, rate_code=rate_code, rate_extra={12: 44, 13: 44100, 14: 4410}.get(
            rate_code), size_code=0 if size0 else None)
        return B.stream(1, bits, [f])
    return build


for _i, (_code, _bs) in enumerate(N_BLOCKS):
    _rc = (12, 13, 14, 0, 1, 4, 8, 11, 9)[_i % 9]
    CASES.append(Case(f"n_bs_code{_code}_{_bs}_rate{_rc}", "n", _n_bs(_code, _bs, _rc, _i % 2 == 0)))

for _bits in (8, 12, 16, 20, 24, 32):
    for _zero in (False, True):
        CASES.append(Case(f"n_size_{_bits}_{'from_streaminfo' if _zero else 'explicit'}", "n",
                          _n_bs(6, 20, 12 + _bits % 3, _zero), (_bits,)))


@case("n_big_block_rice_65535", "n", widths=(16,))
def _n_big(bits):
    """256 KiB of 16-bit samples in one block: more than the wave decoder's LDS, so the lane decoder's int32
    instance takes the frame."""
    r = rng(65535)
    x = [r.randrange(-40, 40) if i % 997 else r.randrange(-32768, 32768) for i in range(65535)]
    assert 4 * (FWIN + 2) + 4 * 65535 > WAVE_LDS
    f = B.frame(65535, [B.fixed(0, x, B.Residual(0, 0, (4,)))], 16, bs_code=7)
    return B.stream(1, 16, [f])


# ---- o. variable block size: sample numbers of 1 to 5 bytes ----

def _var_stream(bits, sizes, sub_of):
    frames, at = [], 0
    for i, bs in enumerate(sizes):
        bs, code = bs if isinstance(bs, tuple) else (bs, bs_code_for(bs))
        frames.append(B.frame(bs, [sub_of(i, bs)], bits, bs_code=code, number=at, variable=True))
        at += bs
    return B.stream(1, bits, frames, variable=True)


def _o_small(bits):
    return _var_stream(8, [130, 2000, 100], lambda i, bs: B.constant([(-1) ** i * (i + 3)] * bs))


def _o_check(want):
    def check(st, bits):
        nums = []
        total = 0
        for (pos, _), bs in zip(st.frames, st.blocksizes):
            nums.append(len(B.utf8(total)))
            total += bs
        assert set(nums) == want
    return check


def _o_big(bits):
    return _var_stream(8, [65535] * 34, lambda i, bs: B.constant([i - 17] * bs))


CASES.append(Case("o_sample_numbers_1_to_3_bytes", "o", _o_small, (8,), _o_check({1, 2, 3})))
CASES.append(Case("o_sample_numbers_to_5_bytes", "o", _o_big, (8,), _o_check({1, 3, 4, 5})))


# ---- p. frame byte lengths ----

def _p_sizes(lo, hi):
    return list(range(lo, hi + 1))


def _p_build(lo, hi, fill):
    def build(bits):
        r = rng(lo)
        sizes = _p_sizes(lo, hi)
        st = _var_stream(8, sizes, lambda i, bs: B.verbatim([r.randrange(-128, 128) for _ in range(bs)]))
        if fill:   # the frame length jumps where the coded number or the block-size field grows: fill the gaps
            lens = {n for _, n in st.frames}
            assert len(B.utf8(st.total)) == len(B.utf8(st.total + 20 * hi)) == 4
            for n in range(min(lens), max(lens) + 1):
                if n not in lens:   # a frame after all these (a 4-byte sample number) with a 16-bit block size field
                    sizes.append((n - (4 + 4 + 2 + 1 + 1 + 2), 7))
                    assert lo <= sizes[-1][0] <= hi
            st = _var_stream(8, sizes, lambda i, bs: B.verbatim([r.randrange(-128, 128) for _ in range(bs)]))
        return st
    return build


def _p_check(st, bits):
    lens = sorted({n for _, n in st.frames})
    assert lens == list(range(lens[0], lens[-1] + 1)) and len(lens) > 512
    assert {0, 1, 63} <= {n % 64 for n in lens}


CASES.append(Case("p_frame_lengths_16_600", "p", _p_build(16, 600, True), (8,), _p_check, direct_only=True))
for _lo, _hi in ((16, 64), (64, 256), (256, 600)):
    CASES.append(Case(f"p_frame_lengths_{_lo}_{_hi}", "p", _p_build(_lo, _hi, False), (8,)))


# ---- frames that must be refused ----

@dataclass
class Refused:
    name: str
    build: object   # bits -> B.Stream (three frames; the second is the bad one)
    widths: tuple = (16, 32)


def _good(bits, number, channels=1):
    subs = [with_res("fixed", 1, smooth(16, number + c, 50)) for c in range(channels)]
    return B.frame(16, subs, bits, bs_code=6, number=number)


def _refused(name, bad_sub, channels=1, first=None):
    def build(bits):
        subs = ([first(bits)] if first else []) + [bad_sub(bits)]
        x = [0] * 16
        for s in subs:
            if s.samples is None or len(s.samples) != 16:
                s.samples = x
        bad = B.frame(16, subs, bits, bs_code=6, number=1)
        return B.stream(channels, bits, [_good(bits, 0, channels), bad, _good(bits, 2, channels)])
    REFUSED.append(Refused(name, build))


def _hdr(kind, wasted_flag=0, pad=0):
    return [(pad, 1), (kind, 6), (wasted_flag, 1)]


FILL = [(0x2AAAAAAA, 30)] * 12   # bits for a parser to run on


def _const_tail(bits):
    return [(5, bits)]


for _t in (2, 7, 13, 31):
    _refused(f"reserved_type_{_t}", lambda bits, t=_t: B.raw_subframe(_hdr(t) + FILL))
_refused("subframe_padding_bit", lambda bits: B.raw_subframe(_hdr(0, pad=1) + _const_tail(bits)))
for _m in (2, 3):
    _refused(f"residual_method_{_m}", lambda bits, m=_m: B.fixed(0, [0] * 16, raw_residual=[(m, 2), (0, 4), (1, 4)] +
                                                                [(1, 2)] * 16))
_refused("lpc_precision_1111", lambda bits: B.raw_subframe(
    _hdr(32) + [(3, bits), (15, 4), (1, 5), (1, 15), (0, 2), (0, 4), (0, 4)] + [(1, 1)] * 15))
_refused("lpc_negative_shift", lambda bits: B.raw_subframe(
    _hdr(32) + [(3, bits), (3, 4), (0b11111, 5), (1, 4), (0, 2), (0, 4), (0, 4)] + [(1, 1)] * 15))
_refused("wasted_equals_bps", lambda bits: B.raw_subframe(_hdr(1, 1) + [(1, bits)] + FILL))
_refused("wasted_above_bps", lambda bits: B.raw_subframe(_hdr(1, 1) + [(0, bits), (1, 3)] + FILL))
_refused("order_above_blocksize", lambda bits: B.raw_subframe(_hdr(31 + 20) + [(1, bits)] * 20 + FILL))
_refused("blocksize_not_multiple_of_partitions", lambda bits: B.fixed(0, [0] * 16, raw_residual=[(0, 2), (5, 4)] + [
    (0b00001, 5)] * 32))
_refused("partition_shorter_than_order", lambda bits: B.raw_subframe(
    _hdr(8 + 4) + [(1, bits)] * 4 + [(0, 2), (3, 4)] + [(0b00001, 5)] * 16))
_refused("escape_runs_past_the_frame", lambda bits: B.fixed(0, [0] * 16, raw_residual=[(0, 2), (0, 4), (15, 4),
                                                                                      (31, 5), (0x155, 31)]))
_refused("last_code_ends_in_the_crc16", lambda bits: B.fixed(0, [0] * 16, raw_residual=[(0, 2), (0, 4), (0, 4)] +
                                                             [(1, 1)] * 15 + [(0, 3)]))


def _run_to_end(bits):
    """Stereo: a verbatim subframe whose first sample is chosen so that the frame's CRC-16 is 0x0000, then a
    fixed subframe whose last Rice code is all zeros: the unary run passes the padding and the CRC-16 and ends
    only at the next frame's sync code."""
    tail = B.fixed(0, [0] * 16, raw_residual=[(0, 2), (0, 4), (0, 4)] + [(1, 1)] * 15 + [(0, 5)])
    good = [_good(bits, 0, 2), _good(bits, 2, 2)]

    def attempt(v):
        x = [v - 65536 if bits == 16 and v >= 32768 else v] + [0] * 15
        tail.samples = [0] * 16
        return B.frame(16, [B.verbatim(x), tail], bits, bs_code=6, number=1)
    f0 = attempt(0)
    at = f0.header_len + 1 + bits // 8 - 2                  # the low 16 bits of the first sample
    assert f0.marks[0].first[0] == 8 * (f0.header_len + 1)
    # the CRC-16 is affine in those bits: crc(v) = crc(0) ^ lo[v & 255] ^ hi[v >> 8]
    body = bytearray(f0.data[:-2])
    c0 = B.crc16(bytes(body))

    def effect(v):
        body[at:at + 2] = v.to_bytes(2, "big")
        return B.crc16(bytes(body)) ^ c0
    hi = {effect(b << 8): b for b in range(256)}
    for a in range(256):
        b = hi.get(effect(a) ^ c0)
        if b is not None:
            f = attempt((b << 8) | a)
            assert f.data[-2:] == b"\0\0"
            return B.stream(2, bits, [good[0], f, good[1]])
    raise AssertionError("no sample gives a CRC-16 of zero")


REFUSED.append(Refused("unary_run_reaches_the_frame_end", _run_to_end))


@functools.lru_cache(maxsize=None)
def built_refused(name: str, bits: int) -> B.Stream:
    return REFUSED_BY_NAME[name].build(bits)


BY_NAME = {c.name: c for c in CASES}
REFUSED_BY_NAME = {c.name: c for c in REFUSED}
assert len(BY_NAME) == len(CASES) and len(REFUSED_BY_NAME) == len(REFUSED)
FAMILIES = "abcdefghijklmnop"
