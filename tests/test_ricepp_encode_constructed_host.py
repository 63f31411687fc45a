"""CPU tests of the constructed ricepp encode cases (tests/ricepp_build.py, the ``enc_*`` families; no GPU needed):
every case is what an encoder writes for its input (the oracle and the compiled reference give ``case.stream``
byte for byte, and the oracle decodes it back), every family reaches what it aims at (counted from ``layout`` and
the restated split rule and kernel geometry), and a small encoder written here (encode.h:43-157 through the
``build`` writer) reproduces every case while each of its deliberately wrong variants differs on a case of the
family aimed at it.  The same families run on the GPU in tests/test_gpu_ricepp_encode_constructed.py."""

from collections import Counter

import numpy as np
import pytest

import ricepp_build as B
from oracle import oracle as O
from oracle import reference as R

# streams per family: a change of a family shows here
FAMILY_SIZES = {"enc_split_start": 2898, "enc_split_walk": 51, "enc_emit_paths": 115, "enc_flush_edges": 92,
                "enc_shapes": 990, "enc_segments": 620, "enc_values": 72}
LONG = ("enc_flush_edges",)  # the only family whose streams are longer than about 6000 samples


def ocfg(cfg: B.Cfg):
    return O.cfg(cfg.bs, cfg.cs, cfg.big, cfg.ulsb)


def inp(c: B.Case) -> np.ndarray:
    return c.want if c.inp is None else c.inp


@pytest.mark.parametrize("family", list(B.ENC_FAMILIES))
def test_every_case_is_canonical(family):
    """The oracle's and the compiled reference's encoder write exactly the case's bytes; the oracle decodes them
    to the samples the fields stand for (the input, but for dropped dirt)."""
    cases = B.ENC_FAMILIES[family]()
    assert len(cases) == FAMILY_SIZES[family]
    assert len({c.what for c in cases}) == len(cases)
    ref = R.available()
    for c in cases:
        assert len(c.stream) * 8 < 128 * 1024, c.what
        assert family in LONG or c.n_samples <= 6000, c.what
        assert c.n_samples % c.cfg.cs == 0 and c.status == B.OK and c.stream == B.build(c.cfg, c.fields), c.what
        assert len(c.stream) <= B.worst_case_bytes(c.cfg, c.n_samples), c.what
        if c.n_samples:
            assert O.encode(ocfg(c.cfg), inp(c)) == c.stream, c.what
            if ref:
                assert R.encode(ocfg(c.cfg), inp(c)) == c.stream, c.what
        assert np.array_equal(O.decode(ocfg(c.cfg), c.stream, c.n_samples), c.want), c.what
    print(f"{family}: {len(cases)} streams, {sum(len(c.stream) for c in cases)} bytes, "
          f"{sum(c.n_samples for c in cases)} samples, reference {'checked' if ref else 'not available'}")
    if not ref:
        pytest.skip("neither oracle/_ref/libdwarfs_ref.so nor the reference tree to build it from")


def walks(c: B.Case):
    """(sub-block, deltas, restated walk) of every sub-block with a non-zero delta."""
    for s, d in zip(c.fields.subs, B.deltas_of(c.cfg, c)):
        if d.any():
            yield s, d, B.split_rule(d)


def test_what_the_split_rule_cannot_do():
    """On every sub-block of every family: no step down, at most one step behind the first pair, bits < 16 n
    whenever fs < 14, and a hill climb that ends at the lowest cost of any fs (ricepp_build's note gives the
    reasons): walks down to 0, walks of several steps, costs of 16 n - 1, 16 n and 16 n + 1 at fs < 14 and hill
    climbs that end above the global minimum do not exist, so no family holds them."""
    seen = 0
    for fam in B.ENC_FAMILIES.values():
        for c in fam():
            for s, d, w in walks(c):
                seen += 1
                assert w.steps <= 1 and (w.dir == 1 or w.steps == 0) and w.fs <= w.start + 2, c.what
                assert w.fs >= 14 or w.bits < 16 * len(d), c.what
                assert w.bits == w.best or w.fs >= 14, c.what  # (the walk ends at 14: raw either way)
                assert isinstance(s, B.Raw) == (w.fs >= 14) and (w.fs >= 14 or s.fs == w.fs), c.what
    assert seen > 10000


def test_families_reach_what_they_aim_at():
    # enc_split_start: every (bs, n, m, variant) triple in the last chunk, both cs per bs, the tie reveals start
    reached, cs_seen = Counter(), set()
    for c in B.enc_split_start():
        ds = B.deltas_of(c.cfg, c)[c.cfg.cs:]
        named = dict(kv.split("=") for kv in c.what.split()[1:5])
        for comp, (s, d) in enumerate(zip(c.fields.subs[c.cfg.cs:], ds)):
            n, total = len(d), int(d.sum())
            # (the second component runs m + 5 and the next variant)
            m, var = (int(named["m"]) + 5 * comp) % 14, (int(named["var"]) + 1 + comp) % 3 - 1
            assert n == int(named["n"]) and total == n * (1 << m) + var, (c.what, total)
            assert int(d.min()) >= (1 << m) - 1 and int(d.max()) <= (1 << m) + 1, c.what
            reached[c.cfg.bs, n, m, var] += 1
            if var == 0:  # all deltas 2^m: equal costs at m - 1 and m, the walk stops at start + 1
                assert isinstance(s, B.Rice) and s.fs == max(m, 1), c.what
        cs_seen.add((c.cfg.bs, c.cfg.cs))
    for bs in B.START_BS_ALL + B.START_BS_SOME:
        assert (bs, 1) in cs_seen and (bs, 2) in cs_seen
        for n in B.start_ns(bs):
            missing = [(m, v) for m in range(14) for v in (-1, 0, 1) if not reached[bs, n, m, v]]
            assert not missing, (bs, n, missing)
    print(f"enc_split_start: {len(reached)} (bs, n, m, sum - n 2^m) boundary points")

    # enc_split_walk: directions, steps, fs 14 and 15, local minima
    kinds = Counter()
    for c in B.enc_split_walk():
        for s, d, w in walks(c):
            kinds["tie at the first pair" if w.tie0 else f"dir {w.dir:+d} steps {w.steps} equal {w.tie_steps}"] += 1
            if w.fs >= 14:
                kinds[f"fs {w.fs} from start {w.start}"] += 1
            if w.fs == 13:
                kinds[f"fs 13 from start {w.start}"] += 1
            if w.fs == 0 or w.start == 0:
                kinds[f"start 0 dir {w.dir:+d}"] += 1
    for k in ("tie at the first pair", "dir -1 steps 0 equal 0", "dir +1 steps 0 equal 0", "dir +1 steps 1 equal 0",
              "dir +1 steps 1 equal 1", "fs 14 from start 12", "fs 14 from start 13", "fs 14 from start 14",
              "fs 15 from start 14", "fs 13 from start 11", "fs 13 from start 12", "fs 13 from start 13",
              "start 0 dir -1", "start 0 dir +1"):
        assert kinds[k] >= 2, (k, kinds)
    print(f"enc_split_walk: {dict(kinds)}")

    # enc_emit_paths: 2k + q per fs and shape in exactly one lane of the wave, long even runs, header phases
    hit, phases, long_even = Counter(), Counter(), 0
    cases = {c.what: c for c in B.enc_emit_paths()}
    for what, cfg, dsubs, meta in B.enc_emit_paths_fields():
        c = cases[what]
        spl = B.enc_template(cfg.bs)[0]
        at = B.layout(cfg, c.fields)
        groups = B.wave_groups(cfg, c.fields)
        for idx, label in meta:
            s = c.fields.subs[idx]
            assert isinstance(s, B.Rice), what
            q = np.array([x for x, _ in s.codes])
            k = s.fs + 1
            lane_max = [int(q[lo:lo + spl][1::2].max()) for lo in range(0, len(q), spl) if len(q[lo:lo + spl]) > 1]
            top = max(lane_max)
            others = [i for g in groups if idx in g for i in g if i != idx]
            rest = max([2 * (o.fs + 1) + max(x for x, _ in o.codes[1::2]) for o in (c.fields.subs[i] for i in others)
                        if isinstance(o, B.Rice) and len(o.codes) > 1] + [0])
            if label == "long_even":
                assert q[0::2].max() >= 1000 and top <= 1
                long_even += 1
                continue
            assert label == (s.fs, 2 * k + top) and lane_max.count(top) == 1 and rest <= 30, (what, label)
            hit[cfg.bs, s.fs, 2 * k + top] += 1
            phases[at[idx].header % 32] += 1
    for bs in B.EMIT_FULL + B.EMIT_RAGGED:
        # (the run alone adds q 2^fs / n to the average delta, and the rule leaves fs once the average passes
        # 2^(fs + 2): every point whose run is at most 1.5 n is asked for, so every point from bs 22 on)
        missing = [(fs, T) for fs in range(14) for T in B.EMIT_T
                   if not hit[bs, fs, T] and T - 2 * (fs + 1) <= 1.5 * bs]
        assert not missing, (bs, missing)
    assert all(hit_fs for hit_fs in (any(hit[bs, fs, T] for bs in B.EMIT_FULL) for fs in range(14) for T in B.EMIT_T))
    assert all(phases[p] for p in range(32)) and long_even >= 6
    print(f"enc_emit_paths: {len(hit)} (bs, fs, 2k + q) points, {long_even} sub-blocks with an even run of 1000 and "
          f"more, header phases {len(phases)}")

    # enc_flush_edges: the complete words at a flush decision, flushes per stream, worst case, total bits mod 32
    words, residues, templates = Counter(), Counter(), set()
    for c in B.enc_flush_edges():
        w, flushes = B.flush_trace(c.cfg, c.fields)
        assert flushes >= 3, (c.what, flushes)
        total = B.layout(c.cfg, c.fields)[-1].end
        if "all raw" in c.what:
            assert len(c.stream) == B.worst_case_bytes(c.cfg, c.n_samples), c.what
            templates.add(B.enc_template(c.cfg.bs) + (c.cfg.cs,))
            assert max(w) >= (512 if c.cfg.bs > 64 else 256)
        else:
            words.update(w)
            residues[total % 32] += 1
    assert all(words[x] >= 8 for x in B.FLUSH_WORDS), words
    assert all(residues[r] for r in range(32))
    assert templates == {(spl, g, cs) for spl, g in ((8, 1), (8, 2), (8, 4), (8, 8), (16, 8), (16, 16), (16, 32))
                         for cs in (1, 2)}
    print(f"enc_flush_edges: complete words at a flush decision {dict((x, words[x]) for x in B.FLUSH_WORDS)}, "
          f"{len(templates)} all-raw templates")

    # enc_shapes: every (bs, cs, format, n)
    shapes = Counter((c.cfg, c.n_samples) for c in B.enc_shapes())
    for bs in B.SHAPE_BS:
        for cs in (1, 2):
            for big, ulsb in B.SHAPE_CFG:
                assert all(shapes[B.Cfg(bs, cs, big, ulsb), n] == 1 for n in B.shape_ns(bs, cs))
    kinds = Counter(type(s).__name__ if not isinstance(s, B.Rice) else s.fs for c in B.enc_shapes() for s in c.fields.subs)
    assert kinds["Zero"] > 50 and kinds["Raw"] > 50 and sum(1 for f in range(14) if kinds[f]) >= 12, kinds
    print(f"enc_shapes: {len(shapes)} (config, n), sub-block kinds {dict(kinds)}")

    # enc_segments: units of 16 chunks, o_1 and o_k residues, minimal middles, short last segments, size mod 4
    by_cfg = Counter()
    for c in B.enc_segments():
        by_cfg[c.cfg] += c.n_samples
    for cfg, total in by_cfg.items():  # (one launch per config: the rule of enc_seg_chunks on its chunk count)
        assert total // (cfg.bs * cfg.cs) // 32 < B.ENC_TARGET_UNITS and B.seg_chunks_rule(total, cfg) == 16
    o1, ok, minimal, short2, short3, masked, mod4, nsegs = Counter(), Counter(), 0, Counter(), Counter(), 0, Counter(), Counter()
    for (what, cfg, first, dsubs, aim), c in zip(B.enc_segments_fields(), B.enc_segments()):
        o, L = B.segments_of(cfg, c.fields)
        nseg = len(o)
        assert 2 <= nseg <= 5, what
        nsegs[cfg.cs, nseg] += 1
        o1[cfg.cs, o[1] % 32] += 1
        for k in range(2, nseg):
            ok[o[k] % 32] += 1
        minimal += sum(1 for k in range(1, nseg - 1) if L[k] == 64 * cfg.cs)
        mod4[len(c.stream) % 4] += 1
        if aim[0].startswith("short"):
            bits = 4 * cfg.cs if aim[1] == "4cs" else int(aim[1])
            assert L[-1] == bits, (what, L)
            (short2 if nseg == 2 else short3)[aim[1]] += 1
            masked += nseg == 2 and L[1] < 32 - o[1] % 32
    assert all(o1[cs, r] for cs in (1, 2) for r in range(32)) and all(ok[r] for r in range(32))
    assert minimal >= 16 and masked >= 8 and all(mod4[r] for r in range(4))
    assert all(short2[n] and short3[n] for n in B.SEG_SHORT) and all(nsegs[cs, k] for cs in (1, 2) for k in (2, 3, 4, 5))
    print(f"enc_segments: o_1 % 32 {len(o1)} (cs, residue), o_k % 32 {len(ok)}, minimal middle segments {minimal}, "
          f"short last {dict(short2)} / {dict(short3)}, L_1 < 32 - sh in {masked}, size % 4 {dict(mod4)}")

    # enc_values
    names = " ".join(c.what for c in B.enc_values())
    assert "0 to 0xffff" in names and any(c.inp is not None for c in B.enc_values())
    raws = sum(isinstance(s, B.Raw) and isinstance(t, (B.Rice, B.Zero)) for c in B.enc_values() if c.cfg.cs == 1
               for s, t in zip(c.fields.subs, c.fields.subs[1:]))
    assert raws >= 8


# ---------------------------------------------------------------------------------------------------------------
# an encoder of its own, and wrong ones
# ---------------------------------------------------------------------------------------------------------------

def write(cfg: B.Cfg, samples: np.ndarray, start_eq=0, start_below=0, tie_walks=False, strict=False, bound=14,
          clamp13=False, raw_le=False, global_min=False, wide=False, raw_pixels=False, zero_on_stored=False,
          last_from_stored=False, ragged_as_bs=False) -> bytes:
    """encode.h:43-157 and codec.h:62-101 through ``B.build``; the keyword arguments make the wrong writers."""
    n = len(samples)
    if n == 0:
        return B.build(cfg, B.Fields((0,) * cfg.cs, ()))
    px = np.array([B.px_read(cfg, int(v)) for v in samples], np.int64)
    last = [int(px[c]) for c in range(cfg.cs)]
    init = tuple(last)
    subs = []
    for base in range(0, n, cfg.cs * cfg.bs):
        cnt = min(n - base, cfg.cs * cfg.bs) // cfg.cs
        for c in range(cfg.cs):
            p = px[base + c:base + cfg.cs * cnt:cfg.cs]
            st = samples[base + c:base + cfg.cs * cnt:cfg.cs]
            diff = np.diff(np.concatenate(([last[c]], p)))
            if not wide:
                diff = (diff + 32768) % 65536 - 32768
            d = np.where(diff >= 0, diff << 1, (-diff << 1) - 1)
            last[c] = int(p[-1])
            nonzero = bool(d.any()) or (zero_on_stored and len(set(st.tolist())) > 1)
            if not nonzero:
                subs.append(B.Zero(cnt))
                continue
            total, size = int(d.sum()), (cfg.bs if ragged_as_bs else cnt)
            cost = lambda f: B.split_cost(d, f)
            q = total // size
            if start_eq and q and total == size << (q.bit_length() - 1):
                q -= 1  # (bit_width one short exactly at sum == n 2^t)
            if start_below and q and total == (size << q.bit_length()) - 1:
                q += 1  # (bit_width one long exactly at sum == n 2^t - 1)
            start = max(0, q.bit_length() - 2)
            if clamp13:
                start = min(start, 13)
            b0, b1 = cost(start), cost(start + 1)
            cand, bits, direction = (start + 1, b1, 1) if b1 <= b0 else (start, b0, -1)
            if b0 != b1 or tie_walks:
                while 0 < cand < bound:
                    t = cost(cand + direction)
                    if t > bits or (strict and t == bits):
                        break
                    bits, cand = t, cand + direction
            if global_min:
                bits, cand = min((cost(f), f) for f in range(16))
            if cand < 14 and (bits <= 16 * cnt if raw_le else bits < 16 * cnt):
                mask = (1 << cand) - 1
                subs.append(B.Rice(cand, tuple((int(x) >> cand, int(x) & mask) for x in d)))
            else:
                subs.append(B.Raw(tuple(int(x) for x in (p if raw_pixels else st))))
                if last_from_stored:
                    last[c] = int(st[-1])
    return B.build(cfg, B.Fields(init, tuple(subs)))


def test_the_restated_writer_agrees_on_every_case():
    for fam in B.ENC_FAMILIES.values():
        for c in fam():
            assert write(c.cfg, inp(c)) == c.stream, c.what


WRONG_WRITERS = [
    ("start one low at sum == n 2^t", "enc_split_start", dict(start_eq=1)),
    ("a tie at the first pair keeps walking", "enc_split_start", dict(tie_walks=True)),
    ("ragged n taken as bs in the start", "enc_split_start", dict(ragged_as_bs=True)),
    ("< for <= in the walk", "enc_split_walk", dict(strict=True)),
    ("walk bound 13 for 14", "enc_split_walk", dict(bound=13)),
    ("global minimum instead of the hill climb", "enc_split_walk", dict(global_min=True)),
    ("17-bit differences", "enc_values", dict(wide=True)),
    ("raw stores the pixel instead of the stored sample", "enc_values", dict(raw_pixels=True)),
    ("zero sub-block decided on stored samples instead of pixels", "enc_values", dict(zero_on_stored=True)),
    ("last after raw taken from the stored sample", "enc_values", dict(last_from_stored=True)),
]


@pytest.mark.parametrize("name,family,kw", WRONG_WRITERS, ids=[w[0] for w in WRONG_WRITERS])
def test_wrong_writers_are_caught(name, family, kw):
    caught = []
    for c in B.ENC_FAMILIES[family]():
        try:
            same = write(c.cfg, inp(c), **kw) == c.stream
        except AssertionError:  # (a code the writer refuses, such as a 17-bit raw value)
            same = False
        if not same:
            caught.append(c.what)
    print(f"{name}: caught by {len(caught)} cases of {family}, the first: {caught[:1]}")
    assert caught, f"{name}: no case of {family} tells it from the right writer"


SAME_WRITERS = [
    ("start one high at sum == n 2^t - 1", dict(start_below=1)),
    ("a start clamp that never reaches 14", dict(clamp13=True)),
    ("raw at bits <= 16 n (the same as bits < 16 n + 1)", dict(raw_le=True)),
]


@pytest.mark.parametrize("name,kw", SAME_WRITERS, ids=[w[0] for w in SAME_WRITERS])
def test_variants_that_are_the_same_writer(name, kw):
    """Three variants no input can tell from the right writer.  At sum == n 2^t - 1 the deltas in units of
    2^start average just under 4, so cost(start) - cost(start + 1) = sum(ceil(floor(x) / 2)) - n > n / 2: no equal
    cost lies at `start`, and as the cost is convex in fs both starts end at the same fs.  A start of 14 means avg >= 2^15; clamped to 13 the
    first pair is (13, 14) and cost(13) = 14 n + sum(d >> 13) >= 14 n + (4 n - n) > 16 n, so the sub-block is raw
    whether 13 is kept or 14 taken.  And fs < 14 implies bits < 16 n (ricepp_build's note), so bits == 16 n never
    meets the comparison.  Shown on the families that hold the starts 12..14 and the raw sub-blocks."""
    for family in ("enc_split_start", "enc_split_walk", "enc_values", "enc_flush_edges"):
        for c in B.ENC_FAMILIES[family]()[:40 if family == "enc_flush_edges" else 600]:
            assert write(c.cfg, inp(c), **kw) == c.stream, c.what
