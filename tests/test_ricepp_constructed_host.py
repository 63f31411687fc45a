"""CPU tests of the constructed ricepp streams (tests/ricepp_build.py; no GPU needed): every stream of every
family through the CPU oracle, the compiled reference where there is one, and a small reader written here; the
counts that say each family reaches the kernel edges it aims at; and deliberately wrong variants of the reader,
each of which must be caught by the family aimed at it.  The expected samples come from the field lists
(``ricepp_build.expand``).  The same families run on the GPU in tests/test_gpu_ricepp_constructed.py."""

from collections import Counter

import numpy as np
import pytest

import ricepp_build as B
from oracle import oracle as O
from oracle import reference as R

# streams per family: a change of a family shows here
FAMILY_SIZES = {"density": 252, "window_edges": 372, "long_runs": 496, "class_pairs": 2048, "values": 504,
                "end_of_input": 304, "decoys": 90}


class Truncated(Exception):
    pass


def read(c: B.Case, diff_bits=32, last_bits=None, behind=False, by_bytes=False, run_cap=None, raw_px_read=True,
         swap_ragged=False):
    """decode.h:42-83 over bitstream_reader.h, one field at a time; a unary run is searched bit by bit.  The
    keyword arguments turn it into the wrong readers of test_wrong_readers_are_caught.  (status, samples)."""
    cfg, n, nb = c.cfg, c.n_samples, c.size
    limit = 8 * nb if by_bytes else 64 * ((nb + 7) // 8)
    data = c.stream[:nb] if not behind else c.stream + b"\xff" * 16
    data = data[:limit // 8].ljust(limit // 8, b"\0")
    word = int.from_bytes(data, "little")
    bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little").tobytes()
    pos = 0

    def take(k):
        nonlocal pos
        if pos + k > limit:
            raise Truncated
        v = (word >> pos) & ((1 << k) - 1)
        pos += k
        return v

    def run():
        nonlocal pos
        t = bits.find(b"\x01", pos)
        if t < 0:
            raise Truncated
        q, pos = t - pos, t + 1
        return q if run_cap is None else min(q, run_cap)

    out = np.zeros(n, np.uint16)
    mask = B.M32 if last_bits is None else (1 << last_bits) - 1
    try:
        last = [take(16) & mask for _ in range(cfg.cs)]
        for base in range(0, n, cfg.cs * cfg.bs):
            cnt = min(n - base, cfg.cs * cfg.bs) // cfg.cs
            for comp in range(cfg.cs):
                k = cfg.cs - 1 - comp if swap_ragged and cnt < cfg.bs else comp
                head = take(4)
                for i in range(cnt):
                    if head == 15:
                        v = take(16)
                        if i == cnt - 1:
                            last[k] = (B.px_read(cfg, v) if raw_px_read else v) & mask
                    else:
                        if head:
                            d = ((run() << (head - 1)) | take(head - 1)) & ((1 << diff_bits) - 1)
                            last[k] = (last[k] + ((d >> 1) ^ (B.M32 if d & 1 else 0))) & mask
                        v = B.px_write(cfg, last[k])
                    out[base + k + cfg.cs * i] = v
    except Truncated:
        return B.TRUNCATED, None
    return B.OK, out


def agrees(c: B.Case, got) -> bool:
    st, out = got
    return st == c.status and (st != B.OK or np.array_equal(out, c.want))


def ocfg(cfg: B.Cfg):
    return O.cfg(cfg.bs, cfg.cs, cfg.big, cfg.ulsb)


def decode_with(mod, c: B.Case):
    try:
        return B.OK, mod.decode(ocfg(c.cfg), c.stream[:c.size], c.n_samples)
    except O.OracleError as e:
        return e.status, None


def test_writer():
    cfg = B.Cfg(4, 1, False, 0)
    f = B.Fields((0x1234,), (B.Rice(2, ((0, 3), (2, 1), (0, 0), (1, 2))), B.Zero(4), B.Raw((1, 2, 0xFFFF))))
    # 0x1234, header 3, codes 1|11, 001|10, 1|00, 01|01, header 0, header 15, three values
    want_bits = ("0010110001001000" "1100" "111" "00110" "100" "0101" "0000" "1111" "1000000000000000"
                 "0100000000000000" "1111111111111111")
    assert B.build(cfg, f) == np.packbits(np.array(list(want_bits), np.uint8), bitorder="little").tobytes()
    at = B.layout(cfg, f)
    assert (at[0].header, at[0].terms.tolist(), at[0].end) == (16, [20, 25, 28, 32], 35)
    assert (at[1].kind, at[1].header, at[2].kind, at[2].header, at[2].end) == ("zero", 35, "raw", 39, 91)
    # differences 3, 9, 0, 6 -> -2, -5, 0, +3
    assert B.expand(cfg, f).tolist() == [0x1232, 0x122D, 0x122D, 0x1230] + [0x1230] * 4 + [1, 2, 0xFFFF]
    big = B.Cfg(4, 1, True, 3)
    assert B.expand(big, B.Fields((0xE001,), (B.Zero(4),))).tolist() == [0x0800] * 4  # (0xE001 << 3) & 0xFFFF, swapped
    assert B.expand(big, B.Fields((0,), (B.Raw((0x3412,) * 4), B.Zero(2)))).tolist() == [0x3412] * 4 + [0x3012] * 2
    for cs in (1, 2):
        for bs in (16, 29, 128):
            for mis in range(4):
                c = B.Cfg(bs, cs)
                for bit in range(8 * mis + 16 * cs + 4 + bs + 4 * cs, 8 * mis + 16 * cs + 600, 7):
                    subs = B.place(c, mis, bit) + [B.Zero(bs)] * cs
                    assert B.layout(c, B.Fields((0,) * cs, tuple(subs)))[-cs].header + 8 * mis == bit
                for phase in range(96):
                    subs = B.place(c, mis, phase, modulo=96) + [B.Zero(bs)] * cs
                    assert (B.layout(c, B.Fields((0,) * cs, tuple(subs)))[-cs].header + 8 * mis) % 96 == phase
    # cut: the fields a reader sees of fewer bytes
    st, seen = B.cut(cfg, f, 11)  # 88 bits: the last raw value loses its 3 high bits
    assert st == B.OK and seen.subs[2] == B.Raw((1, 2, 0x1FFF)) and seen.subs[:2] == f.subs[:2]
    assert B.cut(cfg, f, 3)[0] == B.TRUNCATED  # inside the second code's run: no terminator before the packet ends
    st, seen = B.cut(cfg, f, 2)  # every header reads 0
    assert st == B.OK and seen.subs == (B.Zero(4), B.Zero(4), B.Zero(3))
    assert B.cut(cfg, f, 0)[0] == B.TRUNCATED


@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_family_on_the_cpu_readers(family):
    """The oracle and this file's reader return every case's status and samples; where the stream is what the
    encoder writes for its samples, the oracle's encoder gives back its bytes."""
    cases = B.FAMILIES[family]()
    assert len(cases) == FAMILY_SIZES[family]
    assert len({c.what for c in cases}) == len(cases)
    canonical = 0
    for c in cases:
        assert len(c.stream) <= 16 * 1024 + 64 and c.n_samples <= 6000, c.what  # (128 Kib)
        assert c.n_samples % c.cfg.cs == 0 and (c.want is None) == (c.status != B.OK), c.what
        assert agrees(c, decode_with(O, c)), c.what
        assert agrees(c, read(c)), c.what
        if family in ("class_pairs", "values") and c.status == B.OK and c.n_samples and c.in_bytes is None:
            canonical += O.encode(ocfg(c.cfg), c.want) == c.stream
    print(f"{family}: {len(cases)} streams, {sum(c.size for c in cases)} bytes, "
          f"{sum(c.n_samples for c in cases)} samples, {sum(c.status != B.OK for c in cases)} truncated, "
          f"{canonical} canonical")
    if family in ("class_pairs", "values"):
        assert canonical >= 4
    assert any(c.status == B.OK for c in cases)


@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_family_on_the_compiled_reference(family):
    if not R.available():
        pytest.skip("neither oracle/_ref/libdwarfs_ref.so nor the reference tree to build it from")
    for c in B.FAMILIES[family]():
        assert agrees(c, decode_with(R, c)), c.what


def test_long_runs_exceed_the_worst_case():
    for c in B.long_runs():
        assert c.status == B.OK and len(c.stream) > B.worst_case_bytes(c.cfg, c.n_samples), c.what
        assert B.worst_case_bytes(c.cfg, c.n_samples) == O.worst_case_bytes(ocfg(c.cfg), c.n_samples)


def test_families_reach_what_they_aim_at():
    """The geometry each family claims, counted from ``layout`` (positions from the 4-aligned word the kernels
    count from, so the stream's misalignment is part of them)."""
    # density: every bit phase of both segment widths for headers and terminators, segments that hold the most
    # terminators their fs allows, and segments that hold none between two that hold some
    head, term, fullest, empty = Counter(), Counter(), Counter(), Counter()
    for what, cfg, f, mis, pattern in B.density_fields():
        for at in B.layout(cfg, f):
            if at.kind != "rice" or len(at.terms) < cfg.bs:
                continue
            sb = B.seg_bits(at.fs)
            head[sb, (at.header + 8 * mis) % sb] += 1
            rel = at.terms - at.header  # (the window a kernel reads starts at the sub-block's header)
            for t in rel:
                term[at.fs, int(t) % sb] += 1
            per_seg = Counter((rel // sb).tolist())
            fullest[at.fs] = max(fullest[at.fs], max(per_seg.values()))
            if pattern == "full_empty":
                empty[at.fs] += sum(1 for s in range(max(per_seg)) if s not in per_seg)
    for sb in (24, 32):
        assert all(head[sb, p] for p in range(sb)), sb
    for fs in range(14):
        sb = B.seg_bits(fs)
        assert all(term[fs, p] for p in range(sb)), fs
        assert fullest[fs] == -(-sb // (fs + 1)) and empty[fs] > 0, (fs, fullest[fs], empty[fs])
    print(f"density: header phases {len(head)}, (fs, terminator phase) pairs {len(term)}, "
          f"fullest segment per fs {[fullest[fs] for fs in range(14)]}, empty segments {sum(empty.values())}")

    # window_edges: every end W-5..W+2 with every follower at both places, per window
    reached, multi = Counter(), Counter()
    for what, cfg, f, mis, meta in B.window_edges_fields():
        ats = B.layout(cfg, f)
        if len(meta) == 5:
            W, d, follower, where, aimed = meta
            assert ats[aimed].end - ats[aimed].header == W + d and ats[aimed + 1].header == ats[aimed].header + W + d
            assert int(ats[aimed].terms[-1]) + 1 + ats[aimed].fs == ats[aimed].end
            assert ats[aimed + 1].kind == {"zero": "zero", "raw": "raw"}.get(follower, "rice")
            reached[W, d, follower, where] += 1
        else:
            W, windows, d = meta
            assert ats[1].end - ats[1].header == windows * W + d
            multi[W, windows, d] += 1
    for W in B.EDGE_WINDOWS:
        for d in B.EDGE_ENDS:
            for follower in B.EDGE_FOLLOWERS:
                for where in B.EDGE_PLACES:
                    assert reached[W, d, follower, where], (W, d, follower, where)
        assert all(multi[W, k, d] for k in (2, 3) for d in (-1, 0, 1)), W
    print(f"window_edges: {len(reached)} (window, end, follower, place) combinations, {len(multi)} multi-window ends")

    # long_runs: every run at every place and fs; the packet-edge terminators; the ring's wrap and a refill chunk
    runs, wraps, chunks, packet = Counter(), 0, 0, set()
    for what, cfg, f, mis, (run, fs, where, at) in B.long_runs_fields():
        a = B.layout(cfg, f)[0]
        assert f.subs[0].codes[at][0] == run and a.fs == fs
        runs[run, fs, where] += 1
        t = int(a.terms[at])
        packet.add((where, t % 64))
        lo, hi = t - run + 8 * mis, t + 8 * mis
        wraps += lo // (32 * B.RING_WORDS) != hi // (32 * B.RING_WORDS)
        chunks += lo // (32 * B.CHUNK_WORDS) != hi // (32 * B.CHUNK_WORDS)
    assert all(runs[r, fs, w] for r in B.LONG_RUNS for fs in B.LONG_FS for w in B.LONG_WHERE)
    assert ("packet_bit_63", 63) in packet and ("packet_bit_0", 0) in packet
    assert wraps >= 6 * 3 * 6 and chunks >= wraps
    print(f"long_runs: {len(runs)} (run, fs, place) combinations, {wraps} runs across the ring's wrap, "
          f"{chunks} across a refill chunk")

    # class_pairs: all 256 ordered pairs per bs and cs, in the second component too, and a raw sub-block of one
    # component between Rice sub-blocks of the other
    pairs, second, raw_between = Counter(), Counter(), 0
    for what, cfg, f, mis, (a, b) in B.class_pairs_fields():
        kinds = [0 if isinstance(s, B.Zero) else 15 if isinstance(s, B.Raw) else s.fs + 1 for s in f.subs]
        assert kinds[0::cfg.cs] == [a] * 4 + [b] * 4 + [a]
        pairs[cfg.bs, cfg.cs, a, b] += 1
        if cfg.cs == 2:
            a2, b2 = B.second_pair(a, b)
            assert kinds[1::2] == [a2] * 4 + [b2] * 4 + [a2] and (a2, b2) != (a, b)
            second[cfg.bs, a2, b2] += 1
            raw_between += any(kinds[i] == 15 and 1 <= kinds[i - 1] <= 14 and 1 <= kinds[i + 1] <= 14
                               for i in range(1, len(kinds) - 1))
    assert len(pairs) == 4 * 2 * 256 and len(second) == 4 * 256 and raw_between > 100
    print(f"class_pairs: {len(pairs)} (bs, cs, A, B), {raw_between} streams with a raw sub-block between Rice ones of "
          f"the other component")

    # end_of_input: each cut, and what it falls into
    inside = Counter()
    for what, cfg, f, mis, (tail, end_bit, delta, nbytes) in B.end_of_input_fields():
        ats = B.layout(cfg, f)
        assert (ats[-1].end - 1) % 64 == end_bit
        cutbit = 8 * nbytes
        for at in ats:
            if at.header < cutbit < at.header + 4:
                inside["header", tail] += 1
            elif at.kind == "raw" and at.header + 4 < cutbit < at.end and (cutbit - at.header - 4) % 16:
                inside["raw value", tail] += 1
            elif at.kind == "rice":
                starts = np.concatenate(([at.header + 4], at.terms[:-1] + 1 + at.fs))
                inside["unary run", tail] += int(((starts < cutbit) & (cutbit <= at.terms)).any())
                inside["remainder", tail] += int(((at.terms + 1 < cutbit) & (cutbit < at.terms + 1 + at.fs)).any())
    deltas = {(m[0], m[2]) for *_, m in B.end_of_input_fields()}
    assert deltas == {(t, d) for t in B.END_TAILS for d in range(-9, 10)}
    for kind, tail in (("remainder", "remainders"), ("unary run", "unary"), ("header", "headers"), ("raw value", "raw")):
        assert inside[kind, tail] >= 4, (kind, tail, inside)
    sts = Counter(c.status for c in B.end_of_input())
    assert sts[B.OK] > 100 and sts[B.TRUNCATED] > 40
    print(f"end_of_input: cuts inside {dict(inside)}, statuses {dict(sts)}")

    # decoys: a chain of at least 30 sub-blocks, header values within a range of 4, shifted 1..15 bits, with a
    # decoy header (and 24 more behind it) closely behind a unit boundary of 2^10 and of 2^12 bits
    near = Counter()
    for what, cfg, f, mis, (start, headers, nraw) in B.decoys_fields():
        true0 = 16 * cfg.cs
        assert 1 <= start - true0 - 4 <= 15 and len(headers) >= 30 > B.SPEC_VERIFY > B.SPEC_STEPS
        assert headers[-1] < true0 + nraw * (4 + 16 * cfg.bs)
        for L in (10, 12):
            for h in headers[:len(headers) - B.SPEC_VERIFY]:
                if (h + 8 * mis) % (1 << L) < 4 + 16 * cfg.bs:
                    near[L, cfg.bs, cfg.cs] += 1
                    break
    assert max(B.DECOY_FS) - min(B.DECOY_FS) < 4
    assert all(near[L, bs, cs] >= 10 for L in (10, 12) for bs, cs in B.DECOY_CONFIGS), near
    print(f"decoys: streams with a decoy header within a raw sub-block's length behind a unit boundary: {dict(near)}")


WINDOWS = (B.WIN_ROWS, B.WIN24, B.WIN32)
WRONG_READERS = [
    ("differences kept in 16 bits", "long_runs", dict(diff_bits=16)),
    ("bytes behind in_bytes read instead of zeros", "end_of_input", dict(behind=True)),
    ("truncation judged by bytes instead of 8-byte packets", "end_of_input", dict(by_bytes=True)),
    ("a unary run capped at 65535", "long_runs", dict(run_cap=65535)),
] + [(f"a unary run capped at one window of {w} bits", "long_runs", dict(run_cap=w)) for w in WINDOWS] + [
    ("last after a raw sub-block taken without px_read", "values", dict(raw_px_read=False)),
    ("component order swapped in a ragged chunk", "values", dict(swap_ragged=True)),
]


@pytest.mark.parametrize("name,family,kw", WRONG_READERS, ids=[w[0] for w in WRONG_READERS])
def test_wrong_readers_are_caught(name, family, kw):
    """Each wrong reader disagrees with the wanted result on at least one case of the family aimed at it."""
    caught = [c.what for c in B.FAMILIES[family]() if not agrees(c, read(c, **kw))]
    print(f"{name}: caught by {len(caught)} cases of {family}, the first: {caught[:1]}")
    assert caught, f"{name}: no case of {family} tells it from the right reader"


def test_last_kept_in_16_minus_ulsb_bits_is_the_same_reader():
    """`last` kept in 16 - ulsb bits before the shift is no wrong reader: the stored sample is
    (uint16)(last << ulsb), which drops every bit of last from 16 - ulsb up, sums mod 2^k do not depend on higher
    bits, and px_read yields 16 - ulsb bits.  No stream can tell the two apart; the family with initial values
    above 16 - ulsb and wraps through 0xFFFF >> ulsb shows it."""
    cases = [c for c in B.values() if c.cfg.ulsb]
    assert len(cases) > 100
    for c in cases:
        assert agrees(c, read(c, last_bits=16 - c.cfg.ulsb)), c.what
