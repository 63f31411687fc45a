"""GPU tests of the ricepp encode kernels on constructed inputs (tests/ricepp_build.py, the ``enc_*`` families).
The expected bytes are ``case.stream``, built from the field lists and proved canonical on the CPU by
tests/test_ricepp_encode_constructed_host.py; nothing here is compared with the oracle, the GPU decoder or the
GPU's own output.  Every family is one launch per config, through ``rpp_encode_batch`` called directly (one wave
per stream, never split) and through ``codec.encode_batch`` (``rpp_encode_batch_ws``: a stream of more than 16
chunks is split in these small batches), each once with every stream 16-byte aligned (the vector loads) and once
at sample offsets 1..7 (the per-sample loads).  The output buffer holds 0xA5 before the launch; every region
starts 16-aligned, has the worst-case capacity and 48 guard bytes behind it.  include/ricepp_amd.h promises
nothing about the bytes between a stream's size and its capacity, so those touched are counted and printed."""

import ctypes as C
import time
from collections import defaultdict

import numpy as np
import pytest
import torch

import ricepp_build as B
from dwarfs_amd import _native as N
from dwarfs_amd import codec

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 48
FILL = 0xA5


def _p(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _u64(v) -> torch.Tensor:
    return torch.as_tensor(np.asarray(v, np.int64), device=DEV)


def pack(cases, aligned: bool):
    """The inputs in one int16 tensor: each stream 16-byte aligned, or at sample offsets 1..7 in turn."""
    parts, offs, at = [], [], 0
    for i, c in enumerate(cases):
        start = (at + 7) // 8 * 8 + (0 if aligned else 1 + i % 7)
        parts.append(np.full(start - at, 0x7E7E, np.uint16))
        parts.append(c.want if c.inp is None else c.inp)
        offs.append(start)
        at = start + c.n_samples
    parts.append(np.full(16, 0x7E7E, np.uint16))
    flat = np.concatenate(parts).astype(np.uint16)
    return torch.from_numpy(flat.view(np.int16)).to(DEV), offs


def encode(cfg: B.Cfg, cases, entry: str, aligned: bool):
    """One launch: (statuses, sizes, the whole output buffer, region offsets, capacities)."""
    ccfg = codec.CodecConfig(cfg.bs, cfg.cs, "big" if cfg.big else "little", cfg.ulsb)
    d_in, in_offs = pack(cases, aligned)
    ns = [c.n_samples for c in cases]
    caps = [B.worst_case_bytes(cfg, n) for n in ns]
    out_offs, at = [], GUARD
    for cap in caps:
        out_offs.append(at)
        at = (at + cap + GUARD + 15) // 16 * 16
    out = torch.full((at + 16,), FILL, dtype=torch.uint8, device=DEV)
    if entry == "plain":
        c = ccfg.native()
        sizes = torch.full((len(ns),), -1, dtype=torch.int64, device=DEV)
        st = torch.full((len(ns),), 99, dtype=torch.int32, device=DEV)
        d_off, d_n, d_oo = _u64(in_offs), _u64(ns), _u64(out_offs)
        r = N.lib().rpp_encode_batch(C.byref(c), _p(d_in), _p(d_off), _p(d_n), len(ns), _p(out), _p(d_oo), _p(sizes),
                                     _p(st), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert r == N.RPP_OK
    else:
        enc = codec.encode_batch(ccfg, d_in, in_offs, ns, out=out, out_offsets=np.asarray(out_offs, np.int64))
        sizes, st = enc.sizes, enc.status
    torch.cuda.synchronize()
    return st.cpu().numpy(), sizes.cpu().numpy(), out.cpu().numpy(), out_offs, caps


def check(family: str, cases, entries=("plain", "ws")):
    by_cfg = defaultdict(list)
    for c in cases:
        by_cfg[c.cfg].append(c)
    t0 = time.perf_counter()
    launches, slack = 0, 0
    for cfg, group in by_cfg.items():
        for entry in entries:
            for aligned in (True, False):
                st, sizes, host, offs, caps = encode(cfg, group, entry, aligned)
                launches += 1
                how = (family, cfg, entry, "aligned" if aligned else "offsets 1..7")
                outside = np.ones(len(host), bool)
                bad = []
                for c, s, n, o, cap in zip(group, st, sizes, offs, caps):
                    outside[o:o + cap] = False
                    if s != N.RPP_OK or n != len(c.stream) or host[o:o + len(c.stream)].tobytes() != c.stream:
                        bad.append((c.what, int(s), int(n), len(c.stream)))
                    else:
                        slack += int((host[o + len(c.stream):o + cap] != FILL).sum())
                assert (host[outside] == FILL).all(), (how, "a byte outside every region was written")
                assert not bad, (how, len(bad), bad[:6])
    print(f"{family}: {len(cases)} streams, {sum(c.n_samples for c in cases)} samples, {launches} launches, "
          f"{time.perf_counter() - t0:.2f} s, {slack} bytes touched between size and capacity (no promise made)")


def test_enc_split_start():
    """n deltas 2^m and one of them off by one, every n of bs 16 and 29: the division-free start."""
    check("enc_split_start", B.enc_split_start())


def test_enc_split_walk():
    """Every walk the split rule takes; fs 14 and 15 are raw."""
    check("enc_split_walk", B.enc_split_walk())


def test_enc_emit_paths():
    """2k + q of 31, 32, 33 and 34 in one lane of the wave at every fs; runs of 1000 zeros; every header phase."""
    check("enc_emit_paths", B.enc_emit_paths())


def test_enc_flush_edges():
    """One wave per stream: 255..257 and 271..273 complete words at a flush decision, all-raw worst cases."""
    check("enc_flush_edges", B.enc_flush_edges(), entries=("plain",))


def test_enc_shapes():
    """Every block size and stream length at which the kernel's shape or its ragged handling changes."""
    check("enc_shapes", B.enc_shapes())


def test_enc_values():
    """Extreme differences, wraps, dirt in unused low bits, raw then Rice and zero, both byte orders."""
    check("enc_values", B.enc_values())


def test_enc_segments():
    """Streams split into units of 16 chunks: every o_1 % 32 and o_k % 32, minimal middles, short last segments."""
    cases = B.enc_segments()
    by_cfg = defaultdict(int)
    for c in cases:
        by_cfg[c.cfg] += c.n_samples
    assert all(B.seg_chunks_rule(total, cfg) == 16 for cfg, total in by_cfg.items())
    check("enc_segments", cases, entries=("ws",))


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_enc_segments_mixed_batch(order):
    """Split and unsplit streams interleaved, with a stream of no samples and one of exactly 16 chunks."""
    for cfg in (B.Cfg(16, 1, True, 0), B.Cfg(29, 2, False, 0)):
        split = [c for c in B.enc_segments() if c.cfg == cfg][::9]
        short = [c for c in B.enc_split_start() if c.cfg == cfg][:40]
        empty = B.enc_case(f"no samples {cfg}", cfg, (0,) * cfg.cs, [])
        chunk = cfg.bs * cfg.cs
        exact = B.enc_case(f"exactly 16 chunks {cfg}", cfg, (5,) * cfg.cs, B.dial(cfg, 16, 2 * cfg.bs + 7))
        assert exact.n_samples == 16 * chunk and empty.n_samples == 0 and empty.stream == bytes(2 * cfg.cs)
        assert all(c.n_samples > 16 * chunk for c in split) and all(0 < c.n_samples < 16 * chunk for c in short)
        mixed = [exact]
        for i, c in enumerate(split):
            mixed += [c, short[i % len(short)]]
        mixed.insert(len(mixed) // 2, empty)
        assert B.seg_chunks_rule(sum(c.n_samples for c in mixed), cfg) == 16
        check(f"enc_segments mixed {order}", mixed[::-1] if order == "reversed" else mixed, entries=("ws",))
