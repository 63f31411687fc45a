"""GPU tests of the ricepp decode kernels on constructed streams (tests/ricepp_build.py): every family is one
codec.decode_batch per config and decode path over all its streams, packed at byte offsets of every residue mod 4
with 0xFF between them, the outputs 8-aligned with guard samples between them.  The expected samples come from
the field lists, checked on the CPU against the oracle, the compiled reference and an independent reader by
tests/test_ricepp_constructed_host.py; nothing here is compared with the GPU's own output, with the GPU encoder
or with the oracle."""

import time
from collections import defaultdict

import numpy as np
import pytest
import torch

import ricepp_build as B
from dwarfs_amd import codec

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 8         # samples between two outputs
FILL = 0x5AA5     # what the output buffer holds before the launch

PATHS = {
    "auto": None,
    "fused": codec.DecodeOptions(path="fused"),
    "seg10": codec.DecodeOptions(path="segmented", seg_log2=10),
    "seg13": codec.DecodeOptions(path="segmented", seg_log2=13),
    "seg10_general": codec.DecodeOptions(path="segmented", seg_log2=10, test_flags=codec.N.RPP_TEST_NO_FAST_LANES),
}


def pack(cases):
    """The streams at byte offsets of the misalignment each case asks for, 0xFF in the gaps and behind."""
    buf, offs = bytearray(b"\xff" * 4), []
    for c in cases:
        buf += b"\xff" * ((c.mis - len(buf)) % 4)
        offs.append(len(buf))
        buf += c.stream + b"\xff" * 5
    buf += b"\xff" * 64
    return torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(DEV), offs


def decode(cfg, cases, options):
    """One decode_batch: (statuses, output regions as uint16, True if every guard sample is untouched)."""
    d_in, in_offs = pack(cases)
    out_offs, at = [], GUARD
    for c in cases:
        out_offs.append(at)
        at += (c.n_samples + GUARD + 7) // 8 * 8
    out = torch.full((at,), FILL, dtype=torch.int16, device=DEV)
    sizes = [c.n_samples for c in cases]
    ccfg = codec.CodecConfig(cfg.bs, cfg.cs, "big" if cfg.big else "little", cfg.ulsb)
    _, st = codec.decode_batch(ccfg, d_in, in_offs, [c.size for c in cases], sizes, out=out, out_offsets=out_offs,
                               options=options)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint16)
    mask = np.ones(at, bool)
    for o, n in zip(out_offs, sizes):
        mask[o:o + n] = False
    return st.cpu().numpy(), [host[o:o + n] for o, n in zip(out_offs, sizes)], bool((host[mask] == FILL).all())


def check(cases, path, batch=None):
    """The cases by config, each config's in one launch (or in launches of ``batch`` streams)."""
    by_cfg = defaultdict(list)
    for c in cases:
        by_cfg[c.cfg].append(c)
    codec.segmented_decode_stats(reset=True)
    t0 = time.perf_counter()
    bad_status, bad_samples, launches = [], [], 0
    for cfg, group in by_cfg.items():
        step = batch or len(group)
        for k in range(0, len(group), step):
            part = group[k:k + step]
            st, outs, intact = decode(cfg, part, PATHS[path])
            launches += 1
            assert intact, (cfg, path, "a guard sample was written")
            bad_status += [(c.what, int(s), c.status) for c, s in zip(part, st) if s != c.status]
            bad_samples += [c.what for c, s, got in zip(part, st, outs)
                            if c.status == B.OK and s == B.OK and not np.array_equal(got, c.want)]
    stats = codec.segmented_decode_stats(reset=True)
    print(f"{path}: {len(cases)} streams, {sum(c.n_samples for c in cases)} samples, {launches} launches, launch "
          f"and copies {time.perf_counter() - t0:.3f} s, segmented counters {stats}")
    assert not bad_status, (path, len(bad_status), bad_status[:8])
    assert not bad_samples, (path, len(bad_samples), bad_samples[:8])
    return stats


@pytest.mark.parametrize("path", list(PATHS))
def test_density(path):
    """Every fs at bs 16..256 with the most terminators a segment holds, a terminator on every bit of a segment,
    and full segments alternating with empty ones, the headers at every bit phase."""
    check(B.density(), path)


@pytest.mark.parametrize("path", list(PATHS))
def test_window_edges(path):
    """Sub-blocks that end 5 bits before to 2 bits behind the end of the 384-, 1536- and 2048-bit window, and ones
    of exactly two and three windows."""
    check(B.window_edges(), path)


@pytest.mark.parametrize("path", list(PATHS))
def test_long_runs(path):
    """Unary runs of 23 to 70000 zeros, longer than a segment, a window and the whole ring; q << fs past 2^16 and
    2^17.  The streams are longer than the worst case of their sample count, so the segmented decode, whose
    regions end there (seg_last_bit), must hand them to the fused kernel."""
    stats = check(B.long_runs(), path)
    if path.startswith("seg"):
        assert stats["fallback"] > 0, stats


@pytest.mark.parametrize("path", list(PATHS))
def test_class_pairs(path):
    """A A A A B B B B A for every ordered pair of the 16 kinds of sub-block, bs 16..128, one and two components."""
    check(B.class_pairs(), path)


@pytest.mark.parametrize("path", list(PATHS))
def test_values(path):
    """Zig-zag extremes, wraps of last, initial values above 16 - ulsb, raw with dirty low bits then Rice and zero,
    ulsb 0, 3, 15, both byte orders, ragged last chunks, n = 0 and n = cs."""
    check(B.values(), path)


@pytest.mark.parametrize("path", list(PATHS))
def test_end_of_input(path):
    """in_bytes from 9 short to 9 long, 0xFF behind it: zeros up to the end of the last 8-byte packet, truncated
    exactly when a consumed bit lies behind that."""
    check(B.end_of_input(), path)


@pytest.mark.parametrize("path", list(PATHS))
def test_decoys(path):
    """Raw sub-blocks that hold a self-consistent chain of Rice sub-blocks where a unit's guess searches.  The
    counters are printed, not asserted: whether a decoy is taken is the kernel's business, the result is not."""
    check(B.decoys(), path)


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 17])
def test_rows_batch_shapes(batch):
    """class_pairs and density at bs 16 / 32 in launches of 1, 3, 4, 5 and 17 streams: the rows of one wave mix
    streams the rows kernel takes with streams it hands to the fused kernel."""
    cases = [c for c in B.density() if c.cfg.bs in (16, 32)]
    pairs = [c for c in B.class_pairs() if c.cfg.bs in (16, 32)]
    check(cases + pairs, "auto", batch=batch)
