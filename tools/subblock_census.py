#!/usr/bin/env python3
"""Bit lengths of the Rice sub-blocks of Poisson data (CPU only).

Encodes numpy Poisson(lambda) blocks with the oracle (bs 128, cs 1, big endian: the bench's configuration), walks
every stream header by header and code by code, and prints one JSON line per lambda with the distribution of the
sub-block lengths (header included): mean, max, the share longer than ``--window - 7`` bits (a window of that size
holds the sub-block's last terminator and lets its remainder be read from the lane's own 32 bits), the fs mix and
the lengths of the runs of fitting sub-blocks between two long ones.

    python tools/subblock_census.py [--blocks 256] [--lam 1000 300 3000] [--window 1024]
"""

from __future__ import annotations

import argparse
import json
import sys
from bisect import bisect_left
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oracle import oracle  # noqa: E402


def walk(stream: bytes, n_samples: int, bs: int, cs: int = 1):
    """(fs + 1 header value, bit length) of every sub-block of one stream."""
    bits = np.unpackbits(np.frombuffer(stream, np.uint8), bitorder="little")
    ones = np.flatnonzero(bits).tolist()
    hdr = bits.astype(np.int64)
    out = []
    pos = 16 * cs
    left = n_samples
    while left > 0:
        for _ in range(cs):
            n = min(bs, left // cs if left < bs * cs else bs)
            h = int(hdr[pos] | hdr[pos + 1] << 1 | hdr[pos + 2] << 2 | hdr[pos + 3] << 3)
            p = pos + 4
            if h == 15:
                p += 16 * n
            elif h != 0:
                i = bisect_left(ones, p)
                for _ in range(n):
                    while ones[i] < p:
                        i += 1
                    p = ones[i] + h  # terminator + 1 + fs
            out.append((h, p - pos))
            pos = p
        left -= min(left, bs * cs)
    return out


def census(lam: float, blocks: int, n: int, window: int, seed: int):
    rng = np.random.default_rng(seed)
    cfg = oracle.cfg(128, 1, True, 0)
    lens, heads, gaps = [], [], []
    for _ in range(blocks):
        v = np.minimum(rng.poisson(lam, n), 65535).astype(np.uint16).byteswap()  # stored big endian
        sub = walk(oracle.encode(cfg, v), n, 128)
        heads += [h for h, _ in sub]
        lens += [b for _, b in sub]
        run = 0
        for _, b in sub:  # fitting sub-blocks between two long ones, per stream
            if b > window - 7:
                gaps.append(run)
                run = 0
            else:
                run += 1
    lens = np.asarray(lens)
    heads = np.asarray(heads)
    gaps = np.asarray(gaps) if gaps else np.zeros(0, np.int64)
    long_ = lens > window - 7
    return {
        "lambda": lam, "blocks": blocks, "sub_blocks": int(lens.size), "window": window,
        "mean_bits": round(float(lens.mean()), 2), "max_bits": int(lens.max()),
        "p50": int(np.percentile(lens, 50)), "p99": int(np.percentile(lens, 99)),
        "p999": int(np.percentile(lens, 99.9)),
        "share_long": float(long_.mean()), "n_long": int(long_.sum()),
        "fs_mix": {str(int(h) - 1): round(float((heads == h).mean()), 5) for h in np.unique(heads)},
        "share_long_by_fs": {str(int(h) - 1): float(long_[heads == h].mean()) for h in np.unique(heads)},
        "gap_lt4": int((gaps < 4).sum()), "gap_lt8": int((gaps < 8).sum()), "gap_lt16": int((gaps < 16).sum()),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--samples", type=int, default=32768, help="samples per block (64 KiB)")
    ap.add_argument("--lam", type=float, nargs="+", default=[1000.0])
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args()
    for lam in a.lam:
        print(json.dumps(census(lam, a.blocks, a.samples, a.window, a.seed)), flush=True)


if __name__ == "__main__":
    main()
