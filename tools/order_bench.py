"""Time of the nilsimsa fragment ordering on the GPU next to the host restatement (first measurements; no pass bar).

    python tools/order_bench.py [--out profiles/order_nilsimsa.jsonl] [--skip-large]

Input: the family mix of the tests at size -- a random base digest, every member with f bit positions (drawn with
replacement) flipped, f from (0, 1, 2, 3, 8, 20, 60), families of 1 .. 400 members, shuffled; sizes from a few
values, a shuffled rank.  Rows: n = 20000 with options (256, 256), and n = 1,000,000 with the defaults (16384,
16384).  One JSON line per row: n, options, the family mix, wall-clock seconds of the GPU path per stage (split
launches, leaf chains, tree chains -- each bracketed by device synchronisation -- and the host plumbing around
them), the seconds of rpp_order_host_nilsimsa on one thread of the same machine, and the total distance before and
after.  The two orders are compared and must be equal.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dwarfs_amd import ordering as O  # noqa: E402

FLIPS = (0, 1, 2, 3, 8, 20, 60)
MEMBERS = (1, 2, 3, 5, 8, 12, 40, 100, 400)


def families(seed: int, n: int):
    rng = np.random.default_rng(seed)
    rows, total, mix = [], 0, {f: 0 for f in FLIPS}
    while total < n:
        m = min(int(rng.choice(MEMBERS)), n - total)
        f = int(rng.choice(FLIPS))
        member = np.repeat(rng.integers(0, 2, 256, dtype=np.uint8)[None, :], m, axis=0)
        where = rng.integers(0, 256, (m, f))
        for j in range(f):
            member[np.arange(m), where[:, j]] ^= 1
        rows.append(member)
        mix[f] += m
        total += m
    bits = np.packbits(np.concatenate(rows), axis=1, bitorder="little").view("<u8").astype(np.uint64)
    bits = bits[rng.permutation(n)]
    sizes = rng.choice(np.array([1, 4096, 4096, 65536], np.uint64), n)
    return bits, sizes, rng.permutation(n).astype(np.uint32), {str(f): c for f, c in mix.items()}


def row(n: int, max_children: int, max_cluster_size: int, seed: int) -> dict:
    bits, sizes, rank, mix = families(seed, n)
    O.order_nilsimsa(bits[:2000], sizes[:2000], rank=None, max_children=16, max_cluster_size=16)  # warm-up
    tm = {}
    got = O.order_nilsimsa(bits, sizes, rank, None, max_children, max_cluster_size, timings=tm)
    t0 = time.perf_counter()
    want, st = O.host_order_nilsimsa(bits, sizes, rank, None, max_children, max_cluster_size, return_stats=True)
    host_s = time.perf_counter() - t0
    assert np.array_equal(got, want), "the GPU order differs from the host restatement"
    return {"n": n, "max_children": max_children, "max_cluster_size": max_cluster_size,
            "family_members_by_flips": mix, "family_sizes": list(MEMBERS),
            "gpu_s": {k: round(v, 6) for k, v in tm.items() if k != "levels"}, "split_levels": tm["levels"],
            "host_one_thread_s": round(host_s, 6), "host_stats": st,
            "total_distance_before": O.total_distance(bits, np.arange(n)), "total_distance_after": O.total_distance(bits, got),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "order_nilsimsa.jsonl"))
    ap.add_argument("--skip-large", action="store_true", help="leave out the n = 1,000,000 row")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "order_bench needs a GPU"
    records = []
    for n, mc, mcs in [(20000, 256, 256)] + ([] if args.skip_large else [(1000000, 16384, 16384)]):
        records.append(row(n, mc, mcs, seed=n))
        print(json.dumps(records[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
