"""Throughput of the file hashes and of duplicate-file detection on the GPU (first measurements; no pass bar).

    python tools/dedup_bench.py [--out profiles/file_hash.jsonl] [--reps N]

Times with device events (warm-up first, then `reps` timed calls; median, minimum and maximum kept):
  files_64k    4096 x 64 KiB files, XXH3-128 and XXH3-64 (rpp_file_hash_batch)
  files_16m    256 x 16 MiB files, the same two
  lone_16m     one 16 MiB file, the same two: one wave's speed
  dedup_64k    rpp_file_dedup_batch over 4096 same-size 64 KiB files of which 10 % repeat an earlier file
  group_1m     rpp_group_first_batch alone over 2^20 keys (size + 16-byte digest, 10 % repeats)
The XXH3-64 rows of a run are the yardstick for its XXH3-128 rows: both run the same long-message loop.
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dwarfs_amd import dedup as D  # noqa: E402


def event_time_ms(fn, warmup: int, reps: int) -> list:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def record(records, workload, what, ms, nbytes=None, **extra):
    med = statistics.median(ms)
    r = {"workload": workload, "what": what, "device": "gpu", "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
         "ms_max": round(max(ms), 4), "reps": len(ms), **extra}
    if nbytes is not None:
        r["bytes"] = int(nbytes)
        r["GiB_per_s"] = round(nbytes / 2**30 / (med / 1e3), 3)
        r["GiB_per_s_min"] = round(nbytes / 2**30 / (max(ms) / 1e3), 3)
        r["GiB_per_s_max"] = round(nbytes / 2**30 / (min(ms) / 1e3), 3)
    records.append(r)
    print(json.dumps(r), flush=True)


def hash_rows(records, workload, buf, nfiles, size, reps):
    dev = buf.device
    d_off = torch.arange(nfiles, dtype=torch.int64, device=dev) * size
    d_sz = torch.full((nfiles,), size, dtype=torch.int64, device=dev)
    for algo in ("xxh3-128", "xxh3-64"):
        out = torch.empty((nfiles, 16 if algo == "xxh3-128" else 8), dtype=torch.uint8, device=dev)
        ms = event_time_ms(lambda: D.file_hash_batch(buf, d_off, d_sz, algo, out=out), 2, reps)
        record(records, workload, algo, ms, nfiles * size, files=nfiles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "file_hash.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dedup_bench needs a GPU"
    dev = torch.device("cuda:0")
    records = []

    buf = torch.randint(0, 256, (256 * (16 << 20),), dtype=torch.uint8, device=dev)  # 4 GiB
    hash_rows(records, "files_64k", buf, 4096, 64 << 10, args.reps)
    hash_rows(records, "files_16m", buf, 256, 16 << 20, max(3, args.reps // 4))
    hash_rows(records, "lone_16m", buf, 1, 16 << 20, max(3, args.reps // 4))

    # 4096 same-size files, every tenth one a copy of an earlier file
    n, size = 4096, 64 << 10
    rng = np.random.default_rng(7)
    src = np.arange(n)
    dup = np.arange(9, n, 10)
    src[dup] = (dup * rng.random(len(dup))).astype(np.int64) // 10 * 10  # (an original: index = 0 mod 10)
    d_off = torch.as_tensor(src * size, device=dev)
    d_sz = torch.full((n,), size, dtype=torch.int64, device=dev)
    out = D.find_duplicates_device(buf, d_off, d_sz)
    torch.cuda.synchronize()
    got = out.cpu()
    assert got.hashed.all() and (got.first != np.arange(n)).sum() == len(dup), "dedup_64k: wrong decision"
    ms = event_time_ms(lambda: D.find_duplicates_device(buf, d_off, d_sz, out=out), 2, args.reps)
    record(records, "dedup_64k", "rpp_file_dedup_batch xxh3-128", ms, n * size, files=n, duplicates=len(dup))

    # grouping alone
    n = 1 << 20
    which = np.arange(n)
    which[9::10] = rng.integers(0, n, len(which[9::10])) // 10 * 10
    digests = torch.as_tensor(rng.integers(0, 256, (n, 16), dtype=np.uint8)[which], device=dev)
    sizes = torch.full((n,), 64 << 10, dtype=torch.int64, device=dev)
    first, multi = D.group_first(sizes, digests)
    torch.cuda.synchronize()
    assert int((first.cpu().numpy() != np.arange(n)).sum()) > 0
    ms = event_time_ms(lambda: D.group_first(sizes, digests), 2, args.reps)
    record(records, "group_1m", "rpp_group_first_batch size+16", ms, keys=n,
           Mkeys_per_s=round(n / 1e6 / (statistics.median(ms) / 1e3), 1))

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
