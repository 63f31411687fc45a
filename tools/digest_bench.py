"""Throughput of the named digests on the GPU (first measurements; no pass bar).

    python tools/digest_bench.py [--out profiles/digest.jsonl] [--reps N] [--host-mib M]

Times `digest.digest_batch` with device events (a warm-up call, then `reps` >= 10 timed calls; median, minimum and
maximum kept) for each of the thirteen algorithms on three shapes of random bytes, files on 16-byte boundaries:
  files_64k    4096 files x 64 KiB
  files_16m    64 files x 16 MiB
  files_256b   2^16 files x 256 bytes
and, in the same run on the same buffers, the yardsticks:
  sha512-256   the existing kernel (dedup.file_hash_batch)
  hashlib      the same algorithm on one host thread, over the first `host-mib` MiB of the same files (whole files)
One JSON line per measurement.  sha384, sha512 and sha512-224 share their rounds with the sha512-256 kernel; their
rows carry `of_sha512_256` (median time over the yardstick's median) to check that they lie within its spread.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dwarfs_amd import dedup as D  # noqa: E402
from dwarfs_amd import digest as G  # noqa: E402

HASHLIB = {"md5": "md5", "sha1": "sha1", "sha224": "sha224", "sha256": "sha256", "sha384": "sha384",
           "sha512": "sha512", "sha512-224": "sha512_224", "sha3-224": "sha3_224", "sha3-256": "sha3_256",
           "sha3-384": "sha3_384", "sha3-512": "sha3_512", "blake2b512": "blake2b", "blake2s256": "blake2s"}
SHAPES = (("files_64k", 4096, 64 << 10), ("files_16m", 64, 16 << 20), ("files_256b", 1 << 16, 256))


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


def record(records, workload, what, device, ms, nbytes, **extra):
    med = statistics.median(ms)
    r = {"workload": workload, "what": what, "device": device, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
         "ms_max": round(max(ms), 4), "reps": len(ms), "bytes": int(nbytes),
         "GiB_per_s": round(nbytes / 2**30 / (med / 1e3), 4), **extra}
    records.append(r)
    print(json.dumps(r), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "digest.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-mib", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "digest_bench needs a GPU"
    reps = max(10, args.reps)
    dev = torch.device("cuda:0")
    records = []
    for workload, nfiles, size in SHAPES:
        total = nfiles * size
        data = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
        offs = torch.arange(nfiles, dtype=torch.int64, device=dev) * size
        sizes = torch.full((nfiles,), size, dtype=torch.int64, device=dev)
        shape = {"files": nfiles, "file_bytes": size}
        out = torch.empty((nfiles, 32), dtype=torch.uint8, device=dev)
        base = record(records, workload, "sha512-256 (file_hash_batch)", "gpu", event_time_ms(
            lambda: D.file_hash_batch(data, offs, sizes, "sha512-256", out=out), 1, reps), total, **shape)
        base_spread = (records[-1]["ms_min"] / base, records[-1]["ms_max"] / base)
        host_files = max(1, min(nfiles, (args.host_mib << 20) // size))
        host = data[:host_files * size].cpu().numpy()
        for algo in HASHLIB:
            out = torch.empty((nfiles, G.digest_bytes(algo)), dtype=torch.uint8, device=dev)
            extra = dict(shape)
            med = statistics.median(ms := event_time_ms(
                lambda: G.digest_batch(data, offs, sizes, algo, out=out), 1, reps))
            if algo in ("sha384", "sha512", "sha512-224"):
                extra["of_sha512_256"] = round(med / base, 3)
                extra["sha512_256_spread"] = [round(v, 3) for v in base_spread]
            record(records, workload, algo, "gpu", ms, total, **extra)
            t0 = time.perf_counter()
            want = [hashlib.new(HASHLIB[algo], host[f * size:(f + 1) * size]).digest() for f in range(host_files)]
            dt = (time.perf_counter() - t0) * 1e3
            record(records, workload, f"hashlib {algo}", "cpu, 1 thread", [dt], host_files * size, files=host_files,
                   file_bytes=size)
            got = out[:host_files].cpu().numpy()
            assert [bytes(r) for r in got] == want, (workload, algo)
        del data, out
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
