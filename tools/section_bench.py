"""Throughput of the section checksums on the GPU (first measurements; no pass bar).

    python tools/section_bench.py [--out profiles/section_hash.jsonl] [--reps N]

Times rpp_xxh3_64_batch and rpp_sha512_256_batch with device events (warm-up first, then `reps` timed
calls, the median kept) on three workloads:
  bench_blocks   4096 ricepp-encoded blocks of 32768 Poisson samples each (the flagship benchmark's shape),
                 hashed where the encoder left them (16-aligned capacity slots, device sizes)
  mix            16 x 1 MiB + 8 x 4 MiB + 4 x 16 MiB messages of random bytes
  lone_16m       one 16 MiB message: XXH3 at one wave's speed, SHA-512/256 at one lane's
and, as the CPU side, one thread of hashlib's sha512_256 and of the xxhash module (when it imports) over a
16 MiB buffer.  One JSON line per measurement.
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
from dwarfs_amd import codec  # noqa: E402
from dwarfs_amd import section as S  # noqa: E402


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


def measure(name, data, offs, sizes, total_bytes, nmsg, reps, records):
    d_off = torch.as_tensor(np.asarray(offs, np.int64), device=data.device) if not isinstance(offs, torch.Tensor) else offs
    d_sz = torch.as_tensor(np.asarray(sizes, np.int64), device=data.device) if not isinstance(sizes, torch.Tensor) else sizes
    for algo, fn, r in (("xxh3_64", S.xxh3_64_batch, reps), ("sha512_256", S.sha512_256_batch, max(2, reps // 4))):
        ms = event_time_ms(lambda: fn(data, d_off, d_sz), 2, r)
        med = statistics.median(ms)
        records.append({"workload": name, "algo": algo, "device": "gpu", "messages": nmsg, "bytes": int(total_bytes),
                        "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                        "reps": r, "GiB_per_s": round(total_bytes / 2**30 / (med / 1e3), 3)})
        print(json.dumps(records[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "section_hash.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "section_bench needs a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2024)
    records = []

    nblocks, n = 4096, 32768
    x = (rng.poisson(1000, nblocks * n).astype(np.uint16) << 2).byteswap()
    cfg = codec.CodecConfig(block_size=128, component_stream_count=1, byteorder="big", unused_lsb_count=2)
    enc = codec.encode_batch(cfg, torch.from_numpy(x.view(np.int16)).to(dev), [i * n for i in range(nblocks)],
                             [n] * nblocks)
    torch.cuda.synchronize()
    enc.check()
    total = int(enc.sizes.sum().item())
    measure("bench_blocks", enc.data, enc.d_offsets, enc.sizes, total, nblocks, args.reps, records)
    del enc, x

    sizes = [1 << 20] * 16 + [4 << 20] * 8 + [16 << 20] * 4
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    buf = torch.randint(0, 256, (sum(sizes),), dtype=torch.uint8, device=dev)
    measure("mix", buf, offs, sizes, sum(sizes), len(sizes), args.reps, records)
    measure("lone_16m", buf, [0], [16 << 20], 16 << 20, 1, args.reps, records)

    host = buf[:16 << 20].cpu().numpy().tobytes()
    cpu = [("sha512_256", lambda b: hashlib.new("sha512_256", b).digest())]
    try:
        import xxhash
        cpu.append(("xxh3_64", xxhash.xxh3_64_intdigest))
    except ImportError:
        pass
    for algo, fn in cpu:
        fn(host)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn(host)
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        records.append({"workload": "lone_16m", "algo": algo, "device": "cpu_1_thread", "messages": 1,
                        "bytes": len(host), "ms_median": round(med * 1e3, 4), "reps": 3,
                        "GiB_per_s": round(len(host) / 2**30 / med, 3)})
        print(json.dumps(records[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
