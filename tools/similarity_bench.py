"""Throughput of the similarity hashes on the GPU (first measurements; no pass bar).

    python tools/similarity_bench.py [--out profiles/similarity_hash.jsonl] [--reps N]

Times with device events (two warm-up calls, then `reps` timed calls; median, minimum and maximum kept), the method
of tools/dedup_bench.py and its three workloads:
  files_64k      4096 x 64 KiB files        (256 MiB: fits the 256 MiB last-level cache)
  files_16m      256 x 16 MiB files         (4 GiB: streams from HBM)
  lone_16m       one 16 MiB file            (fits the last-level cache)
  lone_16m_zero  one 16 MiB all-zero file   (every lane of a wave hits the same few bins)
Every workload runs rpp_similarity_hash_batch for both kinds and, as the yardstick, XXH3-128 (rpp_file_hash_batch)
on the same buffers in the same session; `ratio_to_xxh3_128` is the hash's rate over the yardstick's.
`update_only` rows time rpp_similarity_update_batch alone on states that are not reset (the counters just grow):
hash_batch without clearing and finalizing the states.  The host restatement on one thread is recorded for the
16 MiB file as a description.  One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dwarfs_amd import dedup as D  # noqa: E402
from dwarfs_amd import similarity as S  # noqa: E402

KINDS = ("nilsimsa", "similarity")


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


def record(records, workload, what, ms, nbytes, device="gpu", **extra):
    med = statistics.median(ms)
    r = {"workload": workload, "what": what, "device": device, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
         "ms_max": round(max(ms), 4), "reps": len(ms), "bytes": int(nbytes),
         "GiB_per_s": round(nbytes / 2**30 / (med / 1e3), 3),
         "GiB_per_s_min": round(nbytes / 2**30 / (max(ms) / 1e3), 3),
         "GiB_per_s_max": round(nbytes / 2**30 / (min(ms) / 1e3), 3), **extra}
    records.append(r)
    print(json.dumps(r), flush=True)
    return r


def rows(records, workload, buf, nfiles, size, reps):
    dev = buf.device
    d_off = torch.arange(nfiles, dtype=torch.int64, device=dev) * size
    d_sz = torch.full((nfiles,), size, dtype=torch.int64, device=dev)
    nbytes = nfiles * size
    out = torch.empty((nfiles, 16), dtype=torch.uint8, device=dev)
    ms = event_time_ms(lambda: D.file_hash_batch(buf, d_off, d_sz, "xxh3-128", out=out), 2, reps)
    yard = record(records, workload, "xxh3-128", ms, nbytes, files=nfiles)
    for kind in KINDS:
        bufs = S.DeviceSimilarity.new(nfiles, kind, dev)
        ms = event_time_ms(lambda: S.similarity_hash_batch(buf, d_off, d_sz, kind, out=bufs), 2, reps)
        r = record(records, workload, kind, ms, nbytes, files=nfiles)
        r["ratio_to_xxh3_128"] = round(r["GiB_per_s"] / yard["GiB_per_s"], 4)
        st = S.SimilarityState.new(nfiles, kind, dev)
        ms = event_time_ms(lambda: S.update(st, buf, d_off, d_sz), 2, reps)
        r = record(records, workload, kind + " update_only", ms, nbytes, files=nfiles)
        r["ratio_to_xxh3_128"] = round(r["GiB_per_s"] / yard["GiB_per_s"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "similarity_hash.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "similarity_bench needs a GPU"
    dev = torch.device("cuda:0")
    records = []
    few = max(3, args.reps // 4)

    buf = torch.randint(0, 256, (256 * (16 << 20),), dtype=torch.uint8, device=dev)  # 4 GiB
    rows(records, "files_64k", buf, 4096, 64 << 10, args.reps)
    rows(records, "files_16m", buf, 256, 16 << 20, few)
    rows(records, "lone_16m", buf, 1, 16 << 20, args.reps)
    lone = buf[:16 << 20].cpu().numpy().tobytes()
    del buf
    zero = torch.zeros(16 << 20, dtype=torch.uint8, device=dev)
    rows(records, "lone_16m_zero", zero, 1, 16 << 20, args.reps)

    # the host restatement on one thread (a description, not a bar); its digest equals the device's
    for kind in KINDS:
        ms = []
        for _ in range(3):
            t = time.perf_counter()
            digest = S.host_hash(lone, kind)
            ms.append((time.perf_counter() - t) * 1e3)
        got = S.similarity_hashes([lone], kind)
        assert got.digests[0].tobytes() == digest, f"lone_16m {kind}: the device digest differs from the host's"
        record(records, "lone_16m", kind + " host restatement, 1 thread", ms, len(lone), device="host", files=1)

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
