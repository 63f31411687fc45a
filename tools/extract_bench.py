"""Throughput of the file-extraction gather on the GPU (first measurements; no pass bar).

    python tools/extract_bench.py [--out profiles/extract_gather.jsonl] [--reps N]

Times with device events (warm-up first, then `reps` timed calls; median, minimum and maximum kept), three shapes:
  files_64k    4096 files x 64 KiB, one chunk each
  files_16m    64 files x 16 MiB, 16 chunks of 1 MiB each, a file's chunks in 16 different blocks
  chunks_64b   one file of 2^20 chunks x 64 bytes
and for each shape, in the same run:
  gather       rpp_extract_gather_batch alone (tables on the device, output allocated): GiB/s of output
  d2d_copy     a plain device-to-device copy of the same byte count: the yardstick
  file_checksums   gather + XXH3-128 as extract.file_checksums runs them (table upload and output memset included)
  file_hash_batch  XXH3-128 alone on an already contiguous copy of the same files
Source offsets inside the blocks are odd (the funnel-shift path), destinations are the default 16-byte layout.
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
from dwarfs_amd import extract as X  # noqa: E402

BLOCK = 16 << 20  # the decoded blocks: 16 MiB each, with 4 KiB to spare for the odd offsets
SPARE = 4096


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


def record(records, workload, what, ms, nbytes, **extra):
    med = statistics.median(ms)
    r = {"workload": workload, "what": what, "device": "gpu", "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
         "ms_max": round(max(ms), 4), "reps": len(ms), "bytes": int(nbytes),
         "GiB_per_s": round(nbytes / 2**30 / (med / 1e3), 3),
         "GiB_per_s_min": round(nbytes / 2**30 / (max(ms) / 1e3), 3),
         "GiB_per_s_max": round(nbytes / 2**30 / (min(ms) / 1e3), 3), **extra}
    records.append(r)
    print(json.dumps(r), flush=True)
    return med


def table_of(chunks: np.ndarray, first) -> X.FileTable:
    return X.FileTable(chunks, np.asarray(first, np.uint64))


def shapes(nblocks: int):
    rows = np.zeros(4096, X.CHUNK_DTYPE)  # 4096 x 64 KiB, one chunk each, spread over the blocks
    k = np.arange(4096)
    rows["block"], rows["offset"], rows["size"] = k % nblocks, (k // nblocks) * (64 << 10) + 1 + k % 13, 64 << 10
    yield "files_64k", table_of(rows, np.arange(4097))
    rows = np.zeros(64 * 16, X.CHUNK_DTYPE)  # 64 x 16 MiB, 16 chunks of 1 MiB in 16 different blocks
    f, c = np.divmod(np.arange(64 * 16), 16)
    rows["block"], rows["offset"], rows["size"] = (f + c) % nblocks, c * (1 << 20) + 3 + f % 7, 1 << 20
    yield "files_16m", table_of(rows, np.arange(65) * 16)
    rows = np.zeros(1 << 20, X.CHUNK_DTYPE)  # one file of 2^20 chunks x 64 bytes
    k = np.arange(1 << 20)
    rows["block"], rows["offset"], rows["size"] = (k * 7) % nblocks, ((k * 2654435761) % (BLOCK // 64)) * 64 + 5, 64
    yield "chunks_64b", table_of(rows, [0, 1 << 20])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "extract_gather.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "extract_bench needs a GPU"
    dev = torch.device("cuda:0")
    records = []
    nblocks = 16
    blocks = torch.randint(0, 256, (nblocks * (BLOCK + SPARE),), dtype=torch.uint8, device=dev)
    boff = np.arange(nblocks, dtype=np.int64) * (BLOCK + SPARE)
    bsz = np.full(nblocks, BLOCK + SPARE, np.int64)
    d_boff, d_bsz = torch.as_tensor(boff, device=dev), torch.as_tensor(bsz, device=dev)

    for name, table in shapes(nblocks):
        plan = X.plan_gather(table, dev)
        total = int(table.file_sizes.sum())
        out = torch.zeros(plan.out_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(plan.nfiles, dtype=torch.int32, device=dev)
        X.gather_into(blocks, d_boff, d_bsz, plan, out, status)
        torch.cuda.synchronize()
        assert int(status.abs().sum().item()) == 0, name
        # spot check: the first and the last chunk against slices of the blocks
        for c in (0, table.nchunks - 1):
            b, o, n = (int(v) for v in table.chunks[c])
            at = int(plan.d_chunk_dst[c].item())
            assert torch.equal(out[at:at + n], blocks[boff[b] + o:boff[b] + o + n]), (name, c)
        shape = {"files": table.nfiles, "chunks": table.nchunks}
        g = record(records, name, "gather", event_time_ms(
            lambda: X.gather_into(blocks, d_boff, d_bsz, plan, out, status), 2, args.reps), total, **shape)
        src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        c = record(records, name, "d2d_copy", event_time_ms(lambda: dst.copy_(src), 2, args.reps), total)
        records[-2]["of_d2d_copy"] = round(c / g, 3)
        for algo in ("xxh3-128",):
            reps = max(3, args.reps // 4)
            a = record(records, name, f"file_checksums {algo}", event_time_ms(
                lambda: X.file_checksums(blocks, d_boff, d_bsz, table, algo, max_bytes=1 << 31, device=dev), 1, reps),
                total, **shape)
            d_off = torch.as_tensor(plan.file_dst.astype(np.int64), device=dev)
            d_sz = torch.as_tensor(plan.file_sizes.astype(np.int64), device=dev)
            digests = torch.empty((table.nfiles, 16 if algo == "xxh3-128" else 32), dtype=torch.uint8, device=dev)
            h = record(records, name, f"file_hash_batch {algo}", event_time_ms(
                lambda: D.file_hash_batch(out, d_off, d_sz, algo, out=digests), 1, reps), total)
            records[-2]["over_hash_alone"] = round(a / h, 3)
            got, st = X.file_checksums(blocks, d_boff, d_bsz, table, algo, max_bytes=1 << 31, device=dev)
            assert torch.equal(got, digests) and int(st.abs().sum().item()) == 0, (name, algo)
        del out, src, dst, plan

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
