"""Times the segmenter's match search on the GPU and writes one JSON line per measurement.

    python tools/segment_bench.py [--extent-mib 256] [--index-mib 64] [--iters 5] [--out profiles/segment_scan.jsonl]

Configuration: window_bits 12, increment_shift 1, granularity 1, 16 filter bits per index entry.  The indexed data
is `--index-mib` of random bytes in 16 MiB blocks; the extent is `--extent-mib` of random bytes with a tenth of it
copied verbatim from the blocks at odd offsets.  Every device time is taken with device events around `--iters`
calls after two warm-up calls, buffers allocated beforehand:

  hash    rpp_segment_hash_batch (every window hash of the extent, stored)
  scan    rpp_segment_scan_batch against the global filter (count pass, scan, emit pass)
  index   rpp_segment_index_batch over the blocks
  copy    a device-to-device copy of the extent (the yardstick: read n, write n)
  host    rpp_segment_host_scan on 16 threads, the extent cut into 16 pieces that overlap by a window

Rates are GiB/s of extent (index: block) bytes.  `algorithmic_bytes` of the scan is read n, write 8 * hits.
"""
import argparse
import ctypes as C
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dwarfs_amd import _native as N  # noqa: E402
from dwarfs_amd import segmenter as S  # noqa: E402
from dwarfs_amd.section import _ptr  # noqa: E402

GIB = float(1 << 30)


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extent-mib", type=int, default=256)
    ap.add_argument("--index-mib", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_scan.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "segment_bench needs a GPU"
    dev = "cuda"
    n, nb = args.extent_mib << 20, args.index_mib << 20
    block_bytes = min(16 << 20, nb)
    nblocks = nb // block_bytes
    slots_total = nblocks * ((block_bytes - 4096) // 2048 + 1)
    filter_bits = 1 << int(np.ceil(np.log2(max(16 * slots_total, 64))))
    cfg = S.SegmenterConfig(12, 1, 1, filter_bits)
    c = cfg.native()
    rng = np.random.default_rng(2024)
    blocks = rng.integers(0, 256, nb, dtype=np.uint8)
    extent = rng.integers(0, 256, n, dtype=np.uint8)
    piece = 1 << 20
    for k in range(max(1, n // (10 * piece))):  # a tenth of the extent comes from the blocks
        src = int(rng.integers(0, nb - piece)) | 1
        dst = (k * 10 * piece + 12345) | 1
        if dst + piece <= n:
            extent[dst:dst + piece] = blocks[src:src + piece]
    d_blocks, d_ext = torch.from_numpy(blocks).to(dev), torch.from_numpy(extent).to(dev)
    L = N.lib()
    rows = []
    base = {"device": torch.cuda.get_device_name(0), "window_bits": 12, "increment_shift": 1, "granularity": 1,
            "filter_bits": filter_bits, "extent_bytes": n, "indexed_bytes": nb, "iters": args.iters}

    # index
    b_off = torch.arange(nblocks, dtype=torch.int64, device=dev) * block_bytes
    b_sz = torch.full((nblocks,), block_bytes, dtype=torch.int64, device=dev)
    idx = S.BlockIndex.build(d_blocks, b_off, b_sz, cfg)
    ws_i = torch.empty(L.rpp_segment_index_workspace_bytes(nblocks), dtype=torch.uint8, device=dev)
    start_i = torch.empty(nblocks + 1, dtype=torch.int64, device=dev)
    st_i = torch.zeros(1, dtype=torch.int32, device=dev)
    gf = torch.zeros_like(idx.global_filter)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run_index():
        L.rpp_segment_index_batch(C.byref(c), _ptr(d_blocks), _ptr(b_off), _ptr(b_sz), nblocks, block_bytes,
                                  _ptr(idx.hash), _ptr(idx.offset), _ptr(idx.entered), idx.hash.numel(), _ptr(start_i),
                                  _ptr(idx.block_filters), _ptr(gf), _ptr(st_i), _ptr(ws_i), ws_i.numel(), stream)

    t = timed(run_index, args.iters)
    assert int(st_i.item()) == 0 and torch.equal(gf, idx.global_filter)
    rows.append(dict(base, what="index", seconds=t, gib_per_s=nb / GIB / t, slots=int(idx.hash.numel()),
                     entered=int(idx.entered.sum().item())))

    # scan
    d_off = torch.zeros(1, dtype=torch.int64, device=dev)
    d_sz = torch.full((1,), n, dtype=torch.int64, device=dev)
    # (the sum half of the hash is far from uniform on random bytes, so the filter passes more than the 1 in 16 its
    # size suggests: room for every second position)
    out = S.DeviceHits.new(1, n, max(1 << 20, n // 2), dev)
    t = timed(lambda: S.scan_into(out, d_ext, d_off, d_sz, idx.global_filter, cfg), args.iters)
    hits, status = out.count(), out.status()
    assert status == 0, status
    rows.append(dict(base, what="scan", seconds=t, gib_per_s=n / GIB / t, hits=hits, hit_rate=hits / (n - 4095),
                     algorithmic_bytes=n + 8 * hits, algorithmic_gib_per_s=(n + 8 * hits) / GIB / t))

    # hash only
    npos = n - 4095
    hashes = torch.empty(npos, dtype=torch.int32, device=dev)
    ws_h = torch.empty(L.rpp_segment_hash_workspace_bytes(1, n), dtype=torch.uint8, device=dev)
    start_h = torch.empty(2, dtype=torch.int64, device=dev)
    st_h = torch.zeros(1, dtype=torch.int32, device=dev)

    def run_hash():
        L.rpp_segment_hash_batch(C.byref(c), _ptr(d_ext), _ptr(d_off), _ptr(d_sz), 1, n, _ptr(hashes), npos,
                                 _ptr(start_h), _ptr(st_h), _ptr(ws_h), ws_h.numel(), stream)

    t = timed(run_hash, args.iters)
    assert int(st_h.item()) == 0
    rows.append(dict(base, what="hash", seconds=t, gib_per_s=n / GIB / t, algorithmic_bytes=n + 4 * npos,
                     algorithmic_gib_per_s=(n + 4 * npos) / GIB / t))
    del hashes

    # the yardstick: a device copy of the extent
    dst = torch.empty_like(d_ext)
    t = timed(lambda: dst.copy_(d_ext), args.iters)
    rows.append(dict(base, what="copy", seconds=t, gib_per_s=n / GIB / t, algorithmic_bytes=2 * n,
                     algorithmic_gib_per_s=2 * n / GIB / t))
    copy_rate = n / GIB / t
    for r in rows:
        if r["what"] in ("hash", "scan"):
            r["ratio_to_copy"] = r["gib_per_s"] / copy_rate

    # the host restatement on 16 threads; the pieces' hits together equal the device's
    filt = idx.global_filter.cpu().numpy().view(np.uint64)
    threads = 16
    cut = [(i * (n // threads), min(n, (i + 1) * (n // threads) + 4095) if i < threads - 1 else n) for i in range(threads)]
    ext_bytes = extent.tobytes()

    def piece_scan(lohi):
        return S.host_scan(ext_bytes[lohi[0]:lohi[1]], filt, cfg)[2]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        host_hits = sum(ex.map(piece_scan, cut))
    t = time.perf_counter() - t0
    assert host_hits == hits, (host_hits, hits)
    rows.append(dict(base, what="host_scan_16_threads", seconds=t, gib_per_s=n / GIB / t, hits=host_hits))

    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
