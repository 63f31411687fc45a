"""Times the incompressible categorizer's scan on the GPU and writes one JSON line per batch shape.

    python tools/incompressible_bench.py [--iters 5] [--options 0] [--search 0] [--out profiles/incompressible_scan.jsonl]

Data: the batch shapes of tools/zstd_encode_bench.py (sentence, skewed, below-4 and random bytes in pieces of 1 MiB,
and 1024 pieces of 64 KiB); every piece is an extent of its own, so the fragments kernel has one wave per piece.
Every device time is taken with device events around ONE call, buffers allocated beforehand, after two warm-up
calls: "scan_seconds" and "encode_seconds" list the `--iters` calls one by one (their spread is the point), for
``rpp_incompressible_scan_batch`` and for ``rpp_zstd_encode_batch_search`` with the same options and search word on
the same device buffer, in the same run; "scan_median" and "encode_median" are their medians and "gib_per_s" is
GiB/s of input at the scan's median.  "kernels_seconds" holds the mean device time per call of the scan's five
kernels (the search's two, entropy, classify, fragments) from a profiler trace of a further `--iters` calls (null
where the profiler reports no kernels).  "host_seconds" is ``rpp_incompressible_host_scan`` on the same pieces, one
call on ONE thread (the host scan is not threaded).  The sizes of the scan are checked against the encoder's.
No bar is set: that the scan costs less than the encoder (no emit, no output buffer) is an expectation these rows
record, first measurements that no test asserts.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dwarfs_amd import _native as N  # noqa: E402
from dwarfs_amd import categorize as CZ  # noqa: E402
from dwarfs_amd import section as S  # noqa: E402
from dwarfs_amd import zstd as Z  # noqa: E402
from dwarfs_amd.lz4 import _layout  # noqa: E402

GIB = float(1 << 30)
MIB = 1 << 20
KERNELS = ("rpp_lz4_prep_kernel", "rpp_lz4_search_kernel", "rpp_zstd_enc_entropy_kernel",
           "rpp_incompressible_classify_kernel", "rpp_incompressible_fragments_kernel")


def main():
    import numpy as np
    import torch

    import zstd_enc_cases as EC

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--options", type=int, default=0)
    ap.add_argument("--search", type=lambda v: int(v, 0), default=0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "incompressible_scan.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "incompressible_bench needs a GPU"
    dev = "cuda"
    K = EC.K
    shapes = (
        ("sentence_1MiB_x64", K.input_bytes({"kind": "sentence", "length": MIB}), 64),
        ("skewed_1MiB_x64", EC.skewed(7000, MIB), 64),
        ("below4_1MiB_x64", K.rnd(7001, MIB, 4), 64),
        ("random_1MiB_x16", K.rnd(7002, MIB), 16),
        ("skewed_64KiB_x1024", EC.skewed(7003, 65536), 1024),
    )
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    cfg = CZ.IncompressibleConfig(block_size=MIB, generate_fragments=True, options=args.options, search=args.search)
    rows = []
    for shape, piece, n in shapes:
        total = len(piece) * n
        offs, szs, base = CZ.cut([len(piece)] * n, cfg.block_size)
        flat = np.frombuffer(piece * n + bytes(16), np.uint8)
        d_in = torch.from_numpy(flat.copy()).to(dev)
        d_off, d_sz = S._i64(offs.astype(np.int64), dev), S._i64(szs.astype(np.int64), dev)
        d_base = torch.from_numpy(base.view(np.int32).copy()).to(dev)
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

        # the scan: five result arrays and the workspace, no output buffer
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        verdicts = torch.zeros(n, dtype=torch.int32, device=dev)
        totals = torch.zeros((n, CZ.TOTALS), dtype=torch.int64, device=dev)
        frag_rows = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        frag_count = torch.zeros(n, dtype=torch.int32, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        ws_bytes = int(N.lib().rpp_incompressible_workspace_bytes(total, n, n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def scan():
            st = N.lib().rpp_incompressible_scan_batch(p(d_in), p(d_off), p(d_sz), n, p(d_base), n, cfg.max_ratio, 1,
                                                       cfg.options, cfg.search, p(sizes), p(verdicts), p(totals),
                                                       p(frag_rows), p(frag_count), p(status), total, p(ws), ws_bytes,
                                                       stream())
            assert st == N.RPP_OK, st

        # the encoder on the same buffer
        out_offs, cap = _layout([Z.bound(int(s)) for s in szs])
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        d_ooff = S._i64(out_offs, dev)
        enc_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        enc_flags = torch.zeros(n, dtype=torch.int32, device=dev)
        enc_status = torch.zeros(n, dtype=torch.int32, device=dev)
        enc_ws_bytes = int(N.lib().rpp_zstd_encode_workspace_bytes(total, n))
        enc_ws = torch.empty(enc_ws_bytes, dtype=torch.uint8, device=dev)

        def encode():
            st = N.lib().rpp_zstd_encode_batch_search(p(d_in), p(d_off), p(d_sz), n, cfg.options, cfg.search, p(out),
                                                      p(d_ooff), p(enc_sizes), p(enc_flags), p(enc_status), total,
                                                      p(enc_ws), enc_ws_bytes, stream())
            assert st == N.RPP_OK, st

        def timed(call):
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            out_s = []
            for _ in range(args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                torch.cuda.synchronize()
                out_s.append(a.elapsed_time(b) / 1e3)
            return out_s

        t_scan, t_enc = timed(scan), timed(encode)
        assert int(status.abs().sum().item()) == 0 and int(enc_status.abs().sum().item()) == 0
        assert torch.equal(sizes, enc_sizes), "the scan's sizes are not the encoder's"
        kernels = None
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(args.iters):
                    scan()
                torch.cuda.synchronize()
            found = {}
            for e in prof.key_averages():
                for k in KERNELS:
                    if k in e.key.replace("rpp_lz4_deep_search_kernel", "rpp_lz4_search_kernel"):
                        us = getattr(e, "device_time_total", None)
                        if us is None:
                            us = e.cuda_time_total
                        found[k] = us / 1e6 / args.iters
            kernels = found if len(found) == len(KERNELS) else None
        except Exception as e:  # the trace is an extra: the row stands without it
            print(f"no kernel trace: {e}", file=sys.stderr)
        host_seconds = None
        if not args.no_host:
            t0 = time.perf_counter()
            host = CZ.host_scan(flat, offs, szs, base, cfg)
            host_seconds = time.perf_counter() - t0
            assert host[0].tolist() == sizes.cpu().numpy().tolist(), "the host scan's sizes are not the kernels'"
        med = statistics.median(t_scan)
        rows.append({"what": "incompressible_scan", "device": torch.cuda.get_device_name(0), "shape": shape,
                     "options": cfg.options, "search": cfg.search, "pieces": n, "extents": n, "input_bytes": total,
                     "frame_bytes": int(sizes.sum().item()), "incompressible_pieces": int(verdicts.sum().item()),
                     "workspace_bytes": ws_bytes, "encode_output_bytes": int(cap), "iters": args.iters,
                     "scan_seconds": t_scan, "encode_seconds": t_enc, "scan_median": med,
                     "encode_median": statistics.median(t_enc), "gib_per_s": total / GIB / med,
                     "kernels_seconds": kernels, "host_seconds": host_seconds, "host_threads": 1,
                     "first_measurement": True})
        print(json.dumps(rows[-1]), flush=True)
        del d_in, out, ws, enc_ws
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
