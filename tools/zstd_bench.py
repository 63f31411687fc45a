"""Times the Zstandard block decoder on the GPU and writes one JSON line per batch shape.

    python tools/zstd_bench.py [--iters 5] [--out profiles/zstd_block.jsonl]

Data: there is no encoder here and libzstd may be absent, so a batch is made by replicating frames recorded in
tests/golden/zstd_kat.json (each a few hundred KB at most: NOT the 16 MiB blocks mkdwarfs writes, whose frames
hold 128 blocks each and would give the entropy kernel more to do at once per frame and the execute kernel a
longer serial chain).  Every device time is taken with device events around `--iters` calls of
rpp_zstd_decode_batch after two warm-up calls, buffers allocated beforehand, as tools/lz4_bench.py does;
"gib_per_s" is GiB/s of output.  "kernels" holds the mean device time of each of the three kernels per call,
taken from a profiler trace of a further `--iters` calls (null where the profiler reports no kernels).  "copy"
is a device-to-device copy of the output bytes (the yardstick: read n, write n).  No speed bar is set: these
rows are the baseline a tuning change starts from.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dwarfs_amd import _native as N  # noqa: E402
from dwarfs_amd import section as S  # noqa: E402
from dwarfs_amd import zstd as Z  # noqa: E402
from dwarfs_amd.lz4 import _layout, _upload  # noqa: E402

GIB = float(1 << 30)
KERNELS = ("rpp_zstd_index_kernel", "rpp_zstd_entropy_kernel", "rpp_zstd_execute_kernel")
# (name, the frames replicated, copies)
SHAPES = (
    ("below4_300000_l3", ("below4_300000/l3",), 64),
    ("below4_300000_l19", ("below4_300000/l19",), 64),
    ("prefixes_8000_l19", ("prefixes_8000/l19",), 128),
    ("sentence_300000_l3", ("sentence_300000/l3",), 128),
    ("sandwich_raw_blocks", ("sandwich/l3",), 32),
    ("below64_20000_l3", ("below64_20000/l3",), 1024),
    ("every_fixture_frame", None, 8),
)


def main():
    import torch

    import zstd_cases as ZC

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "zstd_block.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "zstd_bench needs a GPU"
    dev = "cuda"
    by_name = {name: (frame, data) for name, frame, data in ZC.frames()}
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    rows = []
    for shape, picks, copies in SHAPES:
        chosen = [by_name[k] for k in (picks or sorted(by_name))] * copies
        frames, datas = [f for f, _ in chosen], [d for _, d in chosen]
        sizes = [len(d) for d in datas]
        total, blocks = sum(sizes), sum(Z.count_blocks(f) for f in frames)
        d_in, in_offs = _upload(frames, dev)
        out_offs, cap = _layout(sizes)
        out = torch.zeros(max(cap, 16), dtype=torch.uint8, device=dev)
        status = torch.zeros(len(frames), dtype=torch.int32, device=dev)
        ws_bytes = int(N.lib().rpp_zstd_decode_workspace_bytes(total, blocks))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        arrays = [S._i64(in_offs, dev), S._i64([len(f) for f in frames], dev), S._i64(out_offs, dev), S._i64(sizes, dev)]

        def call():
            st = N.lib().rpp_zstd_decode_batch(p(d_in), p(arrays[0]), p(arrays[1]), len(frames), p(out), p(arrays[2]),
                                               p(arrays[3]), p(status), blocks, p(ws), ws_bytes,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert st == N.RPP_OK, st

        def timed(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / 1e3 / args.iters

        t = timed(call)
        assert int(status.abs().sum().item()) == 0, "a frame did not decode"
        host = out.cpu().numpy()
        for o, d in list(zip(out_offs, datas))[:len(picks or by_name)]:
            assert host[o:o + len(d)].tobytes() == d, "the decoder does not return the recorded input"
        kernels = None
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(args.iters):
                    call()
                torch.cuda.synchronize()
            found = {}
            for e in prof.key_averages():
                for k in KERNELS:
                    if k in e.key:
                        us = getattr(e, "device_time_total", None)
                        if us is None:
                            us = e.cuda_time_total
                        found[k] = us / 1e6 / args.iters
            kernels = found if len(found) == len(KERNELS) else None
        except Exception as e:  # the trace is an extra: the row stands without it
            print(f"no kernel trace: {e}", file=sys.stderr)
        src = torch.empty_like(out)
        t_copy = timed(lambda: src.copy_(out))
        rows.append({"what": "decode", "device": torch.cuda.get_device_name(0), "shape": shape, "frames": len(frames),
                     "blocks": blocks, "compressed_bytes": sum(map(len, frames)), "output_bytes": total,
                     "workspace_bytes": ws_bytes, "iters": args.iters, "seconds": t, "gib_per_s": total / GIB / t,
                     "kernels_seconds": kernels, "copy_seconds": t_copy, "copy_gib_per_s": total / GIB / t_copy})
        print(json.dumps(rows[-1]), flush=True)
        del d_in, out, ws, src
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
