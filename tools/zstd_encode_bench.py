"""Times the Zstandard block encoder on the GPU and writes one JSON line per batch shape.

    python tools/zstd_encode_bench.py [--iters 5] [--options 0 3] [--out profiles/zstd_encode.jsonl]

Data: blocks of 1 MiB made by the generators of tests/golden/make_lz4_kat.py and tests/zstd_enc_cases.py (NOT the
16 MiB blocks mkdwarfs writes), and every test input once.  Every device time is taken with device events around
`--iters` calls after two warm-up calls, buffers allocated beforehand, as tools/zstd_bench.py does; "gib_per_s" is
GiB/s of input.  "kernels_seconds" holds the mean device time per call of the five kernels (the search's two, then
entropy, place, emit), taken from a profiler trace of a further `--iters` calls (null where the profiler reports
no kernels).  "lz4_seconds" is rpp_lz4_encode_batch on the same inputs, in the same run; "frame_bytes" and
"lz4_bytes" are what the two write.  No speed bar is set: nobody has measured this encoder before, and these
rows are first measurements, the baseline a tuning change starts from.  `--options` lists the encoder's options
words (rpp_zstd_encode_batch_opt: 1 per-block table modes, 2 repeat offsets, 3 both); every batch is encoded with
each of them, one row per batch and options word ("options"), and the rows are appended to the file.
`--search WORD...` lists search words (rpp_zstd_encode_batch_search and rpp_lz4_encode_batch_search: depth 1, 2, 4
or 8, plus 0x100 for LAZY; 0, the default, is the one-candidate search): one row per batch, options word and search
word ("search"), with the LZ4 figures of the same word; "kernels_seconds" then lists the deep search kernel under
"rpp_lz4_search_kernel".
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
from dwarfs_amd import lz4  # noqa: E402
from dwarfs_amd import zstd as Z  # noqa: E402
from dwarfs_amd.lz4 import _layout, _upload  # noqa: E402

GIB = float(1 << 30)
MIB = 1 << 20
KERNELS = ("rpp_lz4_prep_kernel", "rpp_lz4_search_kernel", "rpp_zstd_enc_entropy_kernel", "rpp_zstd_enc_place_kernel",
           "rpp_zstd_enc_emit_kernel")
# with --long 1 the long-distance matcher's kernels (csrc/zstd_long.hip) are listed as well
LONG_KERNELS = ("rpp_zstd_long_prepare_kernel", "rpp_zstd_long_index_kernel", "rpp_zstd_long_find_kernel",
                "rpp_zstd_long_merge_kernel")


def main():
    import torch

    import zstd_enc_cases as EC

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--options", type=int, nargs="+", default=[0])
    ap.add_argument("--search", type=lambda v: int(v, 0), nargs="+", default=[0])
    ap.add_argument("--long", type=int, nargs="+", default=[0], help="the long word: 0, 1 or both; 1 adds a row per "
                    "shape with \"long\": 1 and one batch of 16 MiB blocks, the workload's own block size")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "zstd_encode.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "zstd_encode_bench needs a GPU"
    dev = "cuda"
    K = EC.K
    shapes = (
        ("sentence_1MiB_x64", [K.input_bytes({"kind": "sentence", "length": MIB})] * 64),
        ("skewed_1MiB_x64", [EC.skewed(7000, MIB)] * 64),
        ("below4_1MiB_x64", [K.rnd(7001, MIB, 4)] * 64),
        ("random_1MiB_x16", [K.rnd(7002, MIB)] * 16),
        ("skewed_64KiB_x1024", [EC.skewed(7003, 65536)] * 1024),
        ("every_test_input", [d for _, d in EC.inputs()]),
    )
    if 1 in args.long:  # half of every block repeats its other half, 8 MiB back
        shapes += (("half_repeat_16MiB_x4", [EC.skewed(7004 + i, 8 * MIB) * 2 for i in range(4)]),)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for shape, blocks in shapes:
        sizes = [len(b) for b in blocks]
        total, n = sum(sizes), len(blocks)
        d_in, in_offs = _upload(blocks, dev)
        arrays = [S._i64(in_offs, dev), S._i64(sizes, dev)]
        results = {}
        codecs = [(("zstd", o, w, g), Z.bound,
                   lambda total, n, g=g: N.lib().rpp_zstd_encode_workspace_bytes_long(total, n, g),
                   lambda *a, o=o, w=w, g=g: N.lib().rpp_zstd_encode_batch_long(*a[:4], o, w, g, *a[4:]))
                  for o in args.options for w in args.search for g in args.long]
        codecs += [(("lz4", 0, w, 0), lz4.bound, N.lib().rpp_lz4_encode_workspace_bytes,
                    lambda *a, w=w: N.lib().rpp_lz4_encode_batch_search(*a[:4], w, *a[4:])) for w in args.search]
        for (codec, options, search, long), bound, ws_of, call_of in codecs:
            out_offs, cap = _layout([bound(s) for s in sizes])
            out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
            d_ooff = S._i64(out_offs, dev)
            out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
            flags = torch.zeros(n, dtype=torch.int32, device=dev)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            ws_bytes = int(ws_of(total, n))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

            def call():
                st = call_of(p(d_in), p(arrays[0]), p(arrays[1]), n, p(out), p(d_ooff), p(out_sizes), p(flags),
                             p(status), total, p(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert st == N.RPP_OK, st

            for _ in range(2):
                call()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                call()
            b.record()
            torch.cuda.synchronize()
            assert int(status.abs().sum().item()) == 0, "a block was not encoded"
            kernels = None
            if codec == "zstd":
                host, got = out.cpu().numpy(), out_sizes.cpu().numpy()
                for i in sorted({0, n - 1}):
                    frame = host[out_offs[i]:out_offs[i] + got[i]].tobytes()
                    assert Z.host_decode(frame, sizes[i]) == (N.RPP_OK, blocks[i]), "the frame does not decode"
                try:
                    from torch.profiler import ProfilerActivity, profile

                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        for _ in range(args.iters):
                            call()
                        torch.cuda.synchronize()
                    found, wanted = {}, KERNELS + (LONG_KERNELS if long else ())
                    for e in prof.key_averages():
                        for k in wanted:
                            if k in e.key.replace("rpp_lz4_deep_search_kernel", "rpp_lz4_search_kernel"):
                                us = getattr(e, "device_time_total", None)
                                if us is None:
                                    us = e.cuda_time_total
                                found[k] = us / 1e6 / args.iters
                    kernels = found if len(found) == len(wanted) else None
                except Exception as e:  # the trace is an extra: the row stands without it
                    print(f"no kernel trace: {e}", file=sys.stderr)
            results[codec, options, search, long] = (a.elapsed_time(b) / 1e3 / args.iters, int(out_sizes.sum().item()), ws_bytes, kernels)
            del out, ws
        for o, w, g in ((o, w, g) for o in args.options for w in args.search for g in args.long):
            t_lz4, lz4_bytes, _, _ = results["lz4", 0, w, 0]
            t, frame_bytes, ws_bytes, kernels = results["zstd", o, w, g]
            rows.append({"what": "encode", "device": torch.cuda.get_device_name(0), "shape": shape, "options": o,
                         "search": w, "long": g,
                         "blocks": n, "input_bytes": total, "frame_bytes": frame_bytes, "lz4_bytes": lz4_bytes,
                         "workspace_bytes": ws_bytes, "iters": args.iters, "seconds": t, "gib_per_s": total / GIB / t,
                         "kernels_seconds": kernels, "lz4_seconds": t_lz4, "lz4_gib_per_s": total / GIB / t_lz4,
                         "first_measurement": True})
            print(json.dumps(rows[-1]), flush=True)
        del d_in
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
