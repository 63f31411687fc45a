"""Times the LZ4 block codec on the GPU and writes one JSON line per measurement.

    python tools/lz4_bench.py [--iters 5] [--out profiles/lz4_block.jsonl] [--sizes-only]

Data: two generators, "sentence" (words drawn from a small vocabulary) and "low_entropy" (bytes below 4), as
256 blocks of 1 MiB and as 16 blocks of 16 MiB.  Every device time is taken with device events around `--iters`
calls after two warm-up calls, buffers allocated beforehand:

  encode  rpp_lz4_encode_batch (all four launches)
  decode  rpp_lz4_decode_batch of the blocks the encoder wrote (one wave per block)
  copy    a device-to-device copy of the same bytes (the yardstick: read n, write n)
  liblz4_compress_default / liblz4_decompress_safe   on 16 host threads, where liblz4.so.1 loads

Rates are GiB/s of uncompressed bytes.  No speed bar is set: these rows are the baseline a tuning change starts
from.  "sizes" rows need no GPU (`--sizes-only` writes only them): the compressed size of every fixture input and
of 1 MiB of both generators under the host restatement of the encoder (the kernels' bytes), LZ4_compress_default
and LZ4_compress_HC level 9.
"""
import argparse
import ctypes as C
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
from dwarfs_amd import lz4 as Z  # noqa: E402

GIB = float(1 << 30)
WORDS = ("block archive image header section the of and to in file data offset length index chunk inode "
         "directory entry metadata schema compress segment window hash match literal token stream").split()


def generate(kind: str, n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    if kind == "low_entropy":
        return rng.integers(0, 4, n, dtype=np.uint8).tobytes()
    words = [w.encode() + b" " for w in WORDS]
    out, size = [], 0
    for i in rng.integers(0, len(words), n // 4 + 8):
        out.append(words[i])
        size += len(words[i])
        if size >= n:
            break
    return b"".join(out)[:n]


def liblz4():
    try:
        L = C.CDLL("liblz4.so.1")
    except OSError:
        return None
    L.LZ4_compressBound.argtypes = [C.c_int]
    L.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    return L


def lib_compress(L, data, level=None):
    cap = L.LZ4_compressBound(len(data))
    buf = C.create_string_buffer(cap)
    n = (L.LZ4_compress_default(data, buf, len(data), cap) if level is None else
         L.LZ4_compress_HC(data, buf, len(data), cap, level))
    return buf.raw[:n]


def size_rows(L):
    import make_lz4_kat as K

    inputs = [(name, K.input_bytes(spec)) for name, spec in K.case_specs()]
    inputs += [(f"bench_{kind}_1MiB", generate(kind, 1 << 20, 1)) for kind in ("sentence", "low_entropy")]
    rows = []
    for name, data in inputs:
        row = {"what": "sizes", "input": name, "bytes": len(data), "ours": len(Z.host_encode(data)[0])}
        if L is not None:
            row["liblz4_default"] = len(lib_compress(L, data))
            row["liblz4_hc9"] = len(lib_compress(L, data, 9))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lz4_block.jsonl"))
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--search", type=lambda v: int(v, 0), nargs="+",
                    help="search words (depth 1, 2, 4 or 8, plus 0x100 for LAZY; 0: the one-candidate search): "
                         "only their encode rows are taken, and appended to the file")
    args = ap.parse_args()
    if args.search:
        with open(args.out, "a") as f:
            for r in search_rows(args.iters, args.search):
                f.write(json.dumps(r) + "\n")
                print(json.dumps(r), flush=True)
        return
    L = liblz4()
    rows = size_rows(L)
    if not args.sizes_only:
        rows = gpu_rows(args.iters, L) + rows
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


def search_rows(iters, words):
    """One "encode_search" row per shape of gpu_rows and search word: the whole call, timed as there."""
    import torch

    assert torch.cuda.is_available(), "lz4_bench --search needs a GPU"
    rows = []
    for kind in ("sentence", "low_entropy"):
        host = np.frombuffer(generate(kind, 16 << 20, 7), np.uint8)
        for nblocks, mib in ((256, 1), (16, 16)):
            bs = mib << 20
            total = nblocks * bs
            d_in = torch.from_numpy(np.concatenate([np.roll(host, 4099 * b)[:bs] for b in range(nblocks)])).to("cuda")
            offs, sizes = [b * bs for b in range(nblocks)], [bs] * nblocks
            for w in words:
                res = Z.encode_batch(d_in, offs, sizes, search=w)
                torch.cuda.synchronize()
                res.check()
                comp = int(res.sizes.sum().item())
                for _ in range(2):
                    Z.encode_batch(d_in, offs, sizes, search=w)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    Z.encode_batch(d_in, offs, sizes, search=w)
                b.record()
                torch.cuda.synchronize()
                t = a.elapsed_time(b) / 1e3 / iters
                rows.append({"what": "encode_search", "device": torch.cuda.get_device_name(0), "data": kind,
                             "blocks": nblocks, "block_bytes": bs, "iters": iters, "search": w, "seconds": t,
                             "gib_per_s": total / GIB / t, "compressed_bytes": comp, "ratio": comp / total})
            del d_in
    return rows


def gpu_rows(iters, L):
    import torch

    assert torch.cuda.is_available(), "lz4_bench needs a GPU (or --sizes-only)"
    dev = "cuda"

    def timed(fn):
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

    rows = []
    for kind in ("sentence", "low_entropy"):
        host = np.frombuffer(generate(kind, 16 << 20, 7), np.uint8)  # 16 MiB, rotated differently into every block
        for nblocks, mib in ((256, 1), (16, 16)):
            bs = mib << 20
            total = nblocks * bs
            flat = np.concatenate([np.roll(host, 4099 * b)[:bs] for b in range(nblocks)])
            d_in = torch.from_numpy(flat).to(dev)
            offs = [b * bs for b in range(nblocks)]
            sizes = [bs] * nblocks
            base = {"device": torch.cuda.get_device_name(0), "data": kind, "blocks": nblocks, "block_bytes": bs,
                    "iters": iters}
            res = Z.encode_batch(d_in, offs, sizes)
            torch.cuda.synchronize()
            res.check()
            comp = int(res.sizes.sum().item())
            t = timed(lambda: Z.encode_batch(d_in, offs, sizes))
            rows.append(dict(base, what="encode", seconds=t, gib_per_s=total / GIB / t, compressed_bytes=comp,
                             ratio=comp / total))
            out = torch.empty(total, dtype=torch.uint8, device=dev)
            Z.decode_batch(res.data, res.offsets, res.sizes, sizes, out=out, out_offsets=offs)
            torch.cuda.synchronize()
            assert torch.equal(out, d_in), "the decoder does not return the encoder's input"
            t = timed(lambda: Z.decode_batch(res.data, res.offsets, res.sizes, sizes, out=out, out_offsets=offs))
            rows.append(dict(base, what="decode", seconds=t, gib_per_s=total / GIB / t))
            t = timed(lambda: out.copy_(d_in))
            rows.append(dict(base, what="copy", seconds=t, gib_per_s=total / GIB / t))
            if L is not None:
                blocks = [flat[o:o + bs].tobytes() for o in offs]
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    streams = list(ex.map(lambda b: lib_compress(L, b), blocks))
                t = time.perf_counter() - t0
                rows.append(dict(base, what="liblz4_compress_default_16_threads", seconds=t, gib_per_s=total / GIB / t,
                                 compressed_bytes=sum(map(len, streams))))

                def unpack(s):
                    buf = C.create_string_buffer(bs)
                    assert L.LZ4_decompress_safe(s, buf, len(s), bs) == bs

                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(unpack, streams))
                t = time.perf_counter() - t0
                rows.append(dict(base, what="liblz4_decompress_safe_16_threads", seconds=t, gib_per_s=total / GIB / t))
            del d_in, out, res
    return rows


if __name__ == "__main__":
    main()
