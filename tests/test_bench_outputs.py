"""bench.py --dump-outputs and the plain / --full result line.

The CPU tests drive bench.dump_outputs with a stand-in for ShardPipeline on host tensors; the GPU test runs
the benchmark itself at a small size and checks the dumped arrays against the CPU oracle."""

import json
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sizes", "image_offsets", "enc_status", "dec_status", "encoded", "decoded")


def fake_pipe(sizes, caps, n_samples, seed=1):
    """Host tensors laid out as ShardPipeline's: block i's bytes at out_offsets[i], capacity caps[i], of which
    sizes[i] are valid; the rest of the buffer holds 255 (a dump that reads a gap shows it)."""
    rng = np.random.default_rng(seed)
    sizes, caps = np.asarray(sizes, np.int64), np.asarray(caps, np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    data = np.full(int(caps.sum()), 255, np.uint8)
    image = rng.integers(0, 200, int(sizes.sum()), dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    for o, s, z in zip(out_off, starts, sizes):
        data[o:o + z] = image[s:s + z]
    decoded = rng.integers(-32768, 32768, int(n_samples), dtype=np.int16)
    pipe = SimpleNamespace(
        data=torch.from_numpy(data), sizes=torch.from_numpy(sizes), out_offsets=out_off,
        image_offsets=torch.from_numpy(starts), enc_status=torch.zeros(len(sizes), dtype=torch.int32),
        dec_status=torch.zeros(len(sizes), dtype=torch.int32), decoded=torch.from_numpy(decoded),
        total_samples=int(n_samples))
    return pipe, image, decoded


def load(d):
    return {n: np.load(d / f"{n}.npy") for n in NAMES}


def test_dump_small_is_whole_and_skips_capacity_gaps(tmp_path):
    pipe, image, decoded = fake_pipe([5, 0, 17, 1], [16, 16, 32, 16], 1000)
    bench.dump_outputs(pipe, tmp_path)
    got = load(tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.npy" for n in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["sizes"].tolist() == [5, 0, 17, 1] and got["image_offsets"].tolist() == [0, 5, 5, 22]
    assert np.array_equal(got["encoded"], image.astype(np.float32))
    assert np.array_equal(got["decoded"], decoded.astype(np.float32))


def test_dump_large_is_a_fixed_sample_within_budget(tmp_path):
    nblocks = 37
    rng = np.random.default_rng(5)
    sizes = rng.integers(150_000, 250_000, nblocks)  # ~7.4 M bytes: more than DUMP_SAMPLE
    pipe, image, decoded = fake_pipe(sizes, sizes + rng.integers(0, 64, nblocks), bench.DUMP_SAMPLE + 12345)
    assert sizes.sum() > bench.DUMP_SAMPLE
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(pipe, a)
    bench.dump_outputs(pipe, b)
    ga, gb = load(a), load(b)
    assert all(np.array_equal(ga[n], gb[n]) for n in NAMES)
    assert ga["encoded"].shape == ga["decoded"].shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(ga["encoded"], image[bench._dump_indices(len(image))].astype(np.float32))
    assert np.array_equal(ga["decoded"], decoded[bench._dump_indices(len(decoded))].astype(np.float32))
    assert sum(p.stat().st_size for p in a.iterdir()) <= 64_000_000


def test_dump_per_rank_names(tmp_path):
    pipe, _, _ = fake_pipe([3, 4], [16, 16], 10)
    bench.dump_outputs(pipe, tmp_path, rank=1, world=2)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.rank1.npy" for n in NAMES)


def run_bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_line_and_dump_against_oracle(tmp_path):
    """16 x 64 KiB blocks, 3 timed steps: the plain line carries the headline fields and nothing of --full;
    the dump holds the round trip of the seeded input and the oracle's bitstreams, byte for byte."""
    from oracle import oracle as O

    nblocks, n = 16, 32768
    res = run_bench("--blocks", str(nblocks), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert res["steps"] == 3 and res["unit"] == "GiB/s" and res["higher_is_better"] is True and res["dtype"] == "u16"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(nblocks * n * 2 / (res["ms_per_step"] * 1e-3) / 2**30, rel=1e-3)
    assert "roofline" not in res and "cpu_baseline" not in res and "encode_kernel_us" not in res["config"]
    got = load(tmp_path)
    x = bench.make_poisson_blocks(nblocks, n, 1000.0, 42, torch.device("cuda:0")).cpu().numpy()
    assert np.array_equal(got["decoded"], x.astype(np.float32))
    oc = O.cfg(128, 1, True, 0)
    want = [O.encode(oc, x[i * n:(i + 1) * n].view(np.uint16)) for i in range(nblocks)]
    assert got["sizes"].tolist() == [len(w) for w in want]
    assert got["image_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])[:-1]]).tolist()
    assert np.array_equal(got["encoded"], np.frombuffer(b"".join(want), np.uint8).astype(np.float32))
    assert not got["enc_status"].any() and not got["dec_status"].any()


@pytest.mark.gpu
def test_bench_full_line_keeps_every_block():
    res = run_bench("--blocks", "16", "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.2")
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["roofline"]["bound"] == "hbm" and res["roofline"]["device_copy_GBps"] > 0
    assert res["config"]["encode_kernel_us"] > 0 and res["config"]["decode_kernel_us"] > 0
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["kind"] == "port"
