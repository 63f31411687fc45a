"""DwarFS FLAC block codec over the MI355X kernels (Python mirror).

Mirrors src/compression/flac.cpp: ``flac_block_compressor`` (:215-403),
``flac_block_decompressor`` (:405-489) and the factory registered as
``"flac"`` with options ``level`` (default 5) and ``exhaustive`` (:509-525).
A compressed DwarFS block is

    varint(uncompressed bytes) + thrift-compact flac_block_header + FLAC stream

(framing by the C ABI: rpp_flac_frame_header / rpp_flac_parse_frame,
rpp_flac_stream_header / rpp_flac_parse_stream).  The PCM bytes become int32
samples on the device (rpp_pcm_unpack, the pcm_sample_transformer of
flac.cpp:322-334) and 4096-sample FLAC frames (rpp_flac_encode); decoding runs
the other way (rpp_flac_decode, rpp_pcm_pack).

FLAC decode is pinned to libFLAC 1.3.3 by the three RFC 9639 Appendix D
streams and their MD5s (tests/golden/flac_rfc9639.json); the encoder is pinned
to the format by an independent RFC 9639 reader (tests/flac_ref.py) and its
choices to a rule-by-rule model (tests/flac_enc_model.py: byte for byte at
levels 0-2, from level 3 given the coefficients it wrote); it is not pinned to
libFLAC's encoder choices, and this remains unpinned: libFLAC's model search (LPC orders, precision, apodization) decides its bytes,
and this encoder writes valid FLAC with fixed and LPC predictors chosen by its
own search.  The decoder reads every frame kind RFC 9639 defines.  ``level`` selects libFLAC's preset limits (levels 0-2 fixed
predictors only, 3 LPC up to order 6, 4-6 up to 8, 7-8 up to 12) and
``exhaustive`` codes every LPC order instead of the estimated best
(rpp_flac_encode_ex; flac.cpp:312-313).
"""

from __future__ import annotations

import ctypes as C
import json
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .pcm import PcmSampleEndianness, PcmSamplePadding, PcmSampleSignedness, PcmSampleTransformer

COMPRESSION_TYPE_FLAC = 6  # include/dwarfs/compression.h:41
FLAG_BIG_ENDIAN, FLAG_SIGNED, FLAG_LSB_PADDING, BYTES_PER_SAMPLE_MASK = 0x80, 0x40, 0x20, 0x03  # flac.cpp:41-44


def _dump(obj) -> str:
    """nlohmann::json::dump() of an object: keys sorted, no spaces."""
    return json.dumps(obj, sort_keys=True, separators=(",", ":"))


def _status(st: int, what: str) -> None:
    if st != N.RPP_OK:
        raise RuntimeError(f"[FLAC] {what}: {N.STATUS_NAMES.get(st, st)}")


def frame_header(uncompressed: int, channels: int, bits: int, flags: int) -> bytes:
    f = N.RppFlacFrame(uncompressed, channels, bits, flags)
    buf = (C.c_uint8 * 64)()
    n = N.lib().rpp_flac_frame_header(C.byref(f), buf)
    return bytes(buf[:n])


def parse_frame(data: bytes):
    buf = np.frombuffer(data, np.uint8)
    f = N.RppFlacFrame()
    n = N.lib().rpp_flac_parse_frame(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(f))
    if n < 0:
        raise RuntimeError("malformed flac block header")
    return f, int(n)


def parse_stream(stream: bytes):
    buf = np.frombuffer(stream, np.uint8)
    info = N.RppFlacStreamInfo()
    n = N.lib().rpp_flac_parse_stream(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(info))
    if n < 0:
        raise RuntimeError(f"[FLAC] could not initialize decoder: {N.STATUS_NAMES.get(n, n)}")
    return info, int(n)


def _transformer(flags: int, bits: int) -> PcmSampleTransformer:
    return PcmSampleTransformer(
        PcmSampleEndianness.Big if flags & FLAG_BIG_ENDIAN else PcmSampleEndianness.Little,
        PcmSampleSignedness.Signed if flags & FLAG_SIGNED else PcmSampleSignedness.Unsigned,
        PcmSamplePadding.Lsb if flags & FLAG_LSB_PADDING else PcmSamplePadding.Msb,
        (flags & BYTES_PER_SAMPLE_MASK) + 1, bits)


class FlacBlockCompressor:
    """``flac_block_compressor`` (src/compression/flac.cpp:215-403)."""

    def __init__(self, level: int = 5, exhaustive: bool = False, device="cuda"):
        self.level = int(level)
        self.exhaustive = bool(exhaustive)
        self.device = torch.device(device)

    def clone(self) -> "FlacBlockCompressor":
        return FlacBlockCompressor(self.level, self.exhaustive, self.device)

    def type(self) -> int:
        return COMPRESSION_TYPE_FLAC

    def describe(self) -> str:  # :363-366
        return f"flac [level={self.level}{', exhaustive' if self.exhaustive else ''}]"

    def metadata_requirements(self) -> str:  # :368-379 (nlohmann::json dump: keys sorted, compact)
        return _dump({
            "endianness": ["set", ["big", "little"]],
            "signedness": ["set", ["signed", "unsigned"]],
            "padding": ["set", ["msb", "lsb"]],
            "bytes_per_sample": ["range", 1, 4],
            "bits_per_sample": ["range", 8, 32],
            "number_of_channels": ["range", 1, 8],
        })

    def get_compression_constraints(self, metadata: str) -> dict:  # :381-393
        m = json.loads(metadata)
        return {"granularity": int(m["number_of_channels"]) * int(m["bytes_per_sample"])}

    def estimate_memory_usage(self, data_size: int) -> int:  # :395-398
        return int(data_size)

    @staticmethod
    def _prepare(data: bytes, metadata: Optional[str]):
        """The block's framing (varint + flac_block_header + fLaC/STREAMINFO) and PCM shape (flac.cpp:284-304)."""
        if metadata is None:
            raise RuntimeError("internal error: flac compression requires metadata")
        m = json.loads(metadata)
        channels, bits, nbytes = int(m["number_of_channels"]), int(m["bits_per_sample"]), int(m["bytes_per_sample"])
        if len(data) % (channels * nbytes):
            raise RuntimeError(f"unexpected PCM waveform configuration: {len(data)} bytes to compress, "
                               f"{channels} channels, {nbytes} bytes per sample")
        flags = nbytes - 1
        if m["endianness"] == "big":
            flags |= FLAG_BIG_ENDIAN
        if m["signedness"] == "signed":
            flags |= FLAG_SIGNED
        if m["padding"] == "lsb":
            flags |= FLAG_LSB_PADDING
        head = frame_header(len(data), channels, bits, flags)
        n = len(data) // (channels * nbytes)  # samples per channel
        sh = (C.c_uint8 * 64)()
        sl = N.lib().rpp_flac_stream_header(channels, bits, n, sh)
        return head + bytes(sh[:sl]), n, channels, bits, flags

    def compress(self, data: bytes, metadata: Optional[str]) -> bytes:
        prefix, n, channels, bits, flags = self._prepare(data, metadata)
        if n == 0:
            return prefix
        dev = self.device
        raw = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
        x = torch.empty(n * channels, dtype=torch.int32, device=dev)
        _transformer(flags, bits).unpack(x, raw)
        L = N.lib()
        frames = (n + 4095) // 4096
        out = torch.empty(frames * int(L.rpp_flac_frame_bound(channels, bits)) + 64, dtype=torch.uint8, device=dev)
        ws_bytes = int(L.rpp_flac_encode_workspace_bytes(n, channels, bits))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev)
        _status(L.rpp_flac_encode_ex(C.c_void_p(x.data_ptr()), n, channels, bits, self.level, int(self.exhaustive),
                                     C.c_void_p(out.data_ptr()), C.c_void_p(total.data_ptr()),
                                     C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(s.cuda_stream)), "encode")
        size = int(total.item())
        return prefix + out[:size].cpu().numpy().tobytes()

    def compress_many(self, items) -> list:
        """compress() of every (data, metadata) pair, all blocks' frames in one launch (rpp_flac_encode_batch);
        the result is byte-identical to calling compress() per block."""
        items = list(items)
        if not items:
            return []
        preps = [self._prepare(d, m) for d, m in items]
        dev = self.device
        nb = len(items)
        n = np.array([p[1] for p in preps], np.uint64)
        ch = np.array([p[2] for p in preps], np.uint32)
        bp = np.array([p[3] for p in preps], np.uint32)
        vals = n * ch
        in_off = np.zeros(nb, np.uint64)
        if nb > 1:
            in_off[1:] = np.cumsum(vals)[:-1]
        x = torch.empty(max(int(vals.sum()), 1), dtype=torch.int32, device=dev)
        for b, ((data, _), p) in enumerate(zip(items, preps)):
            if p[1]:
                raw = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
                _transformer(p[4], p[3]).unpack(x[int(in_off[b]):int(in_off[b] + vals[b])], raw)
        L = N.lib()
        P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        frames = int(sum((int(v) + 4095) // 4096 for v in n))
        bound = max(int(L.rpp_flac_frame_bound(int(c), int(b))) for c, b in zip(ch, bp))
        out = torch.empty(frames * bound + 64, dtype=torch.uint8, device=dev)
        offs = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
        ws_bytes = int(L.rpp_flac_encode_batch_workspace_bytes(nb, P(n), P(ch), P(bp)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev)
        _status(L.rpp_flac_encode_batch(C.c_void_p(x.data_ptr()), nb, P(in_off), P(n), P(ch), P(bp), self.level,
                                        int(self.exhaustive), C.c_void_p(out.data_ptr()), C.c_void_p(offs.data_ptr()),
                                        C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(s.cuda_stream)), "encode")
        o = offs.cpu().numpy()
        host = out[: int(o[-1])].cpu().numpy().tobytes()
        return [p[0] + host[int(o[b]):int(o[b + 1])] for b, p in enumerate(preps)]


class FlacBlockDecompressor:
    """``flac_block_decompressor`` (src/compression/flac.cpp:405-489)."""

    def __init__(self, data: bytes, device="cuda"):
        f, n = parse_frame(data)
        self.frame = f
        self.stream = data[n:]
        self.info, self.frames_at = parse_stream(self.stream)
        self.device = torch.device(device)
        self._target: Optional[bytearray] = None
        self._done = False

    def type(self) -> int:
        return COMPRESSION_TYPE_FLAC

    def uncompressed_size(self) -> int:
        return int(self.frame.uncompressed_bytes)

    def metadata(self) -> str:  # :429-440 (nlohmann::json dump: keys sorted, compact)
        fl = int(self.frame.flags)
        return _dump({
            "endianness": "big" if fl & FLAG_BIG_ENDIAN else "little",
            "signedness": "signed" if fl & FLAG_SIGNED else "unsigned",
            "padding": "lsb" if fl & FLAG_LSB_PADDING else "msb",
            "bytes_per_sample": (fl & BYTES_PER_SAMPLE_MASK) + 1,
            "bits_per_sample": int(self.frame.bits_per_sample),
            "number_of_channels": int(self.frame.num_channels),
        })

    def start_decompression(self, target: bytearray) -> None:
        self._target = target

    def decompress_frame(self, frame_size: int = 0) -> bool:
        if self._target is None:
            raise RuntimeError("decompression not started")
        if self._done:
            return False
        self._target[:] = self.decompress()
        self._done = True
        return True

    def _plan(self):
        """The decode's parameters (None: no samples): frames, channels, bits, bytes per sample, samples per
        channel, max block size, candidate slots."""
        info, fl = self.info, int(self.frame.flags)
        channels, bits = int(info.channels), int(info.bits_per_sample)
        nbytes = (fl & BYTES_PER_SAMPLE_MASK) + 1
        n = int(info.total_samples)
        if n * channels * nbytes != self.uncompressed_size():
            raise RuntimeError("[FLAC] failed to process frame: stream length does not match the block")
        if n == 0:
            return None
        body = np.frombuffer(self.stream, np.uint8)[self.frames_at:]
        min_bs = max(16, int(info.min_blocksize) or 16)
        max_bs = int(info.max_blocksize) or 65535
        # Frames: at most n // min_bs + 1 (every block but the last holds at
        # least min_bs samples); spurious sync codes that pass the CRC-8 are
        # rare and handled by the retry of the callers.  Every candidate gets a
        # scratch slot of max_bs samples: a STREAMINFO whose block-size range
        # would make that more than 4x the block's samples (libFLAC writes
        # min == max; DwarFS's flac compressor uses fixed blocking) is refused
        # rather than allowed to size the workspace from a crafted header.
        max_cand = n // min_bs + 65
        if max_cand * max_bs > 4 * n + 128 * max_bs:
            raise RuntimeError("[FLAC] failed to process frame: block size range "
                               f"{int(info.min_blocksize)}..{max_bs} too wide for {n} samples")
        return body, channels, bits, nbytes, n, max_bs, max_cand

    @staticmethod
    def _more_candidates(found: int, n: int, max_bs: int, channels: int, bits: int) -> int:
        """The candidate table for the second pass.  Every candidate has a scratch slot of max_bs samples per
        channel: the slots may take 4x the block's samples + 128 slots (the bound of _plan) or, for the small
        blocks where that is only a few hundred candidates, 64 MiB."""
        slot = max_bs * channels * (8 if bits == 32 else 4)
        if found * max_bs > 4 * n + 128 * max_bs and (found + 64) * slot > 64 << 20:  # (a stream full of false sync codes)
            raise RuntimeError(f"[FLAC] failed to process frame: {found} frame candidates")
        return found + 64  # (more sync candidates than estimated: again, with room for all)

    def _finish(self, x: torch.Tensor, st: int, nbytes: int) -> bytes:
        if st != N.RPP_OK:
            raise RuntimeError(f"[FLAC] failed to process frame: {N.STATUS_NAMES.get(st, st)}")
        out = torch.empty(x.numel() * nbytes, dtype=torch.uint8, device=self.device)
        _transformer(int(self.frame.flags), int(self.frame.bits_per_sample)).pack(out, x)
        return out.cpu().numpy().tobytes()

    def decompress(self) -> bytes:
        plan = self._plan()
        if plan is None:
            return b""
        body, channels, bits, nbytes, n, max_bs, max_cand = plan
        dev = self.device
        d_in = torch.from_numpy(body.copy()).to(dev)
        x = torch.empty(n * channels, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ncand = torch.zeros(1, dtype=torch.int32, device=dev)
        L = N.lib()
        s = torch.cuda.current_stream(dev)
        for _ in range(2):
            ws_bytes = int(L.rpp_flac_decode_workspace_bytes(len(body), channels, bits, max_bs, max_cand))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _status(L.rpp_flac_decode(C.c_void_p(d_in.data_ptr()), len(body), channels, bits, max_bs, n,
                                      C.c_void_p(x.data_ptr()), C.c_void_p(status.data_ptr()), max_cand,
                                      C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(ncand.data_ptr()),
                                      C.c_void_p(s.cuda_stream)), "decode")
            found = int(ncand.item())
            if found <= max_cand:
                break
            max_cand = self._more_candidates(found, n, max_bs, channels, bits)
        return self._finish(x, int(status.item()), nbytes)


def decompress_many(blocks, device="cuda") -> list:
    """``block_decompressor::decompress`` of every FLAC block in ``blocks``, all streams' frames decoded in one
    sequence of launches (rpp_flac_decode_batch); byte-identical to decompress() per block (the first failing
    block raises its error)."""
    decs = [FlacBlockDecompressor(b, device) for b in blocks]
    plans = [d._plan() for d in decs]
    live = [i for i, pl in enumerate(plans) if pl is not None]
    outs = [b""] * len(decs)
    if not live:
        return outs
    dev = torch.device(device)
    nb = len(live)
    body_len = np.array([len(plans[i][0]) for i in live], np.uint64)
    in_off = np.zeros(nb, np.uint64)
    in_off[1:] = np.cumsum((body_len + 15) // 16 * 16)[:-1]
    buf = np.zeros(int(in_off[-1] + body_len[-1]) + 16, np.uint8)
    for k, i in enumerate(live):
        buf[int(in_off[k]):int(in_off[k] + body_len[k])] = plans[i][0]
    d_in = torch.from_numpy(buf).to(dev)
    ch = np.array([plans[i][1] for i in live], np.uint32)
    bp = np.array([plans[i][2] for i in live], np.uint32)
    ns = np.array([plans[i][4] for i in live], np.uint64)
    mbs = np.array([plans[i][5] for i in live], np.uint32)
    mc = np.array([plans[i][6] for i in live], np.uint32)
    vals = ns * ch
    out_off = np.zeros(nb, np.uint64)
    out_off[1:] = np.cumsum(vals)[:-1]
    x = torch.empty(int(vals.sum()), dtype=torch.int32, device=dev)
    status = torch.zeros(nb, dtype=torch.int32, device=dev)
    ncand = torch.zeros(nb, dtype=torch.int32, device=dev)
    L = N.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    s = torch.cuda.current_stream(dev)
    for _ in range(2):
        ws_bytes = int(L.rpp_flac_decode_batch_workspace_bytes(nb, P(body_len), P(ch), P(bp), P(mbs), P(mc)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _status(L.rpp_flac_decode_batch(C.c_void_p(d_in.data_ptr()), nb, P(in_off), P(body_len), P(ch), P(bp),
                                        P(mbs), P(ns), C.c_void_p(x.data_ptr()), P(out_off),
                                        C.c_void_p(status.data_ptr()), P(mc), C.c_void_p(ws.data_ptr()), ws_bytes,
                                        C.c_void_p(ncand.data_ptr()), C.c_void_p(s.cuda_stream)), "decode")
        found = ncand.cpu().numpy().astype(np.int64)
        over = found > mc
        if not over.any():
            break
        for k in np.nonzero(over)[0]:
            mc[k] = FlacBlockDecompressor._more_candidates(int(found[k]), int(ns[k]), int(mbs[k]), int(ch[k]),
                                                           int(bp[k]))
    st = status.cpu().numpy()
    for k, i in enumerate(live):
        lo = int(out_off[k])
        outs[i] = decs[i]._finish(x[lo:lo + int(vals[k])], int(st[k]), plans[i][3])
    return outs


def decompress(data: bytes, device="cuda") -> bytes:
    """``block_decompressor::decompress`` for a FLAC block."""
    return FlacBlockDecompressor(data, device).decompress()


def block_compressor(spec: str, device="cuda") -> FlacBlockCompressor:
    """``block_compressor(spec)`` for ``flac[:level=N][:exhaustive]`` (flac.cpp:509-525)."""
    name, _, opts = spec.partition(":")
    if name != "flac":
        raise RuntimeError(f"unknown compression: {name}")
    level, exhaustive = 5, False
    for kv in filter(None, opts.replace(":", ",").split(",")):
        k, eq, v = kv.partition("=")
        if k == "level" and eq and v.isdigit() and 0 <= int(v) <= 8:
            level = int(v)
        elif k == "exhaustive" and not eq:
            exhaustive = True
        else:
            raise RuntimeError(f"invalid option(s) for flac: {kv}")
    return FlacBlockCompressor(level, exhaustive, device)
