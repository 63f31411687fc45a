"""DwarFS block decoder for Zstandard over the MI355X kernels (Python mirror).

Mirrors ``zstd_block_decompressor`` of src/compression/zstd.cpp:443-483.  A compressed DwarFS block is one
Zstandard frame (RFC 8878), as ``ZSTD_compress2`` writes it (:424-441); the compression type is ZSTD = 2
(include/dwarfs/compression.h:34-42).  The constructor reads the content size from the frame header, as
``ZSTD_getFrameContentSize`` does (:445-460): a frame without it raises ``ZSTD content size unknown``, a header
that cannot be parsed ``ZSTD content size error``; a failed decode raises
``failed to decompress frame (zstd error: <status>)`` (:475-480) with this library's status code.

There is no encoder: ``block_codec.block_compressor("zstd")`` is an unknown compression.  The Content_Checksum
is skipped, not verified, and dictionaries are refused.  ``device="cpu"`` runs the host restatement of the
kernels (rpp_zstd_host_decode); the section helpers need the GPU.  Besides the one-block API there is
``decompress_many``: one batch for many blocks.
"""

from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import section as S
from .codec import _raise_status, _stream_ptr
from .lz4 import _layout, _ptr, _upload

COMPRESSION_TYPE_ZSTD = 2  # include/dwarfs/compression.h:34-42
FLAG_SINGLE_SEGMENT, FLAG_CHECKSUM, FLAG_CONTENT_SIZE = 1, 2, 4


class FrameInfo(NamedTuple):
    header_bytes: int
    content_size: Optional[int]  # None: the frame does not state it
    window: int
    flags: int


def frame_info(data: bytes) -> FrameInfo:
    """``rpp_zstd_frame_info``; a header that cannot be parsed raises like ZSTD_CONTENTSIZE_ERROR."""
    buf = np.frombuffer(bytes(data[:18]) + b"\0", np.uint8)  # (a frame header is 18 bytes at most)
    size, window, flags = C.c_uint64(), C.c_uint64(), C.c_uint32()
    n = N.lib().rpp_zstd_frame_info(buf.ctypes.data_as(C.c_void_p), len(buf) - 1, C.byref(size), C.byref(window),
                                    C.byref(flags))
    if n < 0:
        raise RuntimeError("ZSTD content size error")
    has = bool(flags.value & FLAG_CONTENT_SIZE)
    return FrameInfo(int(n), int(size.value) if has else None, int(window.value), int(flags.value))


def count_blocks(data: bytes) -> int:
    """``rpp_zstd_count_blocks``: the blocks of a frame, or a negative status."""
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    return int(N.lib().rpp_zstd_count_blocks(buf.ctypes.data_as(C.c_void_p), len(buf) - 1))


def host_decode(frame: bytes, size: int):
    """``rpp_zstd_host_decode``: (status, the ``size`` output bytes as they stand when decoding ends)."""
    src = np.frombuffer(bytes(frame) + b"\0", np.uint8)
    out = np.zeros(max(int(size), 1), np.uint8)
    st = N.lib().rpp_zstd_host_decode(src.ctypes.data_as(C.c_void_p), len(src) - 1, out.ctypes.data_as(C.c_void_p),
                                      int(size))
    return int(st), out[:size].tobytes()


def decode_batch(d_in: torch.Tensor, in_offsets, in_sizes, out_sizes: Sequence[int], max_blocks: int,
                 stream: Optional[torch.cuda.Stream] = None, out: Optional[torch.Tensor] = None, out_offsets=None,
                 total_out: Optional[int] = None):
    """One ``rpp_zstd_decode_batch``: (uint8 output tensor, its int64 offsets on the host, int32 status tensor).
    ``max_blocks`` is the number of blocks of all frames together (``count_blocks``); ``total_out`` the output
    bytes the workspace is sized for (default: the sum of ``out_sizes``).  Asynchronous on the stream."""
    dev = d_in.device
    n = len(out_sizes)
    if out_offsets is None:
        out_offsets, cap = _layout(out_sizes)
    else:
        cap = out.numel()
    if out is None:
        out = torch.zeros(max(cap, 16), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if total_out is None:
        total_out = int(sum(int(s) for s in out_sizes))
    ws_bytes = int(N.lib().rpp_zstd_decode_workspace_bytes(int(total_out), int(max_blocks)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    d_ioff, d_isz = S._i64(in_offsets, dev), S._i64(in_sizes, dev)
    d_ooff, d_osz = S._i64(out_offsets, dev), S._i64(list(out_sizes), dev)
    _raise_status(N.lib().rpp_zstd_decode_batch(_ptr(d_in), _ptr(d_ioff), _ptr(d_isz), n, _ptr(out), _ptr(d_ooff),
                                                _ptr(d_osz), _ptr(status), int(max_blocks), _ptr(ws), ws_bytes,
                                                _stream_ptr(stream)))
    return out, np.asarray(out_offsets, np.int64), status


class ZstdBlockDecompressor:
    """``zstd_block_decompressor`` (src/compression/zstd.cpp:443-491)."""

    def __init__(self, data: bytes, device="cuda"):
        size = frame_info(data).content_size
        if size is None:
            raise RuntimeError("ZSTD content size unknown")
        self._size = size
        self.data = bytes(data)
        self.device = torch.device(device)
        self._target: Optional[bytearray] = None
        self._done = False

    def type(self) -> int:
        return COMPRESSION_TYPE_ZSTD

    def uncompressed_size(self) -> int:
        return self._size

    def metadata(self) -> Optional[str]:
        return None

    def start_decompression(self, target: bytearray) -> None:
        self._target = target

    def decompress_frame(self, frame_size: int = 0) -> bool:
        if self._target is None:
            raise RuntimeError("decompression not started")
        if self._done:
            return False
        self._target[:] = decompress_many([self], self.device)[0]
        self._done = True
        return True


def raise_decode_status(st: int) -> None:
    """zstd.cpp:475-480: a failed decode is a runtime_error that names the decoder's result."""
    if st != N.RPP_OK:
        raise RuntimeError(f"failed to decompress frame (zstd error: {st})")


def decompress(data: bytes, device="cuda") -> bytes:
    """``block_decompressor::decompress`` (src/block_decompressor.cpp:41-49)."""
    return decompress_many([ZstdBlockDecompressor(data, device)], device)[0]


def decompress_many(decs: Sequence[ZstdBlockDecompressor], device="cuda") -> List[bytes]:
    """Decodes many Zstandard frames in one batch."""
    if not decs:
        return []
    dev = torch.device(device)
    sizes = [d.uncompressed_size() for d in decs]
    if dev.type == "cpu":  # the host restatement
        results = [host_decode(d.data, n) for d, n in zip(decs, sizes)]
        for st, _ in results:
            raise_decode_status(st)
        return [out for _, out in results]
    blocks = [count_blocks(d.data) for d in decs]
    for b in blocks:
        raise_decode_status(min(b, 0))
    d_in, offs = _upload([d.data for d in decs], dev)
    out, out_offs, status = decode_batch(d_in, offs, [len(d.data) for d in decs], sizes, sum(blocks))
    torch.cuda.current_stream().synchronize()
    host = out.cpu().numpy()
    for st in status.cpu().numpy():
        raise_decode_status(int(st))
    return [host[o:o + n].tobytes() for o, n in zip(out_offs, sizes)]
