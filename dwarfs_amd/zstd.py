"""DwarFS block codec for Zstandard over the MI355X kernels (Python mirror).

Mirrors ``zstd_block_compressor`` (src/compression/zstd.cpp:320-441), ``zstd_block_decompressor`` (:443-483) and
the factory registered as ``"zstd"`` with option ``level``.  A compressed DwarFS block is one
Zstandard frame (RFC 8878), as ``ZSTD_compress2`` writes it (:424-441); the compression type is ZSTD = 2
(include/dwarfs/compression.h:34-42).  The constructor reads the content size from the frame header, as
``ZSTD_getFrameContentSize`` does (:445-460): a frame without it raises ``ZSTD content size unknown``, a header
that cannot be parsed ``ZSTD content size error``; a failed decode raises
``failed to decompress frame (zstd error: <status>)`` (:475-480) with this library's status code.

The encoder is this project's own and deterministic (defined at the top of csrc/zstd_encode_host.cpp): one
frame per block, one Zstandard block per 32 KiB chunk of the LZ4 encoder's match search, predefined sequence
tables, no repeat offsets, no checksum; ``level`` is recorded and changes nothing (it maps to no search word).  The
search word (``search=``, or ``depth=N`` and ``lazy=0|1`` in a spec; ``depth | SEARCH_LAZY``, see lz4.py) turns on the
LZ4 encoder's deeper match search; 0, the default, is the one-candidate greedy search.  The options word
(``ENC_TABLES``, ``ENC_REPEAT``; ``ENC_ADAPTIVE`` is both) turns on per-block table modes and repeat-offset codes.  The long
word (``long=1``, or ``long`` / ``long=1`` in a spec given to ``block_compressor_long``, the reference's option at zstd.cpp:69 and :404-406) adds matches
against anything earlier in the same block (defined at the top of csrc/zstd_long_host.cpp); a block then holds
at most ``LONG_MAX_BLOCK`` bytes.  ``compress`` raises
:class:`lz4.BadCompressionRatioError` when the frame is no smaller than the input; the writer then stores the
block as type NONE, which ``compress_many_sections`` does.  ``zstd.block_compressor("zstd[:level=N]")`` makes
one; ``block_codec.block_compressor("zstd")`` is still an unknown compression.

The Content_Checksum is skipped, not verified, and dictionaries are refused.  ``device="cpu"`` runs the host
restatements of the kernels (rpp_zstd_host_encode / rpp_zstd_host_decode); the section helpers need the GPU.
Besides the one-block API there are ``compress_many`` / ``decompress_many``: one batch for many blocks.
"""

from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import section as S
from .codec import _raise_status, _stream_ptr
from .lz4 import (COMPRESSION_TYPE_NONE, MAX_BLOCK, SEARCH_LAZY, BadCompressionRatioError, EncodedBatch, _layout,
                  _ptr, _upload, check_search, spec_search)

COMPRESSION_TYPE_ZSTD = 2  # include/dwarfs/compression.h:34-42
FLAG_SINGLE_SEGMENT, FLAG_CHECKSUM, FLAG_CONTENT_SIZE = 1, 2, 4
# the encoder's options word: per-block table modes, repeat-offset codes, both
ENC_TABLES, ENC_REPEAT = N.RPP_ZSTD_ENC_TABLES, N.RPP_ZSTD_ENC_REPEAT
ENC_ADAPTIVE = ENC_TABLES | ENC_REPEAT
LONG_MAX_BLOCK = N.RPP_ZSTD_LONG_MAX_BLOCK  # a block's largest size with long=1


def check_long(long: int) -> int:
    if int(long) not in (0, 1):
        raise ValueError(f"unknown zstd long mode: {long}")
    return int(long)


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


def bound(n: int) -> int:
    return int(N.lib().rpp_zstd_bound(int(n)))


def host_encode(data: bytes, options: int = 0, search: int = 0, long: int = 0):
    """``rpp_zstd_host_encode_long``: (the frame, the ratio flag): the bytes the kernels write, on the CPU."""
    src = np.frombuffer(bytes(data) + b"\0", np.uint8)
    cap = bound(len(src) - 1)
    out = np.zeros(cap, np.uint8)
    n, flag = C.c_uint64(), C.c_uint32()
    _raise_status(N.lib().rpp_zstd_host_encode_long(src.ctypes.data_as(C.c_void_p), len(src) - 1, int(options),
                                                    int(search), int(long), out.ctypes.data_as(C.c_void_p), cap,
                                                    C.byref(n), C.byref(flag)))
    return out[:n.value].tobytes(), bool(flag.value)


def host_sequences(data: bytes, search: int = 0, long: int = 0) -> np.ndarray:
    """``rpp_zstd_host_long_sequences``: the (position, length, offset) rows that the host encoder writes the
    frame of (search, long) from (a debug export)."""
    src = np.frombuffer(bytes(data) + b"\0", np.uint8)
    rows = np.zeros((len(src) // 4 + 1, 3), np.uint32)  # (matches of 4 bytes that do not overlap)
    count = C.c_uint64()
    _raise_status(N.lib().rpp_zstd_host_long_sequences(src.ctypes.data_as(C.c_void_p), len(src) - 1, int(search),
                                                       int(long), rows.ctypes.data_as(C.c_void_p), len(rows),
                                                       C.byref(count)))
    return rows[:count.value].copy()


def encode_batch(d_in: torch.Tensor, in_offsets, in_sizes: Sequence[int],
                 stream: Optional[torch.cuda.Stream] = None, options: int = 0, search: int = 0,
                 long: int = 0) -> EncodedBatch:
    """One ``rpp_zstd_encode_batch_long`` over the blocks ``d_in[in_offsets[b] : + in_sizes[b]]`` (a uint8 CUDA
    tensor; host lists of offsets and sizes): one frame per block; ``flags`` is 1 where size >= input size.
    Asynchronous on the stream."""
    dev = d_in.device
    n = len(in_sizes)
    most = LONG_MAX_BLOCK if long else MAX_BLOCK
    for s in in_sizes:
        if s > most:
            raise ValueError(f"a block holds at most {most} bytes, not {s}")
    out_offs, cap = _layout([bound(s) for s in in_sizes])
    total = int(sum(int(s) for s in in_sizes))
    d_ioff, d_isz, d_ooff = S._i64(in_offsets, dev), S._i64(list(in_sizes), dev), S._i64(out_offs, dev)
    out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ws_bytes = int(N.lib().rpp_zstd_encode_workspace_bytes_long(total, n, int(long)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_zstd_encode_batch_long(_ptr(d_in), _ptr(d_ioff), _ptr(d_isz), n, int(options),
                                                     int(search), int(long), _ptr(out), _ptr(d_ooff), _ptr(sizes),
                                                     _ptr(flags), _ptr(status), total, _ptr(ws), ws_bytes,
                                                     _stream_ptr(stream)))
    return EncodedBatch(out, d_ooff, sizes, flags, status, d_in, d_ioff, d_isz)


class ZstdBlockCompressor:
    """``zstd_block_compressor`` (src/compression/zstd.cpp:320-441).  ``level`` (at most 22, ZSTD_maxCLevel) is
    recorded and does not change the search.  ``options`` is the encoder's options word (``ENC_TABLES``,
    ``ENC_REPEAT``, ``ENC_ADAPTIVE``), ``search`` the search word (``depth | SEARCH_LAZY``), ``long`` the long word (0 or 1);
    0, 0 and 0 write the bytes pinned in tests/golden/zstd_enc_kat.json."""

    def __init__(self, level: int = 22, device="cuda", options: int = 0, search: int = 0, long: int = 0):
        if int(level) > 22:
            raise RuntimeError(f"invalid option(s) for zstd: level={level}")
        if int(options) & ~ENC_ADAPTIVE:
            raise ValueError(f"unknown zstd encoder options: {options}")
        self.level = int(level)
        self.device = torch.device(device)
        self.options = int(options)
        self.search = check_search(search)
        self.long = check_long(long)

    def clone(self) -> "ZstdBlockCompressor":
        return ZstdBlockCompressor(self.level, self.device, self.options, self.search, self.long)

    def type(self) -> int:
        return COMPRESSION_TYPE_ZSTD

    def describe(self) -> str:
        # zstd.cpp:329-331 (which does not show its `long`; this one does)
        return f"zstd [level={self.level}, long]" if self.long else f"zstd [level={self.level}]"

    def metadata_requirements(self) -> str:
        return ""

    def get_compression_constraints(self, metadata: Optional[str] = None) -> dict:
        return {}

    def estimate_memory_usage(self, data_size: int) -> int:
        return data_size

    def _encode(self, blocks: Sequence[bytes]) -> EncodedBatch:
        d_in, offs = _upload(blocks, self.device)
        return encode_batch(d_in, offs, [len(b) for b in blocks], options=self.options, search=self.search,
                            long=self.long)

    def compress(self, data: bytes, metadata: Optional[str] = None) -> bytes:
        out = self.compress_many([data], metadata, keep_bad=True)[0]
        if out is None:
            raise BadCompressionRatioError()
        return out

    def compress_many(self, blocks: Sequence[bytes], metadata: Optional[str] = None,
                      keep_bad: bool = False) -> List[Optional[bytes]]:
        """Compresses many blocks in one batch.  A block that trips the ratio rule raises
        :class:`lz4.BadCompressionRatioError`, or with ``keep_bad`` comes back as None."""
        if not blocks:
            return []
        if self.device.type == "cpu":  # the host restatement: the kernels' bytes without a GPU
            frames, flags = zip(*(host_encode(b, self.options, self.search, self.long) for b in blocks))
        else:
            res = self._encode(blocks)
            torch.cuda.current_stream().synchronize()
            res.check()
            sizes, flags, offs = res.sizes.cpu().numpy(), res.flags.cpu().numpy(), res.offsets.cpu().numpy()
            data = res.data.cpu().numpy()
            frames = [data[o:o + n].tobytes() for o, n in zip(offs, sizes)]
        out: List[Optional[bytes]] = []
        for frame, flag in zip(frames, flags):
            if flag and not keep_bad:
                raise BadCompressionRatioError()
            out.append(None if flag else frame)
        return out

    def compress_many_sections(self, blocks: Sequence[bytes], metadata: Optional[str] = None,
                               first_number: int = 0) -> bytes:
        """Compresses many blocks and returns them as image-ready BLOCK sections, numbered from
        ``first_number``.  A block that trips the ratio rule becomes a NONE section (type 0, the raw bytes as
        payload), as the writer does (src/writer/filesystem_writer.cpp:282-284).  Encode, checksums and
        assembly run on the device; the sizes and ratio flags come to the host once in between."""
        if not blocks:
            return b""
        res = self._encode(blocks)
        torch.cuda.current_stream().synchronize()
        res.check()
        sizes, flags = res.sizes.cpu().numpy(), res.flags.cpu().numpy().astype(bool)
        enc_offs, in_offs = res.offsets.cpu().numpy(), res.in_offsets.cpu().numpy()
        payload = torch.cat([res.data, res.source])  # a NONE section's payload is the input itself
        offs = np.where(flags, res.data.numel() + in_offs, enc_offs)
        lens = np.where(flags, [len(b) for b in blocks], sizes)
        headers, i = [], 0
        while i < len(blocks):  # one header launch per run of sections of the same compression type
            j = i
            while j < len(blocks) and flags[j] == flags[i]:
                j += 1
            headers.append(S.section_headers_batch(payload, offs[i:j], lens[i:j], first_number + i, S.SECTION_TYPE_BLOCK,
                                                   COMPRESSION_TYPE_NONE if flags[i] else self.type()))
            i = j
        capacity = int(lens.sum()) + len(blocks) * S.HEADER_BYTES
        asm = S.sections_assemble_batch(torch.cat(headers), payload, offs, lens, capacity)  # (no DwarFS framing)
        return asm.bytes()


def block_compressor(spec: str, device="cuda") -> ZstdBlockCompressor:
    """The factory for ``zstd[:level=N][:depth=N][:lazy=0|1]``; any other option raises ``invalid option(s) for
    zstd: ...``, ``long`` among them (:func:`block_compressor_long` takes it).  ``depth`` and ``lazy`` make the
    search word; ``level`` maps to none."""
    return _from_spec(spec, device, False)


def block_compressor_long(spec: str, device="cuda") -> ZstdBlockCompressor:
    """The factory for ``zstd[:level=N][:long[=0|1]][:depth=N][:lazy=0|1]``: :func:`block_compressor` with the
    reference's ``long`` option (a flag, as in its option map: alone it means 1), which makes the long word."""
    return _from_spec(spec, device, True)


def _from_spec(spec: str, device, with_long: bool) -> ZstdBlockCompressor:
    name, *opts = spec.split(":")
    if name != "zstd":
        raise RuntimeError(f"unknown compression: {name}")
    level, long = [22], [0]
    if with_long:
        opts = ["long=1" if opt == "long" else opt for opt in opts]

    def take(key, value):
        if with_long and key == "long" and value in ("0", "1"):
            long[0] = int(value)
            return True
        try:
            if key != "level" or int(value) > 22:
                return False
        except ValueError:
            return False
        level[0] = int(value)
        return True

    search = spec_search(opts, "zstd", take)
    return ZstdBlockCompressor(level[0], device, search=search, long=long[0])
