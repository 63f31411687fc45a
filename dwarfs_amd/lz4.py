"""DwarFS block codec for LZ4 over the MI355X kernels (Python mirror).

Mirrors src/compression/lz4.cpp: ``lz4_block_compressor`` (:60-117, one class for ``lz4`` and ``lz4hc``),
``lz4_block_decompressor`` (:119-171) and the factories registered as ``"lz4"`` and ``"lz4hc"`` with option
``level`` (:173-222).  A compressed DwarFS block is

    uint32 little-endian uncompressed size + one LZ4 block

(the framing comes from the C ABI: rpp_lz4_frame_header / rpp_lz4_parse_frame).  Compression types are LZ4 = 3
and LZ4HC = 4 (include/dwarfs/compression.h:34-42); both decode alike.  ``compress`` raises
:class:`BadCompressionRatioError` when the framed payload is no smaller than the input; the writer then stores
the block as type NONE (src/writer/filesystem_writer.cpp:282-284, 539-541), which ``compress_many_sections``
does.

``device="cpu"`` runs the host restatement of the kernels (rpp_lz4_host_encode / rpp_lz4_host_decode), which
writes the same bytes; the section helpers need the GPU.

One encoder serves both names: ``lz4hc:level=N`` records the level (0..12) and maps to no search: what changes
the search is the search word (``search=``, or ``depth=N`` and ``lazy=0|1`` in a spec), ``depth | SEARCH_LAZY``
with a depth of 1, 2, 4 or 8 candidates per hash value; 0, the default, is the one-candidate greedy search
(defined at the top of csrc/lz4_host.cpp).  Besides the one-block API there are ``compress_many`` /
``decompress_many``: one launch for a batch.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import section as S
from .codec import _raise_status, _stream_ptr

COMPRESSION_TYPE_NONE = 0  # include/dwarfs/compression.h:34-42
COMPRESSION_TYPE_LZ4 = 3
COMPRESSION_TYPE_LZ4HC = 4
MAX_BLOCK = 1 << 30  # RPP_LZ4_MAX_BLOCK
FRAME_BYTES = 4
SEARCH_LAZY = N.RPP_SEARCH_LAZY  # the search word: depth (1, 2, 4 or 8) | SEARCH_LAZY; 0: the one-candidate search


class BadCompressionRatioError(RuntimeError):
    """``bad_compression_ratio_error`` (include/dwarfs/block_compressor.h): the block did not shrink."""

    def __init__(self):
        super().__init__("bad compression ratio")


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def bound(n: int) -> int:
    return int(N.lib().rpp_lz4_bound(int(n)))


def frame_header(uncompressed: int) -> bytes:
    buf = (C.c_uint8 * 4)()
    n = N.lib().rpp_lz4_frame_header(int(uncompressed), buf)
    return bytes(buf[:n])


def parse_frame(data: bytes):
    """(uncompressed size, offset of the LZ4 block); a payload below 4 bytes raises."""
    buf = np.frombuffer(bytes(data[:FRAME_BYTES]), np.uint8)
    size = C.c_uint32()
    n = N.lib().rpp_lz4_parse_frame(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(size))
    if n < 0:
        raise RuntimeError("malformed LZ4 block header")
    return int(size.value), int(n)


def host_decode(block: bytes, size: int):
    """``rpp_lz4_host_decode``: (status, the ``size`` output bytes as they stand when decoding ends)."""
    src = np.frombuffer(bytes(block), np.uint8)
    out = np.zeros(max(int(size), 1), np.uint8)
    st = N.lib().rpp_lz4_host_decode(src.ctypes.data_as(C.c_void_p), len(src), out.ctypes.data_as(C.c_void_p), int(size))
    return int(st), out[:size].tobytes()


def check_search(search: int) -> int:
    """The search word ``depth | SEARCH_LAZY`` (depth 1, 2, 4 or 8), or 0: anything else raises ValueError."""
    search = int(search)
    if search != 0 and (search & ~SEARCH_LAZY) not in (1, 2, 4, 8):
        raise ValueError(f"unknown search word: {search}")
    return search


def spec_search(opts: Sequence[str], name: str, other=lambda key, value: False) -> int:
    """The search word of a spec's options ``depth=N`` (1, 2, 4, 8) and ``lazy=0|1`` (lazy alone: depth 1); an
    option that is neither and that ``other(key, value)`` does not take raises ``invalid option(s) for ...``."""
    depth, lazy, bad = 0, 0, []
    for opt in opts:
        key, eq, value = opt.partition("=")
        if key == "depth" and eq and value in ("1", "2", "4", "8"):
            depth = int(value)
        elif key == "lazy" and eq and value in ("0", "1"):
            lazy = int(value)
        elif not (eq and other(key, value)):
            bad.append(opt)
    if bad:
        raise RuntimeError(f"invalid option(s) for {name}: " + ", ".join(bad))
    return (depth or 1) | SEARCH_LAZY if lazy else depth


def host_encode(data: bytes, search: int = 0):
    """``rpp_lz4_host_encode_search``: (the LZ4 block, the ratio flag): the bytes the kernels write, on the
    CPU."""
    src = np.frombuffer(bytes(data), np.uint8)
    cap = bound(len(src))
    out = np.zeros(cap, np.uint8)
    n, flag = C.c_uint64(), C.c_uint32()
    _raise_status(N.lib().rpp_lz4_host_encode_search(src.ctypes.data_as(C.c_void_p), len(src), int(search),
                                                     out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(flag)))
    return out[:n.value].tobytes(), bool(flag.value)


def _layout(sizes: Sequence[int], align: int = 16):
    offs = np.zeros(len(sizes), np.int64)
    at = 0
    for i, n in enumerate(sizes):
        offs[i] = at
        at += (int(n) + align - 1) // align * align
    return offs, at


@dataclass
class EncodedBatch:
    """Device-resident result of :func:`encode_batch` (valid once the stream is synchronised)."""

    data: torch.Tensor       # uint8: block b is data[offsets[b] : offsets[b] + sizes[b]]
    offsets: torch.Tensor    # int64 [n]
    sizes: torch.Tensor      # int64 [n]
    flags: torch.Tensor      # int32 [n]: 1 where 4 + size >= input size
    status: torch.Tensor     # int32 [n]
    source: torch.Tensor     # uint8: the inputs, block b at in_offsets[b]
    in_offsets: torch.Tensor
    in_sizes: torch.Tensor

    def check(self) -> None:
        for st in self.status.cpu().numpy():
            _raise_status(int(st))


def encode_batch(d_in: torch.Tensor, in_offsets, in_sizes: Sequence[int],
                 stream: Optional[torch.cuda.Stream] = None, search: int = 0) -> EncodedBatch:
    """One ``rpp_lz4_encode_batch_search`` over the blocks ``d_in[in_offsets[b] : + in_sizes[b]]`` (a uint8 CUDA
    tensor; host lists of offsets and sizes).  Asynchronous on the stream."""
    dev = d_in.device
    n = len(in_sizes)
    for s in in_sizes:
        if s > MAX_BLOCK:
            raise ValueError(f"an LZ4 block holds at most {MAX_BLOCK} bytes, not {s}")
    out_offs, cap = _layout([bound(s) for s in in_sizes])
    total = int(sum(int(s) for s in in_sizes))
    d_ioff, d_isz, d_ooff = S._i64(in_offsets, dev), S._i64(list(in_sizes), dev), S._i64(out_offs, dev)
    out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ws_bytes = int(N.lib().rpp_lz4_encode_workspace_bytes(total, n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_lz4_encode_batch_search(_ptr(d_in), _ptr(d_ioff), _ptr(d_isz), n, int(search), _ptr(out),
                                                      _ptr(d_ooff), _ptr(sizes), _ptr(flags), _ptr(status), total,
                                                      _ptr(ws), ws_bytes, _stream_ptr(stream)))
    return EncodedBatch(out, d_ooff, sizes, flags, status, d_in, d_ioff, d_isz)


def decode_batch(d_in: torch.Tensor, in_offsets, in_sizes, out_sizes: Sequence[int],
                 stream: Optional[torch.cuda.Stream] = None, out: Optional[torch.Tensor] = None, out_offsets=None):
    """One ``rpp_lz4_decode_batch``: (uint8 output tensor, its int64 offsets on the host, int32 status tensor).
    Asynchronous on the stream."""
    dev = d_in.device
    n = len(out_sizes)
    if out_offsets is None:
        out_offsets, cap = _layout(out_sizes)
    else:
        cap = out.numel()
    if out is None:
        out = torch.zeros(max(cap, 16), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    # (named, so that the four arrays are four allocations until the call has been issued)
    d_ioff, d_isz = S._i64(in_offsets, dev), S._i64(in_sizes, dev)
    d_ooff, d_osz = S._i64(out_offsets, dev), S._i64(list(out_sizes), dev)
    _raise_status(N.lib().rpp_lz4_decode_batch(_ptr(d_in), _ptr(d_ioff), _ptr(d_isz), n, _ptr(out), _ptr(d_ooff),
                                               _ptr(d_osz), _ptr(status), _stream_ptr(stream)))
    return out, np.asarray(out_offsets, np.int64), status


def _upload(blocks: Sequence[bytes], device):
    offs, cap = _layout([len(b) for b in blocks])
    flat = np.zeros(max(cap, 16), np.uint8)
    for o, b in zip(offs, blocks):
        flat[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return torch.from_numpy(flat).to(device), offs


class Lz4BlockCompressor:
    """``lz4_block_compressor`` (src/compression/lz4.cpp:60-117): ``level`` None is ``lz4``, a number
    ``lz4hc:level=N``; the level maps to no search.  ``search`` is the search word (``depth | SEARCH_LAZY``); 0
    writes the bytes of the one-candidate search."""

    def __init__(self, level: Optional[int] = None, device="cuda", search: int = 0):
        if level is not None and not 0 <= int(level) <= 12:
            raise RuntimeError(f"invalid option(s) for lz4hc: level={level}")
        self.level = None if level is None else int(level)
        self.device = torch.device(device)
        self.search = check_search(search)

    def clone(self) -> "Lz4BlockCompressor":
        return Lz4BlockCompressor(self.level, self.device, self.search)

    def type(self) -> int:
        return COMPRESSION_TYPE_LZ4 if self.level is None else COMPRESSION_TYPE_LZ4HC

    def describe(self) -> str:
        return "lz4" if self.level is None else f"lz4hc [level={self.level}]"

    def metadata_requirements(self) -> str:
        return ""

    def get_compression_constraints(self, metadata: Optional[str] = None) -> dict:
        return {}

    def estimate_memory_usage(self, data_size: int) -> int:
        return data_size

    def _encode(self, blocks: Sequence[bytes]) -> EncodedBatch:
        d_in, offs = _upload(blocks, self.device)
        return encode_batch(d_in, offs, [len(b) for b in blocks], search=self.search)

    def compress(self, data: bytes, metadata: Optional[str] = None) -> bytes:
        out = self.compress_many([data], metadata, keep_bad=True)[0]
        if out is None:
            raise BadCompressionRatioError()
        return out

    def compress_many(self, blocks: Sequence[bytes], metadata: Optional[str] = None,
                      keep_bad: bool = False) -> List[Optional[bytes]]:
        """Compresses many blocks in a single launch.  A block that trips the ratio rule raises
        :class:`BadCompressionRatioError`, or with ``keep_bad`` comes back as None."""
        if not blocks:
            return []
        if self.device.type == "cpu":  # the host restatement: the kernels' bytes without a GPU
            streams, flags = zip(*(host_encode(b, self.search) for b in blocks))
        else:
            res = self._encode(blocks)
            torch.cuda.current_stream().synchronize()
            res.check()
            sizes, flags, offs = res.sizes.cpu().numpy(), res.flags.cpu().numpy(), res.offsets.cpu().numpy()
            data = res.data.cpu().numpy()
            streams = [data[o:o + n].tobytes() for o, n in zip(offs, sizes)]
        out: List[Optional[bytes]] = []
        for b, stream, flag in zip(blocks, streams, flags):
            if flag and not keep_bad:
                raise BadCompressionRatioError()
            out.append(None if flag else frame_header(len(b)) + stream)
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
        frames = [b"" if f else frame_header(len(b)) for f, b in zip(flags, blocks)]
        d_fr, d_fl = S._rows(frames, S.FRAME_ROW, self.device)
        headers, i = [], 0
        while i < len(blocks):  # one header launch per run of sections of the same compression type
            j = i
            while j < len(blocks) and flags[j] == flags[i]:
                j += 1
            headers.append(S.section_headers_batch(payload, offs[i:j], lens[i:j], first_number + i, S.SECTION_TYPE_BLOCK,
                                                   COMPRESSION_TYPE_NONE if flags[i] else self.type(), d_fr[i:j],
                                                   d_fl[i:j]))
            i = j
        capacity = int(lens.sum()) + len(blocks) * (S.HEADER_BYTES + FRAME_BYTES)
        asm = S.sections_assemble_batch(torch.cat(headers), payload, offs, lens, capacity, d_fr, d_fl)
        return asm.bytes()


class Lz4BlockDecompressor:
    """``lz4_block_decompressor`` (src/compression/lz4.cpp:119-171)."""

    def __init__(self, data: bytes, device="cuda", compression: int = COMPRESSION_TYPE_LZ4):
        self._size, n = parse_frame(data)
        self.data = bytes(data[n:])
        self.device = torch.device(device)
        self._compression = compression
        self._target: Optional[bytearray] = None
        self._done = False

    def type(self) -> int:
        return self._compression

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
    """lz4.cpp:147-151: a failed decode is a runtime_error that names the decoder's result."""
    if st != N.RPP_OK:
        raise RuntimeError(f"LZ4: decompression failed (error: {st})")


def decompress(data: bytes, device="cuda") -> bytes:
    """``block_decompressor::decompress`` (src/block_decompressor.cpp:41-49)."""
    return decompress_many([Lz4BlockDecompressor(data, device)], device)[0]


def decompress_many(decs: Sequence[Lz4BlockDecompressor], device="cuda") -> List[bytes]:
    """Decodes many LZ4 blocks with one launch."""
    if not decs:
        return []
    dev = torch.device(device)
    sizes = [d.uncompressed_size() for d in decs]
    if dev.type == "cpu":  # the host restatement
        results = [host_decode(d.data, n) for d, n in zip(decs, sizes)]
        for st, _ in results:
            raise_decode_status(st)
        return [out for _, out in results]
    d_in, offs = _upload([d.data for d in decs], dev)
    out, out_offs, status = decode_batch(d_in, offs, [len(d.data) for d in decs], sizes)
    torch.cuda.current_stream().synchronize()
    host = out.cpu().numpy()
    for st in status.cpu().numpy():
        raise_decode_status(int(st))
    return [host[o:o + n].tobytes() for o, n in zip(out_offs, sizes)]
