"""DwarFS section headers and checksums over the MI355X kernels.

Tensor-level wrappers of the section group of ``include/ricepp_amd.h``: the
writer's two checksums per block (``fsblock::build_section_header``,
src/writer/filesystem_writer.cpp:606-651 -- XXH3-64 over header[48,64) + data,
then SHA-512/256 over header[40,64) + data), the 64-byte ``section_header_v2``
(include/dwarfs/fstypes.h:85-97), the byte-packed image fragment, and the
reader's checks (``fs_section_v2::check_fast``, src/internal/fs_section.cpp:226-259;
``fs_section_checker::verify``).  Everything stays on the device and on the
caller's stream; only ``parse_header`` / ``walk`` are host code.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .codec import _raise_status, _stream_ptr

HEADER_BYTES = 64
FRAME_ROW = 32
PREFIX_ROW = 64
SECTION_TYPE_BLOCK = 0  # section_type::BLOCK (include/dwarfs/fstypes.h:50-65)

INTEGRITY_ERROR = "block data integrity check failed"  # src/reader/internal/cached_block.cpp:58-67


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _i64(values, device) -> torch.Tensor:
    if isinstance(values, torch.Tensor):
        return values.to(device=device, dtype=torch.int64).contiguous()
    return torch.as_tensor(np.asarray(values, dtype=np.int64), device=device)


def _rows(rows: Optional[Sequence[bytes]], width: int, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """A list of byte strings (each <= width) as a device array of `width`-byte rows plus an int32 length array."""
    if rows is None:
        return None, None
    buf = np.zeros((max(len(rows), 1), width), np.uint8)
    lens = np.zeros(max(len(rows), 1), np.int32)
    for i, r in enumerate(rows):
        if len(r) > width:
            raise ValueError(f"row {i} holds {len(r)} bytes, more than {width}")
        buf[i, :len(r)] = np.frombuffer(r, np.uint8)
        lens[i] = len(r)
    return torch.from_numpy(buf).to(device), torch.from_numpy(lens).to(device)


def _prefix_args(prefix, prefix_len, device):
    if prefix is None:
        return None, None
    if isinstance(prefix, torch.Tensor):
        if prefix_len is None:
            raise ValueError("a prefix tensor needs prefix_len")
        return prefix.contiguous(), prefix_len.to(device=device, dtype=torch.int32).contiguous()
    return _rows(prefix, PREFIX_ROW, device)


def xxh3_64_batch(data: torch.Tensor, offsets, sizes, prefix=None, prefix_len=None,
                  stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """XXH3-64 (seed 0) of the messages ``prefix[b] + data[offsets[b] : offsets[b] + sizes[b]]``.

    ``data`` is a uint8 CUDA tensor; ``prefix`` a list of byte strings of at most 64 bytes each (or a device
    tensor of 64-byte rows with ``prefix_len``).  Returns an int64 device tensor holding the 64-bit values."""
    dev = data.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_pre, d_plen = _prefix_args(prefix, prefix_len, dev)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    _raise_status(N.lib().rpp_xxh3_64_batch(_ptr(data), _ptr(d_off), _ptr(d_sz), n, _ptr(d_pre), _ptr(d_plen),
                                            _ptr(out), _stream_ptr(stream)))
    return out


def xxh3_128_batch(data: torch.Tensor, offsets, sizes, prefix=None, prefix_len=None,
                   stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """XXH3-128 (seed 0) of the same messages as :func:`xxh3_64_batch`: a uint8 device tensor [n, 16] in
    DwarFS's digest order (low64 little endian, then high64 little endian)."""
    dev = data.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_pre, d_plen = _prefix_args(prefix, prefix_len, dev)
    out = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_xxh3_128_batch(_ptr(data), _ptr(d_off), _ptr(d_sz), n, _ptr(d_pre), _ptr(d_plen),
                                             _ptr(out), _stream_ptr(stream)))
    return out


def sha512_256_batch(data: torch.Tensor, offsets, sizes, prefix=None, prefix_len=None,
                     stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """SHA-512/256 of the same messages as :func:`xxh3_64_batch`: a uint8 device tensor [n, 32]."""
    dev = data.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_pre, d_plen = _prefix_args(prefix, prefix_len, dev)
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_sha512_256_batch(_ptr(data), _ptr(d_off), _ptr(d_sz), n, _ptr(d_pre), _ptr(d_plen),
                                               _ptr(out), _stream_ptr(stream)))
    return out


def _frame_args(frames, frame_len, device):
    if frames is None:
        return None, None
    if isinstance(frames, torch.Tensor):
        if frame_len is None:
            raise ValueError("a frame tensor needs frame_len")
        return frames.contiguous(), frame_len.to(device=device, dtype=torch.int32).contiguous()
    return _rows(frames, FRAME_ROW, device)


def section_headers_batch(payload: torch.Tensor, offsets, sizes, first_number: int, section_type: int,
                          compression: int, frames=None, frame_len=None,
                          stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Complete v2 headers (uint8 device tensor [n, 64]) of the sections ``frames[b] + payload[offsets[b] :
    offsets[b] + sizes[b]]``, numbered from ``first_number``."""
    dev = payload.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_fr, d_fl = _frame_args(frames, frame_len, dev)
    out = torch.empty((n, HEADER_BYTES), dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_section_headers_batch(_ptr(payload), _ptr(d_off), _ptr(d_sz), n, int(first_number),
                                                    int(section_type), int(compression), _ptr(d_fr), _ptr(d_fl),
                                                    _ptr(out), _stream_ptr(stream)))
    return out


@dataclass
class AssembledSections:
    """Device-resident result of :func:`sections_assemble_batch`."""

    image: torch.Tensor     # uint8, the fragment is image[:total]
    offsets: torch.Tensor   # int64 [n] start of section b's header
    sizes: torch.Tensor     # int64 [n] header + frame + payload bytes
    total: torch.Tensor     # int64 [1]

    def bytes(self) -> bytes:
        """The fragment on the host (synchronises the current stream)."""
        n = int(self.total.item())
        return self.image[:n].cpu().numpy().tobytes()


def sections_assemble_batch(headers: torch.Tensor, payload: torch.Tensor, offsets, sizes, capacity: int, frames=None,
                            frame_len=None, stream: Optional[torch.cuda.Stream] = None,
                            image: Optional[torch.Tensor] = None) -> AssembledSections:
    """Header, frame and payload of every section back to back, byte-packed, in one device buffer of
    ``capacity`` bytes (at least the sum of 64 + frame + payload sizes; or the caller's ``image``)."""
    dev = payload.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_fr, d_fl = _frame_args(frames, frame_len, dev)
    if image is None:
        image = torch.empty(max(int(capacity), 16), dtype=torch.uint8, device=dev)
    sec_sizes = torch.empty(n, dtype=torch.int64, device=dev)
    sec_offs = torch.empty(n, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _raise_status(N.lib().rpp_sections_assemble_batch(_ptr(headers), _ptr(d_fr), _ptr(d_fl), _ptr(payload),
                                                      _ptr(d_off), _ptr(d_sz), n, _ptr(image), _ptr(sec_sizes),
                                                      _ptr(sec_offs), _ptr(total), _stream_ptr(stream)))
    return AssembledSections(image, sec_offs, sec_sizes, total)


def sections_verify_batch(image: torch.Tensor, image_bytes: int, section_offsets, level: int = 1,
                          stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Per-section status (int32 device tensor) of the sections whose headers start at ``section_offsets`` of
    the device image: RPP_OK, RPP_CHECKSUM_MISMATCH, RPP_INVALID_ARGUMENT (magic / major version) or
    RPP_TRUNCATED_INPUT.  ``level`` 1 checks XXH3-64, 2 also SHA-512/256."""
    dev = image.device
    d_off = _i64(section_offsets, dev)
    n = d_off.numel()
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _raise_status(N.lib().rpp_sections_verify_batch(_ptr(image), int(image_bytes), _ptr(d_off), n, int(level),
                                                    _ptr(status), _stream_ptr(stream)))
    return status


def parse_header(data: bytes) -> N.RppSectionHeader:
    """``rpp_parse_section_header`` of the first 64 bytes of ``data``; ValueError for a short buffer, a wrong
    magic or another major version."""
    if len(data) < HEADER_BYTES:
        raise ValueError("section header needs 64 bytes")
    buf = (C.c_uint8 * HEADER_BYTES).from_buffer_copy(bytes(data[:HEADER_BYTES]))
    h = N.RppSectionHeader()
    if N.lib().rpp_parse_section_header(buf, C.byref(h)) != N.RPP_OK:
        raise ValueError("not a DwarFS v2 section header")
    return h


def walk(image: bytes) -> Tuple[List[Tuple[int, N.RppSectionHeader]], Optional[int]]:
    """The sections of an image from offset 0: ``[(offset, header)]`` of those that lie inside it, and the
    offset of a trailing header that does not parse or runs past the end (None if the walk ends cleanly)."""
    out, at = [], 0
    while at < len(image):
        try:
            h = parse_header(image[at:at + HEADER_BYTES])
        except ValueError:
            return out, at
        if h.length > len(image) - at - HEADER_BYTES:
            return out, at
        out.append((at, h))
        at += HEADER_BYTES + int(h.length)
    return out, None
