"""Duplicate-file detection over the MI355X kernels.

The scanner's first per-byte pass (``file_scanner_::scan_dedupe``, src/writer/internal/file_scanner.cpp:274-413):
every file that shares its (size, start hash) with another file is hashed with the ``--file-hash`` algorithm
(default ``xxh3-128``, tools/src/mkdwarfs_main.cpp:593-594), and files with equal hashes share the inode of the
one scanned first.  Tensor-level wrappers of the dedup group of ``include/ricepp_amd.h``; digests are in
DwarFS's byte order (``checksum_xxh3::finalize``, src/checksum.cpp:185-196).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .codec import _raise_status, _stream_ptr
from .section import _i64, _ptr

ALGORITHMS = ("xxh3-64", "xxh3-128", "sha512-256")
LARGE_FILE_THRESHOLD = 1024 * 1024  # kLargeFileThreshold (file_scanner.cpp:59)
LARGE_FILE_START_HASH_SIZE = 4096   # kLargeFileStartHashSize (file_scanner.cpp:60)


def _algo(name: str) -> Tuple[int, int]:
    """(enum value, digest bytes) of an algorithm name; ValueError for an unknown one."""
    L = N.lib()
    a = L.rpp_file_hash_algo(str(name).encode())
    if a < 0:
        raise ValueError(f"unknown file hash algorithm {name!r} (known: {', '.join(ALGORITHMS)})")
    return a, L.rpp_file_hash_digest_bytes(a)


def _u8(values, device) -> Optional[torch.Tensor]:
    if values is None:
        return None
    if isinstance(values, torch.Tensor):
        return values.to(device=device, dtype=torch.uint8).contiguous()
    return torch.as_tensor(np.asarray(values, dtype=np.uint8), device=device)


def file_hash_batch(data: torch.Tensor, offsets, sizes, algo: str = "xxh3-128", select=None,
                    stream: Optional[torch.cuda.Stream] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Digests (uint8 device tensor [n, digest bytes]) of the files ``data[offsets[b] : offsets[b] + sizes[b]]``.
    With ``select`` (n bytes), a file whose byte is 0 is not read and its row of ``out`` is left as it is
    (a fresh ``out`` is zero-filled)."""
    a, nbytes = _algo(algo)
    dev = data.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_sel = _u8(select, dev)
    if d_sel is not None and d_sel.numel() != n:
        raise ValueError("select needs one byte per file")
    if out is None:
        out = torch.zeros((n, nbytes), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.numel() != n * nbytes or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of {n} x {nbytes} bytes")
    _raise_status(N.lib().rpp_file_hash_batch(a, _ptr(data), _ptr(d_off), _ptr(d_sz), _ptr(d_sel), n, _ptr(out),
                                              _stream_ptr(stream)))
    return out


def group_first(sizes, digests: Optional[torch.Tensor] = None, select=None,
                stream: Optional[torch.cuda.Stream] = None, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """Groups the keys (sizes[b], digests[b]): returns ``(first, multi)``, int32 and uint8 device tensors --
    first[b] is the smallest index whose key equals key b, multi[b] is 1 if key b occurs more than once.
    ``digests`` is a uint8 device tensor [n, 8 | 16 | 32] or None (the size alone); keys with
    ``select[b] == 0`` take no part (first[b] = b, multi[b] = 0)."""
    dev = digests.device if digests is not None else torch.device(device)
    d_sz = _i64(sizes, dev)
    n = d_sz.numel()
    width = 0
    if digests is not None:
        digests = digests.contiguous()
        width = digests.numel() // n if n else 0
        if digests.dtype != torch.uint8 or digests.numel() != n * width or width not in (0, 8, 16, 32):
            raise ValueError("digests must be uint8 rows of 8, 16 or 32 bytes, one per key")
    d_sel = _u8(select, dev)
    if d_sel is not None and d_sel.numel() != n:
        raise ValueError("select needs one byte per key")
    L = N.lib()
    ws_bytes = L.rpp_group_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    multi = torch.empty(n, dtype=torch.uint8, device=dev)
    _raise_status(L.rpp_group_first_batch(_ptr(d_sz), _ptr(digests if width else None), width, _ptr(d_sel), n,
                                          _ptr(first), _ptr(multi), _ptr(ws), ws_bytes, _stream_ptr(stream)))
    return first, multi


def group_start_slot(size: int, digest: bytes = b"", n: int = 1) -> int:
    """Test hook: the slot at which the probe sequence of the key (size, digest) starts in the table that
    :func:`group_first` uses for ``n`` keys (``rpp_group_workspace_bytes(n) / 4`` slots)."""
    buf = (C.c_uint8 * max(len(digest), 1)).from_buffer_copy(bytes(digest) or b"\0")
    return int(N.lib().rpp_group_start_slot(int(size), buf, len(digest), int(n)))


@dataclass
class DeviceDuplicates:
    """Device-resident result of :func:`find_duplicates_device` (valid once the stream has run)."""

    algo: str
    first: torch.Tensor      # int32 [n]: the first file with file b's (size, digest); b if not hashed
    hashed: torch.Tensor     # uint8 [n]: 1 if the file was hashed
    digests: torch.Tensor    # uint8 [n, digest bytes]; rows of files that were not hashed are left as they were
    workspace: torch.Tensor

    def cpu(self) -> "Duplicates":
        """The result on the host (synchronises)."""
        return Duplicates(self.algo, self.first.cpu().numpy(), self.hashed.cpu().numpy(),
                          self.digests.cpu().numpy())


@dataclass
class Duplicates:
    """The scanner's decision on the host."""

    algo: str
    first: np.ndarray    # int32 [n]
    hashed: np.ndarray   # uint8 [n]
    digests: np.ndarray  # uint8 [n, digest bytes]

    def hexdigest(self, i: int) -> Optional[str]:
        """File i's digest as DwarFS prints it, or None for a file that was not hashed."""
        return self.digests[i].tobytes().hex() if self.hashed[i] else None


def find_duplicates_device(data: torch.Tensor, offsets, sizes, algo: str = "xxh3-128",
                           stream: Optional[torch.cuda.Stream] = None,
                           out: Optional[DeviceDuplicates] = None) -> DeviceDuplicates:
    """The scanner's decision for files already on the device (``rpp_file_dedup_batch``): asynchronous on the
    stream, no host round trip, graph-capturable when ``offsets`` / ``sizes`` are int64 device tensors and
    ``out`` (an earlier result for as many files and the same algorithm) provides the buffers."""
    a, nbytes = _algo(algo)
    dev = data.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    L = N.lib()
    ws_bytes = L.rpp_file_dedup_workspace_bytes(n)
    if out is None:
        out = DeviceDuplicates(algo, torch.empty(n, dtype=torch.int32, device=dev),
                               torch.empty(n, dtype=torch.uint8, device=dev),
                               torch.zeros((n, nbytes), dtype=torch.uint8, device=dev),
                               torch.empty(ws_bytes, dtype=torch.uint8, device=dev))
    elif out.algo != algo or out.first.numel() != n or out.workspace.numel() < ws_bytes:
        raise ValueError("out was made for another algorithm or file count")
    _raise_status(L.rpp_file_dedup_batch(a, _ptr(data), _ptr(d_off), _ptr(d_sz), n, _ptr(out.digests),
                                         _ptr(out.first), _ptr(out.hashed), _ptr(out.workspace), ws_bytes,
                                         _stream_ptr(stream)))
    return out


def find_duplicates(files: Sequence[bytes], algo: str = "xxh3-128", device="cuda") -> Duplicates:
    """The scanner's decision for ``files`` in scan order: one upload, ``rpp_file_dedup_batch``, one download."""
    _algo(algo)
    sizes = np.array([len(f) for f in files], dtype=np.int64)
    offsets = np.zeros(len(files), dtype=np.int64)
    if len(files):
        offsets[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    total = int(offsets[-1] + sizes[-1]) if len(files) else 0
    host = np.zeros(max(total, 16), dtype=np.uint8)
    for o, f in zip(offsets, files):
        host[o:o + len(f)] = np.frombuffer(f, np.uint8)
    data = torch.from_numpy(host).to(device)
    return find_duplicates_device(data, offsets, sizes, algo).cpu()


def scanner_model(files: Sequence[bytes]) -> Tuple[List[int], List[int]]:
    """``(first, hashed)`` as the reference's scanner decides them, computed from the bytes alone: a file is
    hashed exactly when another file shares its unique key -- its size and, from 1 MiB on, its first 4 KiB
    (which stand for their start hash) -- and hashed files with equal bytes share the first one's inode."""
    def key(f):
        return len(f), (bytes(f[:LARGE_FILE_START_HASH_SIZE]) if len(f) >= LARGE_FILE_THRESHOLD else b"")

    count = {}
    for f in files:
        count[key(f)] = count.get(key(f), 0) + 1
    hashed = [1 if count[key(f)] > 1 else 0 for f in files]
    seen, first = {}, []
    for i, f in enumerate(files):
        first.append(seen.setdefault(bytes(f), i) if hashed[i] else i)
    return first, hashed
