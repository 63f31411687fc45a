"""Similarity hashes of the inode scan over the MI355X kernels.

For every unique file the reference computes a similarity hash that the fragment orderer sorts or clusters by
(``inode_::scan_full`` / ``scan_fragments`` / ``scan_range``, src/writer/internal/inode_manager.cpp:399-537):
``nilsimsa``, a 256-bit locality-sensitive digest (the default of ``--order``), or ``similarity``, 32 bits made of
the four most frequent buckets of a 4-byte rolling hash.  Tensor-level wrappers of the similarity group of
``include/ricepp_amd.h``.  Both hashes are histograms, so a state can be fed by several calls and a message is
cut into chunks that run on different workgroups; the states are the same bytes on the host and on the device.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .codec import _raise_status, _stream_ptr
from .dedup import _u8
from .section import _i64, _ptr

KINDS = ("nilsimsa", "similarity")


def _kind(name: str) -> Tuple[int, int, int]:
    """(enum value, digest bytes, state bytes) of a kind name; ValueError for an unknown one."""
    L = N.lib()
    k = L.rpp_similarity_kind(str(name).encode())
    if k < 0:
        raise ValueError(f"unknown similarity hash {name!r} (known: {', '.join(KINDS)})")
    return k, L.rpp_similarity_digest_bytes(k), L.rpp_similarity_state_bytes(k)


def chunk_bytes() -> int:
    """The bytes of a message that one workgroup accumulates (``rpp_similarity_chunk_bytes``)."""
    return int(N.lib().rpp_similarity_chunk_bytes())


def hexdigest(digest, kind: str = "nilsimsa") -> str:
    """A digest as the reference's tests print it: the bytes reversed, as hex (for ``similarity`` the 32-bit
    value as 8 hex digits)."""
    return bytes(np.asarray(digest, dtype=np.uint8).tobytes())[::-1].hex()


@dataclass
class SimilarityState:
    """n hash states on the device (uint8 tensor [n, state bytes]) and their kind; zero-filled = initial."""

    kind: str
    states: torch.Tensor

    @classmethod
    def new(cls, n: int, kind: str = "nilsimsa", device="cuda") -> "SimilarityState":
        _, _, sbytes = _kind(kind)
        return cls(kind, torch.zeros((int(n), sbytes), dtype=torch.uint8, device=device))

    @classmethod
    def from_host(cls, states: np.ndarray, kind: str, device="cuda") -> "SimilarityState":
        """Uploads host states (uint8 [n, state bytes], e.g. of :class:`HostState`)."""
        _, _, sbytes = _kind(kind)
        arr = np.ascontiguousarray(states, dtype=np.uint8).reshape(-1, sbytes)
        return cls(kind, torch.from_numpy(arr.copy()).to(device))

    def __len__(self) -> int:
        return self.states.shape[0]

    def reset(self) -> None:
        self.states.zero_()

    def cpu(self) -> np.ndarray:
        """The raw states on the host (synchronises)."""
        return self.states.cpu().numpy()


def update(state: SimilarityState, data: torch.Tensor, offsets, sizes, select=None,
           stream: Optional[torch.cuda.Stream] = None) -> SimilarityState:
    """Feeds ``data[offsets[b] : offsets[b] + sizes[b]]`` into state b (``rpp_similarity_update_batch``);
    successive calls hash the concatenation of their spans.  States with ``select[b] == 0`` are left untouched."""
    k, _, _ = _kind(state.kind)
    dev = state.states.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    if n != len(state) or d_off.numel() != n:
        raise ValueError("update needs one offset and one size per state")
    d_sel = _u8(select, dev)
    if d_sel is not None and d_sel.numel() != n:
        raise ValueError("select needs one byte per state")
    _raise_status(N.lib().rpp_similarity_update_batch(k, _ptr(data), _ptr(d_off), _ptr(d_sz), _ptr(d_sel), n,
                                                      _ptr(state.states), _stream_ptr(stream)))
    return state


def finalize(state: SimilarityState, select=None, stream: Optional[torch.cuda.Stream] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Digests (uint8 device tensor [n, digest bytes]) of the states, which are left unchanged; rows with
    ``select[b] == 0`` are not written (a fresh ``out`` is zero-filled)."""
    k, nbytes, _ = _kind(state.kind)
    dev = state.states.device
    n = len(state)
    d_sel = _u8(select, dev)
    if d_sel is not None and d_sel.numel() != n:
        raise ValueError("select needs one byte per state")
    if out is None:
        out = torch.zeros((n, nbytes), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.numel() != n * nbytes or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of {n} x {nbytes} bytes")
    _raise_status(N.lib().rpp_similarity_finalize_batch(k, _ptr(state.states), _ptr(d_sel), n, _ptr(out),
                                                        _stream_ptr(stream)))
    return out


@dataclass
class DeviceSimilarity:
    """Reusable buffers of :func:`similarity_hash_batch` for n files of one kind (graph capture)."""

    kind: str
    digests: torch.Tensor    # uint8 [n, digest bytes]; rows of files that were not hashed are left as they were
    has: torch.Tensor        # uint8 [n]: 1 if the file was hashed
    workspace: torch.Tensor

    @classmethod
    def new(cls, n: int, kind: str = "nilsimsa", device="cuda") -> "DeviceSimilarity":
        k, nbytes, _ = _kind(kind)
        ws_bytes = N.lib().rpp_similarity_hash_workspace_bytes(k, int(n))
        return cls(kind, torch.zeros((int(n), nbytes), dtype=torch.uint8, device=device),
                   torch.zeros(int(n), dtype=torch.uint8, device=device),
                   torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=device))


def similarity_hash_batch(data: torch.Tensor, offsets, sizes, kind: str = "nilsimsa", max_size: Optional[int] = None,
                          select=None, stream: Optional[torch.cuda.Stream] = None,
                          out: Optional[DeviceSimilarity] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``scan_full`` for files already on the device (``rpp_similarity_hash_batch``): returns ``(digests, has)``,
    uint8 device tensors [n, digest bytes] and [n].  A file with ``select[b] == 0`` or larger than ``max_size``
    gets ``has[b] = 0`` and keeps its digest row (zero in fresh buffers).  Asynchronous on the stream, no host
    round trip, graph-capturable when ``offsets`` / ``sizes`` / ``select`` are device tensors of their final
    dtype and ``out`` (:meth:`DeviceSimilarity.new`) provides the buffers."""
    k, _, _ = _kind(kind)
    dev = data.device
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    d_sel = _u8(select, dev)
    if d_sel is not None and d_sel.numel() != n:
        raise ValueError("select needs one byte per file")
    L = N.lib()
    ws_bytes = L.rpp_similarity_hash_workspace_bytes(k, n)
    if out is None:
        out = DeviceSimilarity.new(n, kind, dev)
    elif out.kind != kind or out.has.numel() != n or out.workspace.numel() < ws_bytes:
        raise ValueError("out was made for another kind or file count")
    _raise_status(L.rpp_similarity_hash_batch(k, _ptr(data), _ptr(d_off), _ptr(d_sz), _ptr(d_sel),
                                              int(max_size or 0), n, _ptr(out.digests), _ptr(out.has),
                                              _ptr(out.workspace), ws_bytes, _stream_ptr(stream)))
    return out.digests, out.has


@dataclass
class SimilarityHashes:
    """Digests on the host."""

    kind: str
    digests: np.ndarray  # uint8 [n, digest bytes]
    has: np.ndarray      # uint8 [n]

    def hexdigest(self, i: int) -> Optional[str]:
        """File i's digest as the reference prints it, or None for a file that was not hashed."""
        return hexdigest(self.digests[i], self.kind) if self.has[i] else None

    def value(self, i: int) -> Optional[int]:
        """The 32-bit value of a ``similarity`` digest."""
        return int.from_bytes(self.digests[i].tobytes(), "little") if self.has[i] else None


def pack_files(files: Sequence[bytes], align: int = 16) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(bytes, offsets, sizes) of ``files`` laid out at multiples of ``align``."""
    sizes = np.array([len(f) for f in files], dtype=np.int64)
    offsets = np.zeros(len(files), dtype=np.int64)
    if len(files):
        offsets[1:] = np.cumsum((sizes[:-1] + align - 1) // align * align)
    total = int(offsets[-1] + sizes[-1]) if len(files) else 0
    host = np.zeros(max(total, 16), dtype=np.uint8)
    for o, f in zip(offsets, files):
        host[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return host, offsets, sizes


def similarity_hashes(files: Sequence[bytes], kind: str = "nilsimsa", max_size: Optional[int] = None,
                      device="cuda") -> SimilarityHashes:
    """The hash of every file: one upload, ``rpp_similarity_hash_batch``, one download."""
    _kind(kind)
    host, offsets, sizes = pack_files(files)
    data = torch.from_numpy(host).to(device)
    digests, has = similarity_hash_batch(data, offsets, sizes, kind, max_size)
    return SimilarityHashes(kind, digests.cpu().numpy(), has.cpu().numpy())


class HostState:
    """One state on the host, over ``rpp_similarity_host_update`` / ``_finalize`` (no GPU)."""

    def __init__(self, kind: str = "nilsimsa", raw: Optional[bytes] = None):
        self.kind = kind
        self._k, self._dbytes, sbytes = _kind(kind)
        self._buf = (C.c_uint8 * sbytes)()
        if raw is not None:
            if len(raw) != sbytes:
                raise ValueError(f"a {kind} state has {sbytes} bytes")
            C.memmove(self._buf, bytes(raw), sbytes)

    def update(self, data: bytes) -> "HostState":
        data = bytes(data)
        src = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        _raise_status(N.lib().rpp_similarity_host_update(self._k, C.cast(self._buf, C.c_void_p),
                                                         C.cast(src, C.c_void_p), len(data)))
        return self

    def raw(self) -> bytes:
        return bytes(self._buf)

    def digest(self) -> bytes:
        out = (C.c_uint8 * self._dbytes)()
        _raise_status(N.lib().rpp_similarity_host_finalize(self._k, C.cast(self._buf, C.c_void_p),
                                                           C.cast(out, C.c_void_p)))
        return bytes(out)

    def hexdigest(self) -> str:
        return hexdigest(np.frombuffer(self.digest(), np.uint8), self.kind)


def host_hash(data: bytes, kind: str = "nilsimsa") -> bytes:
    """The digest of ``data`` computed on the host."""
    return HostState(kind).update(data).digest()


def host_hashes(files: Sequence[bytes], kind: str = "nilsimsa") -> List[bytes]:
    return [host_hash(f, kind) for f in files]
