"""File digests by name over the MI355X kernels: what ``dwarfsck --checksum=ALGO`` and ``mkdwarfs --file-hash=ALGO``
accept beyond the XXH3 hashes.

The reference hands every name but ``xxh3-64`` / ``xxh3-128`` to its crypto library (``checksum_evp``,
src/checksum.cpp:264-280); published checksum lists are written with ``sha256``, ``md5``, ``sha1`` and ``sha512``.
Tensor-level wrappers of the ``rpp_digest_*`` group of ``include/ricepp_amd.h``: thirteen digests computed by the
kernels of csrc/digest/digest_kernels.hip, one lane per file, and the three of :mod:`dwarfs_amd.dedup` forwarded.
Digests are in each standard's byte order (what ``EVP_DigestFinal_ex`` returns), so :func:`hexdigests` prints what
``sha256sum`` and its kin print.  A CPU tensor runs the host definition (``rpp_digest_host``).
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .codec import _raise_status, _stream_ptr
from .dedup import _u8
from .section import _i64, _ptr

# the canonical names, in the order of enum rpp_digest_id
ALGORITHMS = ("md5", "sha1", "sha224", "sha256", "sha384", "sha512", "sha512-224", "sha3-224", "sha3-256", "sha3-384",
              "sha3-512", "blake2b512", "blake2s256", "xxh3-64", "xxh3-128", "sha512-256")


def _algo(name: str) -> Tuple[int, int]:
    """(enum value, digest bytes) of an algorithm name (OpenSSL's names in any letter case, the XXH3 names
    exactly); ValueError for an unknown one."""
    L = N.lib()
    a = L.rpp_digest_algo(str(name).encode())
    if a < 0:
        raise ValueError(f"unknown digest algorithm {name!r} (known: {', '.join(ALGORITHMS)})")
    return a, L.rpp_digest_bytes(a)


def digest_bytes(algo: str) -> int:
    return _algo(algo)[1]


def digest_batch(data: torch.Tensor, offsets, sizes, algo: str, select=None,
                 stream: Optional[torch.cuda.Stream] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Digests (uint8 tensor [n, digest bytes] on ``data``'s device) of the files
    ``data[offsets[b] : offsets[b] + sizes[b]]``, as ``dedup.file_hash_batch``.  With ``select`` (n bytes), a file
    whose byte is 0 is not read and its row of ``out`` is left as it is (a fresh ``out`` is zero-filled).  A CPU
    ``data`` runs ``rpp_digest_host``, which has no XXH3."""
    a, nbytes = _algo(algo)
    dev = data.device
    if data.dtype != torch.uint8 or not data.is_contiguous():
        raise ValueError("data must be a contiguous uint8 tensor")
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    n = d_sz.numel()
    if d_off.numel() != n:
        raise ValueError("offsets and sizes need one entry per file")
    d_sel = _u8(select, dev)
    if d_sel is not None and d_sel.numel() != n:
        raise ValueError("select needs one byte per file")
    if out is None:
        out = torch.zeros((n, nbytes), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.numel() != n * nbytes or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous uint8 tensor of {n} x {nbytes} bytes on {dev}")
    L = N.lib()
    if dev.type == "cpu":
        if algo in ("xxh3-64", "xxh3-128"):
            raise ValueError(f"{algo} has no host definition: it needs a GPU device")
        _raise_status(L.rpp_digest_host(a, _ptr(data), _ptr(d_off), _ptr(d_sz), _ptr(d_sel), n, _ptr(out)))
    else:
        _raise_status(L.rpp_digest_batch(a, _ptr(data), _ptr(d_off), _ptr(d_sz), _ptr(d_sel), n, _ptr(out),
                                         _stream_ptr(stream)))
    return out


def hexdigests(digests: torch.Tensor) -> List[str]:
    """One lower-case hex string per row, as the checksum tools print them."""
    return [row.tobytes().hex() for row in np.atleast_2d(digests.cpu().numpy())]
