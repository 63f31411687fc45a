"""ctypes wrapper around oracle/_ref/libdwarfs_ref.so: the reference itself (its ricepp codec and its nilsimsa,
similarity and rsync hashes), compiled unmodified by oracle/ref_build.py behind oracle/ref_driver.cpp.

TEST INFRASTRUCTURE ONLY, with the call shapes of oracle/oracle.py.  This module never reads the reference tree:
it loads the library that the recipe left under oracle/_ref/ (which travels with the working tree but is not in
git).  ``available()`` says whether there is one; ``lib()`` raises ``ReferenceUnavailable`` otherwise.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import ref_build
from .oracle import (INVALID_ARGUMENT, OK, OUTPUT_TOO_SMALL, TRUNCATED_INPUT, UNSUPPORTED_CONFIG, Config,  # noqa: F401
                     OracleError, cfg)

LIB_PATH = ref_build.LIB_PATH
EXCEPTION = -5


class ReferenceUnavailable(RuntimeError):
    pass


class ReferenceError_(OracleError):
    """A status of the driver (the codes of oracle.py; -5: another exception of the reference)."""


_lib = None


def available() -> bool:
    """True if the library is there or can be built (the recipe is a no-op without the reference tree)."""
    return ref_build.build() is not None


def lib():
    global _lib
    if _lib is None:
        path = ref_build.build()
        if path is None:
            raise ReferenceUnavailable(f"{LIB_PATH} is absent and so is the reference tree to build it from")
        L = C.CDLL(str(path))
        P, Z = C.c_void_p, C.c_size_t
        L.ref_build_flags.restype = C.c_char_p
        L.ref_ricepp_worst_case_bytes.argtypes = [C.POINTER(Config), Z, C.POINTER(Z)]
        L.ref_ricepp_encode.argtypes = [C.POINTER(Config), P, Z, P, Z, C.POINTER(Z)]
        L.ref_ricepp_decode.argtypes = [C.POINTER(Config), P, Z, P, Z]
        L.ref_nilsimsa.argtypes = [P, P, Z, P]
        L.ref_similarity.argtypes = [P, P, Z, C.POINTER(C.c_uint32)]
        L.ref_rsync_hashes.argtypes = [P, Z, Z, Z, P, Z, C.POINTER(Z)]
        L.ref_rsync_repeating_window.argtypes = [C.c_uint8, Z]
        L.ref_rsync_repeating_window.restype = C.c_uint32
        _lib = L
    return _lib


def build_flags() -> str:
    return lib().ref_build_flags().decode()


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _raise(st: int) -> None:
    if st:
        raise ReferenceError_(st)


# ---- ricepp ----

def worst_case_bytes(c: Config, n: int) -> int:
    out = C.c_size_t(0)
    _raise(lib().ref_ricepp_worst_case_bytes(C.byref(c), n, C.byref(out)))
    return out.value


def encode(c: Config, samples: np.ndarray) -> bytes:
    samples = np.ascontiguousarray(samples, dtype=np.uint16)
    cap = 2 * samples.size + samples.size // max(c.block_size, 1) + 128
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t(0)
    _raise(lib().ref_ricepp_encode(C.byref(c), _p(samples), samples.size, _p(out), cap, C.byref(n)))
    return out[: n.value].tobytes()


def decode(c: Config, data: bytes, n_samples: int) -> np.ndarray:
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = np.zeros(max(n_samples, 1), np.uint16)
    _raise(lib().ref_ricepp_decode(C.byref(c), _p(buf), len(data), _p(out), n_samples))
    return out[:n_samples]


# ---- hashes ----

def _pieces(data: bytes, sizes: Optional[Sequence[int]]):
    sizes = np.asarray([len(data)] if sizes is None else list(sizes), dtype=np.uint64)
    if int(sizes.sum()) != len(data):
        raise ValueError("update sizes must add up to the length of the data")
    return np.frombuffer(bytes(data) or b"\0", np.uint8), sizes


def nilsimsa(data: bytes, sizes: Optional[Sequence[int]] = None) -> bytes:
    """The 32 digest bytes (bit i at byte i // 8, bit i % 8); ``sizes``: one update per piece instead of one."""
    buf, sz = _pieces(data, sizes)
    out = np.zeros(32, np.uint8)
    _raise(lib().ref_nilsimsa(_p(buf), _p(sz), sz.size, _p(out)))
    return out.tobytes()


def similarity(data: bytes, sizes: Optional[Sequence[int]] = None) -> int:
    buf, sz = _pieces(data, sizes)
    out = C.c_uint32(0)
    _raise(lib().ref_similarity(_p(buf), _p(sz), sz.size, C.byref(out)))
    return out.value


def similarity_digest(data: bytes, sizes: Optional[Sequence[int]] = None) -> bytes:
    """The 32-bit value as the four little-endian bytes the product's digests hold."""
    return similarity(data, sizes).to_bytes(4, "little")


def rsync_hashes(data: bytes, window_bytes: int, granularity: int) -> np.ndarray:
    """rsync_hash driven as the segmenter drives it over ``data`` cut to whole frames: the value of every window
    that starts at a multiple of ``granularity`` bytes."""
    n = len(data) // granularity * granularity
    buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
    cap = max(0, (n - window_bytes) // granularity + 1)
    out = np.zeros(max(cap, 1), np.uint32)
    count = C.c_size_t(0)
    _raise(lib().ref_rsync_hashes(_p(buf), n, window_bytes, granularity, _p(out), cap, C.byref(count)))
    assert count.value == cap
    return out[:cap]


def repeating_window(byte: int, length: int) -> int:
    return int(lib().ref_rsync_repeating_window(byte, length))
