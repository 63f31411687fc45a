"""mkdwarfs's ``incompressible`` categorizer over the MI355X kernels (Python mirror).

Mirrors ``incompressible_categorizer_`` (src/writer/categorizer/incompressible_categorizer.cpp): every
``block_size`` piece of every file is compressed with a fast encoder, and a piece whose compressed size is at
least ``max_ratio`` times its own size is ``incompressible`` and is kept from the compressors later on.  The
complete definition is at the top of csrc/scan/incompressible_host.cpp; in one line: a piece's size is the size of
the one frame this project's Zstandard encoder (zstd.py) writes for it under ``options`` and ``search``, and the
verdict is ``float(size) >= max_ratio * float(n)``.  The size is **not** libzstd's: ``--incompressible-zstd-level``
has no counterpart, ``options`` and ``search`` take its place, and (0, 0), the default, is the fastest path.  The
encoder's match window is 64 KiB, so data whose only redundancy lies further back reads as incompressible.

The kernels give the raw numbers (:func:`scan_pieces`): per piece size and verdict, per extent the totals and, with
``generate_fragments``, the run-length rows.  What becomes of them is restated here from the reference:
``get_fragments`` (:109-140: an empty list becomes one fragment of the extent's size, which is incompressible iff
``total_out >= max_ratio * total_in`` and is kept only when forced or not the default), the job's ``add_hole``
(:234-240: flush with force, a default fragment of the hole's size, reset) and ``result`` (:242-251: force iff
fragments exist already), and ``job`` (:292-304: a file below ``min_input_size`` has no job and none of its bytes
is looked at).  ``subcategory_less`` and the metadata requirements have no counterpart.  ``device="cpu"`` runs the
host restatement (``rpp_incompressible_host_scan``).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _native as N
from .codec import _raise_status, _stream_ptr
from .lz4 import MAX_BLOCK, _ptr, check_search
from .zstd import ENC_ADAPTIVE, LONG_MAX_BLOCK, check_long

DEFAULT_CATEGORY = "<default>"  # categorizer::DEFAULT_CATEGORY
INCOMPRESSIBLE_CATEGORY = "incompressible"
CATEGORY_NAMES = (DEFAULT_CATEGORY, INCOMPRESSIBLE_CATEGORY)  # by the kernels' category number
TOTALS = 5  # RPP_INCOMPRESSIBLE_TOTALS: total_in, total_out, blocks, incompressible_blocks, single verdict


def parse_size_with_unit(value: Union[int, str]) -> int:
    """``parse_size_with_unit`` (src/util.cpp:566-604): digits, then at most one of k, m, g, t in either case."""
    if isinstance(value, (int, np.integer)):
        return int(value)
    text = str(value)
    digits = len(text) - len(text.lstrip("0123456789"))
    if digits == 0:
        raise RuntimeError(f"cannot parse size value: {text}")
    number, suffix = int(text[:digits]), text[digits:]
    if suffix == "":
        return number
    if len(suffix) == 1 and suffix.lower() in "kmgt":
        return number << 10 * ("kmgt".index(suffix.lower()) + 1)
    raise RuntimeError(f"unsupported size suffix: {suffix}")


@dataclass(frozen=True)
class IncompressibleConfig:
    """``incompressible_categorizer_config`` with the factory's defaults (:316-339); ``options`` and ``search`` are
    the encoder's words (zstd.py) in the place of ``zstd_level``."""

    min_input_size: Union[int, str] = 256
    block_size: Union[int, str] = 1 << 20
    generate_fragments: bool = False
    max_ratio: float = 0.99
    options: int = 0
    search: int = 0
    long: int = 0  # the encoder's long word (zstd.py): 1 lets a piece match anything earlier in itself

    def __post_init__(self):
        object.__setattr__(self, "min_input_size", parse_size_with_unit(self.min_input_size))
        object.__setattr__(self, "block_size", parse_size_with_unit(self.block_size))
        object.__setattr__(self, "generate_fragments", bool(self.generate_fragments))
        object.__setattr__(self, "max_ratio", float(self.max_ratio))
        if not 1 <= self.block_size <= MAX_BLOCK:
            raise ValueError(f"block_size must be between 1 and {MAX_BLOCK}, not {self.block_size}")
        if int(self.options) & ~ENC_ADAPTIVE:
            raise ValueError(f"unknown zstd encoder options: {self.options}")
        object.__setattr__(self, "options", int(self.options))
        object.__setattr__(self, "search", check_search(self.search))
        object.__setattr__(self, "long", check_long(self.long))
        if self.long and self.block_size > LONG_MAX_BLOCK:
            raise ValueError(f"block_size must be at most {LONG_MAX_BLOCK} with long=1, not {self.block_size}")


class Hole(NamedTuple):
    """A hole of a sparse file: ``size`` bytes that are not data."""
    size: int


class Fragment(NamedTuple):
    category: str  # "<default>" or "incompressible"
    size: int


class Stats(NamedTuple):
    """The figures of the reference's trace line, summed over the file's extents."""
    incompressible_blocks: int
    total_blocks: int
    total_in: int
    total_out: int


class FileResult(NamedTuple):
    fragments: Optional[List[Fragment]]  # None: the file has no job (below min_input_size)
    stats: Optional[Stats]


@dataclass
class PieceScan:
    """What the kernels say (host arrays).  Extent e holds the pieces ``piece_base[e] : piece_base[e + 1]``; its
    fragment rows are ``frag_rows[piece_base[e] : piece_base[e] + frag_count[e]]`` (category number, bytes), and
    the rows behind them are as the call found them."""

    sizes: np.ndarray        # uint64 [pieces]: the encoder's frame size
    verdicts: np.ndarray     # uint32 [pieces]: 1 incompressible
    totals: np.ndarray       # uint64 [extents, 5]: total_in, total_out, blocks, incompressible_blocks, single verdict
    frag_rows: np.ndarray    # uint64 [pieces, 2]
    frag_count: np.ndarray   # uint32 [extents]
    piece_base: np.ndarray   # uint32 [extents + 1]
    piece_sizes: np.ndarray  # uint64 [pieces]
    total_bytes: int         # the bytes of the buffer the call built: every extent's, nothing else

    def fragments(self, e: int) -> List[tuple]:
        at = int(self.piece_base[e])
        return [(int(c), int(n)) for c, n in self.frag_rows[at:at + int(self.frag_count[e])]]


def cut(extent_sizes: Sequence[int], block_size: int):
    """The pieces of extents laid end to end in one buffer: (offsets, sizes, piece_base)."""
    offs, sizes, base, at = [], [], [0], 0
    for n in extent_sizes:
        for o in range(0, int(n), block_size):
            offs.append(at + o)
            sizes.append(min(block_size, int(n) - o))
        at += int(n)
        base.append(len(offs))
    return np.asarray(offs, np.uint64), np.asarray(sizes, np.uint64), np.asarray(base, np.uint32)


def scan_batch(d_in: torch.Tensor, in_offsets, in_sizes, piece_base, cfg: IncompressibleConfig, out=None,
               stream: Optional[torch.cuda.Stream] = None):
    """One ``rpp_incompressible_scan_batch`` over pieces of the uint8 CUDA tensor ``d_in`` (host arrays of offsets,
    sizes and the extents' piece ranges): the device tensors (sizes, verdicts, totals, frag_rows, frag_count,
    status), which ``out`` may provide.  Asynchronous on the stream; no output buffer is allocated."""
    dev = d_in.device
    npieces, nextents = len(in_sizes), len(piece_base) - 1
    total = int(np.asarray(in_sizes, np.uint64).sum())
    d_off = torch.from_numpy(np.asarray(in_offsets, np.uint64).view(np.int64)).to(dev)
    d_sz = torch.from_numpy(np.asarray(in_sizes, np.uint64).view(np.int64)).to(dev)
    d_base = torch.from_numpy(np.asarray(piece_base, np.uint32).view(np.int32)).to(dev)
    if out is None:
        out = (torch.zeros(npieces, dtype=torch.int64, device=dev), torch.zeros(npieces, dtype=torch.int32, device=dev),
               torch.zeros((nextents, TOTALS), dtype=torch.int64, device=dev),
               torch.zeros((npieces, 2), dtype=torch.int64, device=dev),
               torch.zeros(nextents, dtype=torch.int32, device=dev), torch.zeros(npieces, dtype=torch.int32, device=dev))
    sizes, verdicts, totals, rows, count, status = out
    ws_bytes = int(N.lib().rpp_incompressible_workspace_bytes_long(total, npieces, nextents, cfg.long))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_incompressible_scan_batch_long(
        _ptr(d_in), _ptr(d_off), _ptr(d_sz), npieces, _ptr(d_base), nextents, cfg.max_ratio,
        int(cfg.generate_fragments), cfg.options, cfg.search, cfg.long, _ptr(sizes), _ptr(verdicts), _ptr(totals),
        _ptr(rows), _ptr(count), _ptr(status), total, _ptr(ws), ws_bytes, _stream_ptr(stream)))
    return out


def host_scan(flat: np.ndarray, in_offsets, in_sizes, piece_base, cfg: IncompressibleConfig, out=None):
    """``rpp_incompressible_host_scan``: the same numbers on the CPU, as host arrays."""
    npieces, nextents = len(in_sizes), len(piece_base) - 1
    offs, szs = np.ascontiguousarray(in_offsets, np.uint64), np.ascontiguousarray(in_sizes, np.uint64)
    base = np.ascontiguousarray(piece_base, np.uint32)
    if out is None:
        out = (np.zeros(npieces, np.uint64), np.zeros(npieces, np.uint32), np.zeros((nextents, TOTALS), np.uint64),
               np.zeros((npieces, 2), np.uint64), np.zeros(nextents, np.uint32), np.zeros(npieces, np.int32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _raise_status(N.lib().rpp_incompressible_host_scan_long(
        p(flat), p(offs), p(szs), npieces, p(base), nextents, cfg.max_ratio, int(cfg.generate_fragments), cfg.options,
        cfg.search, cfg.long, *(p(a) for a in out)))
    return out


def scan_pieces(extents: Sequence[bytes], cfg: IncompressibleConfig, device="cuda") -> PieceScan:
    """The raw results for a list of extents (each a contiguous run of file data): one launch sequence for all
    their pieces.  The extents are laid end to end in one buffer and cut by offsets, without a copy per piece."""
    dev = torch.device(device)
    offs, szs, base = cut([len(x) for x in extents], cfg.block_size)
    npieces, nextents = len(szs), len(extents)
    total = int(sum(len(x) for x in extents))
    flat = np.zeros(max(total, 16), np.uint8)
    flat[:total] = np.frombuffer(b"".join(bytes(x) for x in extents), np.uint8)
    if npieces == 0:  # (the native calls do nothing for no pieces)
        res = (np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros((nextents, TOTALS), np.uint64),
               np.zeros((0, 2), np.uint64), np.zeros(nextents, np.uint32), np.zeros(0, np.int32))
    elif dev.type == "cpu":
        res = host_scan(flat, offs, szs, base, cfg)
    else:
        out = scan_batch(torch.from_numpy(flat).to(dev), offs, szs, base, cfg)
        torch.cuda.current_stream().synchronize()
        res = tuple(t.cpu().numpy() for t in out)
    sizes, verdicts, totals, rows, count, status = res
    for st in status:
        _raise_status(int(st))
    return PieceScan(sizes.view(np.uint64), verdicts.view(np.uint32), totals.view(np.uint64), rows.view(np.uint64),
                     count.view(np.uint32), base, szs, total)


class IncompressibleCategorizer:
    """``incompressible_categorizer_``.  A file is ``bytes``, or a list of ``bytes`` and :class:`Hole` in file
    order (neighbouring ``bytes`` are one extent).  ``last_total_bytes`` is the size of the buffer the last call
    built: the bytes of the files that got a job."""

    def __init__(self, cfg: Optional[IncompressibleConfig] = None, device="cuda"):
        self.cfg = cfg if cfg is not None else IncompressibleConfig()
        self.device = torch.device(device)
        self.last_total_bytes = 0

    def categories(self):
        return (INCOMPRESSIBLE_CATEGORY,)

    @staticmethod
    def _parts(file) -> list:
        """The file as data extents and holes in order, neighbouring data merged."""
        if isinstance(file, (bytes, bytearray, memoryview)):
            return [bytes(file)]
        parts: list = []
        for item in file:
            if isinstance(item, Hole):
                parts.append(item)
            elif parts and not isinstance(parts[-1], Hole):
                parts[-1] = parts[-1] + bytes(item)
            else:
                parts.append(bytes(item))
        return parts

    def _extent_fragments(self, scan: PieceScan, e: int, force_single_default: bool) -> List[Fragment]:
        """``data_extent_fragments::get_fragments``"""
        rows = scan.fragments(e)
        if rows:
            return [Fragment(CATEGORY_NAMES[c], n) for c, n in rows]
        total_in, _, _, _, single = (int(v) for v in scan.totals[e])
        if total_in > 0 and (force_single_default or single):
            return [Fragment(CATEGORY_NAMES[single], total_in)]
        return []

    def categorize_many(self, files: Sequence) -> List[FileResult]:
        """Every file's fragments and stats from one launch sequence over all their pieces."""
        jobs, extents = [], []
        for file in files:
            parts = self._parts(file)
            size = sum(p.size if isinstance(p, Hole) else len(p) for p in parts)
            if size < self.cfg.min_input_size:  # job(): no job, and none of the file's bytes goes anywhere
                jobs.append(None)
                continue
            jobs.append(parts)
            extents.extend(p for p in parts if not isinstance(p, Hole))
        scan = scan_pieces(extents, self.cfg, self.device)
        self.last_total_bytes = scan.total_bytes
        out, e = [], 0
        for parts in jobs:
            if parts is None:
                out.append(FileResult(None, None))
                continue
            frags: List[Fragment] = []
            hard = blocks = t_in = t_out = 0
            open_extent = None  # the extent that add_data has fed since the last reset
            for p in parts:
                if isinstance(p, Hole):  # add_hole: flush with force, the hole as a default fragment, reset
                    if open_extent is not None:
                        frags += self._extent_fragments(scan, open_extent, True)
                        open_extent = None
                    frags.append(Fragment(DEFAULT_CATEGORY, int(p.size)))
                else:
                    open_extent = e
                    t_in, t_out, blocks, hard = (a + int(b) for a, b in zip((t_in, t_out, blocks, hard), scan.totals[e]))
                    e += 1
            if open_extent is not None:  # result(): force iff fragments exist already
                frags += self._extent_fragments(scan, open_extent, bool(frags))
            out.append(FileResult(frags, Stats(hard, blocks, t_in, t_out)))
        return out

    def categorize(self, data) -> FileResult:
        return self.categorize_many([data])[0]
