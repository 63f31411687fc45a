"""The segmenter's match search over the MI355X kernels.

``mkdwarfs``' segmenter (src/writer/segmenter.cpp, include/dwarfs/writer/internal/cyclic_hash.h) looks for parts of
incoming data that already exist in an earlier block: an rsync hash over a sliding window at every frame position,
a per-block table of the hashes at step-aligned offsets behind a one-hash bloom filter, and for every filter hit a
byte compare that is extended backwards and forwards.  These are the tensor-level wrappers of the segment group of
``include/ricepp_amd.h``: the window hashes, the block index, the filtered hit list and verify-and-extend.  The
sequential control loop (choosing the best match, emitting chunks, appending to blocks, the look-back bookkeeping)
stays with the caller; candidates come from the index as it stands when the scan is launched.
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

HIT_DTYPE = np.dtype([("pos", "<u4"), ("hash", "<u4")])
CANDIDATE_DTYPE = np.dtype([("extent_offset", "<u8"), ("block_offset", "<u8"), ("pos", "<u4"), ("off", "<u4"),
                            ("begin", "<u4"), ("end", "<u4"), ("block_frames", "<u4"), ("reserved", "<u4")])
MATCH_DTYPE = np.dtype([("off", "<u4"), ("pos", "<u4"), ("size", "<u4")])


@dataclass(frozen=True)
class SegmenterConfig:
    """``rpp_segment_config``: W = 1 << window_bits frames of ``granularity`` bytes, index step
    max(1, W >> increment_shift) frames, bloom filters of ``filter_bits`` bits (a power of two, at least 64)."""

    window_bits: int = 12
    increment_shift: int = 1
    granularity: int = 1
    filter_bits: int = 1 << 16

    def native(self) -> N.RppSegmentConfig:
        for v in (self.window_bits, self.increment_shift, self.granularity):
            if not 0 <= int(v) < 2**32:
                _raise_status(N.RPP_UNSUPPORTED_CONFIG)
        if not 0 <= int(self.filter_bits) < 2**64:
            _raise_status(N.RPP_UNSUPPORTED_CONFIG)
        c = N.RppSegmentConfig(int(self.window_bits), int(self.increment_shift), int(self.granularity), 0,
                               int(self.filter_bits))
        _raise_status(N.lib().rpp_segment_check_config(C.byref(c)))
        return c

    @property
    def window_frames(self) -> int:
        return 1 << self.window_bits

    @property
    def window_bytes(self) -> int:
        return self.window_frames * self.granularity

    @property
    def step_frames(self) -> int:
        return max(1, self.window_frames >> self.increment_shift)

    @property
    def filter_words(self) -> int:
        return self.filter_bits // 64

    def positions(self, frames: int) -> int:
        return int(N.lib().rpp_segment_positions(C.byref(self.native()), int(frames)))

    def slots(self, frames: int) -> int:
        return int(N.lib().rpp_segment_index_slots(C.byref(self.native()), int(frames)))


def tile_frames() -> int:
    """The positions of an extent that one workgroup hashes (``rpp_segment_tile_frames``)."""
    return int(N.lib().rpp_segment_tile_frames())


def _host_sizes(sizes) -> np.ndarray:
    if isinstance(sizes, torch.Tensor):
        return sizes.detach().cpu().numpy().astype(np.int64)
    return np.asarray(sizes, dtype=np.int64).reshape(-1)


def _check_device_status(st: int) -> None:
    if st == N.RPP_INVALID_ARGUMENT:
        raise ValueError("an extent or block of 2^32 frames or more, or sizes beyond the stated total")
    _raise_status(st)


def window_hashes(data: torch.Tensor, offsets, sizes, cfg: SegmenterConfig,
                  stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """The hash at every window position of every extent ``data[offsets[b] : offsets[b] + sizes[b] * g]`` (offsets
    in bytes, sizes in frames): ``(hashes, starts)``, a uint32-valued int32 device tensor and the n + 1 host
    offsets into it (extent b's hashes are ``hashes[starts[b]:starts[b + 1]]``; an extent shorter than the window
    has none).  Synchronises to read the status."""
    c = cfg.native()
    dev = data.device
    sz = _host_sizes(sizes)
    n = sz.size
    if (sz < 0).any() or (sz >= 2**32).any():
        raise ValueError("an extent must be shorter than 2^32 frames")
    total = int(sz.sum())
    npos = np.array([cfg.positions(int(f)) for f in sz], dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(npos))).astype(np.int64)
    hashes = torch.empty(max(int(starts[-1]), 1), dtype=torch.int32, device=dev)
    if n == 0:
        return hashes[:0], starts
    d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
    L = N.lib()
    ws_bytes = L.rpp_segment_hash_workspace_bytes(n, total)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    _raise_status(L.rpp_segment_hash_batch(C.byref(c), _ptr(data), _ptr(d_off), _ptr(d_sz), n, total, _ptr(hashes),
                                           int(starts[-1]), _ptr(d_start), _ptr(d_status), _ptr(ws), ws_bytes,
                                           _stream_ptr(stream)))
    if stream is not None:
        stream.synchronize()
    _check_device_status(int(d_status.item()))
    assert d_start.cpu().numpy().tolist() == starts.tolist()
    return hashes[:int(starts[-1])], starts


@dataclass
class BlockIndex:
    """The index of n blocks on the device: dense slot arrays (block b's slots are ``starts[b]:starts[b + 1]``),
    one filter per block and the global filter (int64 tensors holding the uint64 words)."""

    cfg: SegmenterConfig
    block_offsets: np.ndarray   # bytes, into the block data
    block_frames: np.ndarray
    starts: np.ndarray          # n + 1
    hash: torch.Tensor          # int32 (uint32 values) [slots]
    offset: torch.Tensor        # int32 [slots], frames
    entered: torch.Tensor       # uint8 [slots]
    block_filters: torch.Tensor  # int64 [n, words]
    global_filter: torch.Tensor  # int64 [words]

    @classmethod
    def build(cls, data: torch.Tensor, offsets, sizes, cfg: SegmenterConfig, global_filter: Optional[torch.Tensor] = None,
              stream: Optional[torch.cuda.Stream] = None) -> "BlockIndex":
        """``rpp_segment_index_batch`` for the blocks ``data[offsets[b] : offsets[b] + sizes[b] * g]``.  A given
        ``global_filter`` is ORed into (blocks indexed by several calls share it)."""
        c = cfg.native()
        dev = data.device
        sz = _host_sizes(sizes)
        n = sz.size
        if (sz < 0).any() or (sz >= 2**32).any():
            raise ValueError("a block must be shorter than 2^32 frames")
        nslots = np.array([cfg.slots(int(f)) for f in sz], dtype=np.int64)
        starts = np.concatenate(([0], np.cumsum(nslots))).astype(np.int64)
        total = int(starts[-1])
        words = cfg.filter_words
        if global_filter is None:
            global_filter = torch.zeros(words, dtype=torch.int64, device=dev)
        elif global_filter.dtype != torch.int64 or global_filter.numel() != words or not global_filter.is_contiguous():
            raise ValueError(f"global_filter must be a contiguous int64 tensor of {words} words")
        idx = cls(cfg, _host_sizes(offsets), sz, starts,
                  torch.zeros(max(total, 1), dtype=torch.int32, device=dev)[:total],
                  torch.zeros(max(total, 1), dtype=torch.int32, device=dev)[:total],
                  torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)[:total],
                  torch.zeros((n, words), dtype=torch.int64, device=dev), global_filter)
        if n == 0:
            return idx
        d_off, d_sz = _i64(offsets, dev), _i64(sizes, dev)
        L = N.lib()
        ws_bytes = L.rpp_segment_index_workspace_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        d_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_status = torch.zeros(1, dtype=torch.int32, device=dev)
        _raise_status(L.rpp_segment_index_batch(C.byref(c), _ptr(data), _ptr(d_off), _ptr(d_sz), n, int(sz.max()),
                                                _ptr(idx.hash), _ptr(idx.offset), _ptr(idx.entered), total,
                                                _ptr(d_start), _ptr(idx.block_filters), _ptr(idx.global_filter),
                                                _ptr(d_status), _ptr(ws), ws_bytes, _stream_ptr(stream)))
        if stream is not None:
            stream.synchronize()
        _check_device_status(int(d_status.item()))
        return idx

    def slots(self, b: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(hash as uint32, offset, entered) of block b on the host."""
        lo, hi = int(self.starts[b]), int(self.starts[b + 1])
        return (self.hash[lo:hi].cpu().numpy().view(np.uint32), self.offset[lo:hi].cpu().numpy().view(np.uint32),
                self.entered[lo:hi].cpu().numpy())


@dataclass
class DeviceHits:
    """Reusable buffers of :func:`scan_into` for n extents of ``total_frames`` frames in all (graph capture)."""

    capacity: int
    hits: torch.Tensor       # int32 [capacity, 2]: (pos, hash) as uint32 values
    hit_start: torch.Tensor  # int64 [n + 1]
    result: torch.Tensor     # int64 [2]: count | status in the low 32 bits of word 1
    workspace: torch.Tensor
    n: int
    total_frames: int

    @classmethod
    def new(cls, n: int, total_frames: int, capacity: int, device="cuda") -> "DeviceHits":
        ws_bytes = N.lib().rpp_segment_scan_workspace_bytes(int(n), int(total_frames))
        return cls(int(capacity), torch.zeros((max(int(capacity), 1), 2), dtype=torch.int32, device=device),
                   torch.zeros(int(n) + 1, dtype=torch.int64, device=device),
                   torch.zeros(2, dtype=torch.int64, device=device),
                   torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device), int(n), int(total_frames))

    def count(self) -> int:
        return int(self.result[0].item())

    def status(self) -> int:
        low = int(self.result[1].item()) & 0xFFFFFFFF
        return low - (1 << 32) if low & 0x80000000 else low

    def host(self) -> np.ndarray:
        """The hits written (``HIT_DTYPE``): min(count, capacity) of them."""
        k = min(self.count(), self.capacity)
        return self.hits[:k].cpu().numpy().view(np.uint32).reshape(-1, 2).copy().view(HIT_DTYPE).reshape(-1)


def scan_into(out: DeviceHits, data: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, filt: torch.Tensor,
              cfg: SegmenterConfig, stream: Optional[torch.cuda.Stream] = None) -> DeviceHits:
    """``rpp_segment_scan_batch`` into ``out``: asynchronous on the stream, no host round trip, graph-capturable
    (``offsets`` / ``sizes`` are int64 device tensors, ``filt`` an int64 device tensor of ``cfg.filter_words``)."""
    c = cfg.native()
    if filt.dtype != torch.int64 or filt.numel() != cfg.filter_words or not filt.is_contiguous():
        raise ValueError(f"the filter must be a contiguous int64 tensor of {cfg.filter_words} words")
    if offsets.dtype != torch.int64 or sizes.dtype != torch.int64 or sizes.numel() != out.n or offsets.numel() != out.n:
        raise ValueError("offsets and sizes must be int64 device tensors with one entry per extent of `out`")
    L = N.lib()
    _raise_status(L.rpp_segment_scan_batch(C.byref(c), _ptr(data), _ptr(offsets), _ptr(sizes), out.n,
                                           out.total_frames, _ptr(filt), _ptr(out.hits), out.capacity,
                                           _ptr(out.hit_start), _ptr(out.result), _ptr(out.workspace),
                                           out.workspace.numel(), _stream_ptr(stream)))
    return out


def scan(data: torch.Tensor, offset: int, frames: int, filt: torch.Tensor, cfg: SegmenterConfig,
         capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """The filter hits of one extent: ``(positions, hashes, count)``, uint32 host arrays in ascending position.
    With a ``capacity`` below the count only the first ``capacity`` hits come back (``count > len(positions)``
    tells the overflow); without one the scan is repeated with room for all."""
    if not 0 <= int(frames) < 2**32:
        raise ValueError("an extent must be shorter than 2^32 frames")
    dev = data.device
    d_off, d_sz = _i64([int(offset)], dev), _i64([int(frames)], dev)
    cap = int(capacity) if capacity is not None else max(1024, cfg.positions(frames) // 64)
    while True:
        out = scan_into(DeviceHits.new(1, frames, cap, dev), data, d_off, d_sz, filt, cfg)
        count, st = out.count(), out.status()
        if st == N.RPP_OUTPUT_TOO_SMALL and capacity is None:
            cap = count
            continue
        if st != N.RPP_OUTPUT_TOO_SMALL:
            _check_device_status(st)
        h = out.host()
        return h["pos"].copy(), h["hash"].copy(), count


def extend(extent_data: torch.Tensor, block_data: torch.Tensor, candidates: np.ndarray, cfg: SegmenterConfig,
           stream: Optional[torch.cuda.Stream] = None) -> np.ndarray:
    """``rpp_segment_extend_batch``: ``candidates`` is a host array of ``CANDIDATE_DTYPE``; returns
    ``MATCH_DTYPE`` rows (size 0 = no match)."""
    c = cfg.native()
    cand = np.ascontiguousarray(candidates, dtype=CANDIDATE_DTYPE).reshape(-1)
    n = cand.size
    if n == 0:
        return np.zeros(0, MATCH_DTYPE)
    dev = extent_data.device
    d_cand = torch.from_numpy(cand.view(np.uint8).copy()).to(dev)
    d_out = torch.zeros(n * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    _raise_status(N.lib().rpp_segment_extend_batch(C.byref(c), _ptr(extent_data), _ptr(block_data), _ptr(d_cand), n,
                                                   _ptr(d_out), _stream_ptr(stream)))
    if stream is not None:
        stream.synchronize()
    return d_out.cpu().numpy().view(MATCH_DTYPE).copy()


def candidates(positions, offs, extent_offset: int, block_offset, begin: int, end: int, block_frames) -> np.ndarray:
    """``CANDIDATE_DTYPE`` rows for hits at ``positions`` against slot offsets ``offs``."""
    pos = np.asarray(positions, dtype=np.uint32).reshape(-1)
    c = np.zeros(pos.size, CANDIDATE_DTYPE)
    c["extent_offset"] = extent_offset
    c["block_offset"] = block_offset
    c["pos"] = pos
    c["off"] = offs
    c["begin"] = begin
    c["end"] = end
    c["block_frames"] = block_frames
    return c


def find_candidates(extent: bytes, blocks: Sequence[bytes], cfg: SegmenterConfig, device="cuda") -> np.ndarray:
    """Every verified match of ``extent`` against the index of ``blocks`` as it stands: the blocks are indexed, the
    extent is scanned against the global filter, hits are joined to the entered slots of equal hash on the host,
    and the pairs are verified and extended on the device.  Returns rows ``(pos, block, off, size)`` (int64
    [k, 4], sorted) of the matches with size > 0, duplicates removed."""
    g = cfg.granularity
    bsz = [len(b) // g for b in blocks]
    boff = np.zeros(len(blocks), dtype=np.int64)
    if len(blocks):
        boff[1:] = np.cumsum([(len(b) + 15) // 16 * 16 for b in blocks[:-1]])
    blob = bytearray(int(boff[-1]) + len(blocks[-1]) + 16 if len(blocks) else 16)
    for o, b in zip(boff, blocks):
        blob[o:o + len(b)] = b
    d_blocks = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(device)
    d_ext = torch.from_numpy(np.frombuffer(bytes(extent) + bytes(16), np.uint8).copy()).to(device)
    n = len(extent) // g
    index = BlockIndex.build(d_blocks, boff, bsz, cfg)
    pos, hashes, _ = scan(d_ext, 0, n, index.global_filter, cfg)
    rows: List[np.ndarray] = []
    for b in range(len(blocks)):
        h, off, entered = index.slots(b)
        h, off = h[entered != 0], off[entered != 0]
        order = np.argsort(h, kind="stable")
        h, off = h[order], off[order]
        lo, hi = np.searchsorted(h, hashes, "left"), np.searchsorted(h, hashes, "right")
        reps = hi - lo
        if reps.sum() == 0:
            continue
        ppos = np.repeat(pos, reps)
        slot = np.concatenate([np.arange(a, z) for a, z in zip(lo, hi) if z > a])
        m = extend(d_ext, d_blocks, candidates(ppos, off[slot], 0, int(boff[b]), 0, n, bsz[b]), cfg)
        m = m[m["size"] > 0]
        rows.append(np.stack([m["pos"].astype(np.int64), np.full(m.size, b, np.int64), m["off"].astype(np.int64),
                              m["size"].astype(np.int64)], axis=1))
    if not rows:
        return np.zeros((0, 4), np.int64)
    return np.unique(np.concatenate(rows), axis=0)


# ---- the host restatement (no GPU) ----

def _bytes_ptr(buf) -> C.c_void_p:
    return C.cast(buf, C.c_void_p)


def _cbuf(data: bytes):
    data = bytes(data)
    return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")


def host_hashes(data: bytes, cfg: SegmenterConfig) -> np.ndarray:
    """``rpp_segment_host_hashes``: the uint32 hash of every window position of ``data`` (whole frames only)."""
    c = cfg.native()
    frames = len(data) // cfg.granularity
    out = np.zeros(cfg.positions(frames), np.uint32)
    _raise_status(N.lib().rpp_segment_host_hashes(C.byref(c), _bytes_ptr(_cbuf(data)), frames,
                                                  C.c_void_p(out.ctypes.data)))
    return out


@dataclass
class HostIndex:
    hash: np.ndarray
    offset: np.ndarray
    entered: np.ndarray
    block_filter: np.ndarray   # uint64 [words]
    global_filter: np.ndarray  # uint64 [words]


def host_index(block: bytes, cfg: SegmenterConfig, global_filter: Optional[np.ndarray] = None) -> HostIndex:
    """``rpp_segment_host_index`` of one block; a given ``global_filter`` (uint64 [words]) is ORed into."""
    c = cfg.native()
    frames = len(block) // cfg.granularity
    ns = cfg.slots(frames)
    words = cfg.filter_words
    gf = np.zeros(words, np.uint64) if global_filter is None else global_filter
    if gf.dtype != np.uint64 or gf.size != words or not gf.flags.c_contiguous:
        raise ValueError(f"global_filter must be a contiguous uint64 array of {words} words")
    r = HostIndex(np.zeros(ns, np.uint32), np.zeros(ns, np.uint32), np.zeros(ns, np.uint8), np.zeros(words, np.uint64), gf)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    _raise_status(N.lib().rpp_segment_host_index(C.byref(c), _bytes_ptr(_cbuf(block)), frames, p(r.hash), p(r.offset),
                                                 p(r.entered), p(r.block_filter), p(r.global_filter)))
    return r


def host_scan(data: bytes, filt: np.ndarray, cfg: SegmenterConfig,
              capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """``rpp_segment_host_scan``: ``(positions, hashes, count)`` as :func:`scan` returns them."""
    c = cfg.native()
    filt = np.ascontiguousarray(filt, dtype=np.uint64)
    if filt.size != cfg.filter_words:
        raise ValueError(f"the filter must hold {cfg.filter_words} words")
    frames = len(data) // cfg.granularity
    cap = cfg.positions(frames) if capacity is None else int(capacity)
    hits = np.zeros(max(cap, 1), HIT_DTYPE)
    count = C.c_uint64(0)
    st = N.lib().rpp_segment_host_scan(C.byref(c), _bytes_ptr(_cbuf(data)), frames, C.c_void_p(filt.ctypes.data),
                                       C.c_void_p(hits.ctypes.data), cap, C.cast(C.byref(count), C.c_void_p))
    if st != N.RPP_OUTPUT_TOO_SMALL:
        _raise_status(st)
    k = min(int(count.value), cap)
    return hits["pos"][:k].copy(), hits["hash"][:k].copy(), int(count.value)


def host_extend(extent_data: bytes, block_data: bytes, cands: np.ndarray, cfg: SegmenterConfig) -> np.ndarray:
    """``rpp_segment_host_extend``: ``MATCH_DTYPE`` rows for ``CANDIDATE_DTYPE`` rows."""
    c = cfg.native()
    cand = np.ascontiguousarray(cands, dtype=CANDIDATE_DTYPE).reshape(-1)
    out = np.zeros(cand.size, MATCH_DTYPE)
    if cand.size:
        _raise_status(N.lib().rpp_segment_host_extend(C.byref(c), _bytes_ptr(_cbuf(extent_data)),
                                                      _bytes_ptr(_cbuf(block_data)), C.c_void_p(cand.ctypes.data),
                                                      cand.size, C.c_void_p(out.ctypes.data)))
    return out
