"""File extraction over the MI355X kernels: chunks of decoded blocks become files, and files become checksums.

The reader's two bulk paths -- ``dwarfsextract`` (src/utility/filesystem_extractor.cpp) and ``dwarfsck --checksum=ALGO``
(tools/src/dwarfsck_main.cpp, ``do_checksum``) -- walk every file's chunk list ``(block, offset, size)``
(thrift/metadata.thrift, ``chunk``) and read the chunk bytes out of the decoded blocks.  Here the decoded blocks stay
on the device (``block_codec.decode_sections_device``), one gather launch lays every file of a batch contiguously
into one device buffer (``rpp_extract_gather_batch``; the rules are at the top of csrc/extract/extract_host.cpp),
and the file digests come from ``dedup.file_hash_batch`` on that buffer without a round trip through the host.
A checksum name that ``dedup`` does not know (``sha256``, ``md5``, ``sha1``, ...: ``digest.ALGORITHMS``) goes through
``digest.digest_batch`` instead, on the device or, with ``device="cpu"``, on the host definition.

The caller supplies the chunk tables: the frozen metadata is not parsed here.  A file is a list of :class:`Chunk`
and :class:`Hole` (a sparse file's hole: ``size`` zero bytes without a source).  A chunk that does not fit its
block, or whose destination does not fit the output, is a *bad chunk*: its file has the status ``RPP_BAD_CHUNK``,
its destination bytes are left as they were, and every other chunk is copied as usual.  ``device="cpu"`` runs the
sequential definition (``rpp_extract_host_gather``).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import dedup, digest
from .categorize import Hole
from .codec import _raise_status, _stream_ptr
from .dedup import _algo, file_hash_batch
from .section import _i64, _ptr

CHUNK_DTYPE = np.dtype([("block", "<u4"), ("offset", "<u4"), ("size", "<u8")])  # rpp_chunk
HOLE_BLOCK = N.RPP_CHUNK_HOLE
FILE_ALIGN = 16  # a file starts on a 16-byte boundary of the gathered buffer
DEFAULT_MAX_BYTES = 1 << 30


class Chunk(NamedTuple):
    """``size`` bytes of block ``block`` from ``offset`` on."""
    block: int
    offset: int
    size: int


def tile_bytes() -> int:
    """The gather kernel's tile: one workgroup writes this many consecutive output bytes."""
    return int(N.lib().rpp_extract_tile_bytes())


@dataclass
class FileTable:
    """Files as chunk lists in CSR form: file f holds the rows ``first_chunk[f] : first_chunk[f + 1]`` of ``chunks``."""

    chunks: np.ndarray       # CHUNK_DTYPE [nchunks]
    first_chunk: np.ndarray  # uint64 [nfiles + 1]

    @classmethod
    def from_files(cls, files: Sequence[Sequence]) -> "FileTable":
        rows, first = [], [0]
        for file in files:
            for item in file:
                if isinstance(item, Hole):
                    rows.append((HOLE_BLOCK, 0, int(item.size)))
                else:
                    block, offset, size = item
                    rows.append((int(block), int(offset), int(size)))
            first.append(len(rows))
        return cls(np.array(rows, dtype=CHUNK_DTYPE).reshape(-1), np.asarray(first, np.uint64))

    @property
    def nfiles(self) -> int:
        return len(self.first_chunk) - 1

    @property
    def nchunks(self) -> int:
        return len(self.chunks)

    def _chunk_ends(self) -> np.ndarray:
        ends = np.zeros(self.nchunks + 1, np.uint64)
        np.cumsum(self.chunks["size"], out=ends[1:])
        return ends

    @property
    def file_sizes(self) -> np.ndarray:
        """uint64 [nfiles]: the sum of each file's chunk sizes."""
        ends, first = self._chunk_ends(), self.first_chunk.astype(np.int64)
        return ends[first[1:]] - ends[first[:-1]]

    def layout(self, lo: int = 0, hi: Optional[int] = None, file_dst=None):
        """The destinations of the files ``lo : hi``: ``(file_dst, chunk_dst, out_bytes)``.  ``file_dst`` defaults to
        the files back to back, each on a FILE_ALIGN boundary; it must not decrease and must leave every file room.
        ``chunk_dst`` (one entry more than the files have chunks) is the exclusive scan of the chunk sizes laid over
        ``file_dst``; its last entry is the end of the last chunk."""
        hi = self.nfiles if hi is None else hi
        sizes = self.file_sizes[lo:hi]
        if file_dst is None:
            padded = (sizes + np.uint64(FILE_ALIGN - 1)) // np.uint64(FILE_ALIGN) * np.uint64(FILE_ALIGN)
            file_dst = np.zeros(hi - lo, np.uint64)
            np.cumsum(padded[:-1], out=file_dst[1:])
            out_bytes = int(padded.sum())
        else:
            file_dst = np.asarray(file_dst, np.uint64)
            out_bytes = int((file_dst + sizes).max()) if hi > lo else 0
        first = self.first_chunk.astype(np.int64)
        c0, c1 = int(first[lo]), int(first[hi])
        ends = self._chunk_ends()
        counts = np.diff(first[lo:hi + 1])
        chunk_dst = np.zeros(c1 - c0 + 1, np.uint64)
        # a chunk's place: its file's, plus the chunk sizes of the same file before it
        chunk_dst[:-1] = np.repeat(file_dst - ends[first[lo:hi]], counts) + ends[c0:c1]
        if c1 > c0:
            chunk_dst[-1] = chunk_dst[-2] + self.chunks["size"][c1 - 1]
        return file_dst, chunk_dst, out_bytes


@dataclass
class GatherPlan:
    """The tables of one gather call on the device (files ``lo : hi`` of a :class:`FileTable`)."""

    nfiles: int
    nchunks: int
    out_bytes: int
    file_dst: np.ndarray    # uint64 [nfiles]
    file_sizes: np.ndarray  # uint64 [nfiles]
    d_chunks: torch.Tensor
    d_chunk_dst: torch.Tensor
    d_first_chunk: torch.Tensor
    workspace: torch.Tensor


def _host_tables(table: FileTable, lo: int, hi: int, file_dst, chunk_dst, out_bytes):
    hi = table.nfiles if hi is None else hi
    dst, cdst, total = table.layout(lo, hi, file_dst)
    if chunk_dst is not None:
        cdst = np.ascontiguousarray(chunk_dst, np.uint64)
    c0, c1 = int(table.first_chunk[lo]), int(table.first_chunk[hi])
    chunks = np.ascontiguousarray(table.chunks[c0:c1])
    first = np.ascontiguousarray(table.first_chunk[lo:hi + 1] - table.first_chunk[lo], np.uint64)
    return hi, dst, cdst, (total if out_bytes is None else int(out_bytes)), chunks, first


def plan_gather(table: FileTable, device="cuda", lo: int = 0, hi: Optional[int] = None, file_dst=None,
                chunk_dst=None, out_bytes: Optional[int] = None) -> GatherPlan:
    """Uploads the tables of the files ``lo : hi``.  ``file_dst`` places the files (default: back to back on 16-byte
    boundaries); ``chunk_dst`` and ``out_bytes`` override what :meth:`FileTable.layout` derives from it (tests)."""
    dev = torch.device(device)
    hi, dst, cdst, total, chunks, first = _host_tables(table, lo, hi, file_dst, chunk_dst, out_bytes)
    raw = np.zeros(max(len(chunks), 1), CHUNK_DTYPE)
    raw[:len(chunks)] = chunks
    ws_bytes = int(N.lib().rpp_extract_workspace_bytes(len(chunks), hi - lo, total))
    return GatherPlan(hi - lo, len(chunks), total, dst, table.file_sizes[lo:hi],
                      torch.from_numpy(raw.view(np.uint8)).to(dev), torch.from_numpy(cdst.view(np.int64)).to(dev),
                      torch.from_numpy(first.view(np.int64)).to(dev),
                      torch.empty(ws_bytes, dtype=torch.uint8, device=dev))


def padded_blocks(blocks: torch.Tensor) -> torch.Tensor:
    """``blocks`` as the gather needs it: uint8, contiguous, on a 16-byte boundary and a multiple of 16 bytes long
    (the kernels load aligned 16-byte words).  A tensor that is all that already is returned as it is."""
    blocks = blocks.contiguous().view(torch.uint8).reshape(-1)
    if blocks.numel() % 16 == 0 and blocks.data_ptr() % 16 == 0 and blocks.numel():
        return blocks
    out = torch.zeros(max((blocks.numel() + 15) // 16 * 16, 16), dtype=torch.uint8, device=blocks.device)
    out[:blocks.numel()] = blocks
    return out


def gather_into(blocks: torch.Tensor, block_offsets, block_sizes, plan: GatherPlan, out: torch.Tensor,
                status: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                blocks_bytes: Optional[int] = None) -> torch.Tensor:
    """One ``rpp_extract_gather_batch`` into ``out`` (uint8, 16-aligned, at least ``plan.out_bytes`` bytes; bytes that
    no chunk covers stay as they are): the int32 status per file.  ``blocks`` must satisfy :func:`padded_blocks`;
    ``blocks_bytes`` (default: all of it) is the length the chunks are checked against.  Asynchronous on the stream."""
    dev = blocks.device
    if blocks.dtype != torch.uint8 or blocks.data_ptr() % 16 or blocks.numel() % 16:
        raise ValueError("blocks must be a uint8 tensor on a 16-byte boundary, padded to a multiple of 16 bytes")
    if out.dtype != torch.uint8 or out.numel() < plan.out_bytes or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of at least {plan.out_bytes} bytes")
    d_boff, d_bsz = _i64(block_offsets, dev), _i64(block_sizes, dev)
    if status is None:
        status = torch.empty(plan.nfiles, dtype=torch.int32, device=dev)
    _raise_status(N.lib().rpp_extract_gather_batch(
        _ptr(blocks), blocks.numel() if blocks_bytes is None else int(blocks_bytes), _ptr(d_boff), _ptr(d_bsz),
        d_bsz.numel(), _ptr(plan.d_chunks), _ptr(plan.d_chunk_dst), plan.nchunks, _ptr(plan.d_first_chunk),
        plan.nfiles, _ptr(out), plan.out_bytes, _ptr(status), _ptr(plan.workspace), plan.workspace.numel(),
        _stream_ptr(stream)))
    return status


def host_gather(blocks, block_offsets, block_sizes, table: FileTable, lo: int = 0, hi: Optional[int] = None,
                file_dst=None, chunk_dst=None, out_bytes: Optional[int] = None, out: Optional[np.ndarray] = None,
                blocks_bytes: Optional[int] = None):
    """``rpp_extract_host_gather``, the definition, on host arrays: ``(out, file_dst, file_sizes, status)``.  ``out``
    (default: zeros) keeps the bytes that no chunk covers."""
    hi, dst, cdst, total, chunks, first = _host_tables(table, lo, hi, file_dst, chunk_dst, out_bytes)
    flat = np.ascontiguousarray(np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray)) else blocks,
                                np.uint8)
    boff, bsz = np.ascontiguousarray(block_offsets, np.uint64), np.ascontiguousarray(block_sizes, np.uint64)
    if out is None:
        out = np.zeros(total, np.uint8)
    if out.dtype != np.uint8 or out.size < total or not out.flags.c_contiguous:
        raise ValueError(f"out must be a contiguous uint8 array of at least {total} bytes")
    status = np.zeros(hi - lo, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    _raise_status(N.lib().rpp_extract_host_gather(
        p(flat), flat.size if blocks_bytes is None else int(blocks_bytes), p(boff), p(bsz), len(bsz), p(chunks),
        cdst.ctypes.data_as(C.c_void_p), len(chunks), first.ctypes.data_as(C.c_void_p), hi - lo, p(out), total,
        p(status)))
    return out, dst, table.file_sizes[lo:hi], status


def gather_files(blocks, block_offsets, block_sizes, table: FileTable, device="cuda", lo: int = 0,
                 hi: Optional[int] = None, stream: Optional[torch.cuda.Stream] = None):
    """The files ``lo : hi`` of ``table`` laid contiguously, each on a 16-byte boundary: ``(data, offsets, sizes,
    status)`` -- uint8, int64, int64 and int32 tensors on the device.  ``blocks`` is the buffer of decoded blocks
    (``block_codec.decode_sections_device`` gives all three); the bytes of a bad chunk, and the padding between
    files, are zero.  With ``device="cpu"`` everything is on the host and comes from ``rpp_extract_host_gather``."""
    dev = torch.device(device)
    if dev.type == "cpu":
        host = blocks.cpu().numpy() if isinstance(blocks, torch.Tensor) else blocks
        as_np = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a  # noqa: E731
        out, dst, sizes, status = host_gather(host, as_np(block_offsets), as_np(block_sizes), table, lo, hi)
        return (torch.from_numpy(out), torch.from_numpy(dst.astype(np.int64)),
                torch.from_numpy(sizes.astype(np.int64)), torch.from_numpy(status))
    blocks = padded_blocks(blocks.to(dev))
    plan = plan_gather(table, dev, lo, hi)
    out = torch.zeros(max(plan.out_bytes, 16), dtype=torch.uint8, device=dev)
    status = gather_into(blocks, block_offsets, block_sizes, plan, out, stream=stream)
    return (out, torch.from_numpy(plan.file_dst.astype(np.int64)).to(dev),
            torch.from_numpy(plan.file_sizes.astype(np.int64)).to(dev), status)


def _first_bad(status: np.ndarray, base: int = 0) -> None:
    bad = np.flatnonzero(status != N.RPP_OK)
    if len(bad):
        st = int(status[bad[0]])
        raise RuntimeError(f"file {base + int(bad[0])}: {N.STATUS_NAMES.get(st, st)} "
                           "(a chunk outside its block or its destination)")


def extract_files(blocks, block_offsets, block_sizes, table: FileTable, device="cuda",
                  max_bytes: int = DEFAULT_MAX_BYTES) -> List[bytes]:
    """Every file's bytes.  Raises ``RuntimeError`` naming the first file with ``RPP_BAD_CHUNK``."""
    files: List[bytes] = []
    for lo, hi in batches(table.file_sizes, max_bytes):
        data, offsets, sizes, status = gather_files(blocks, block_offsets, block_sizes, table, device, lo, hi)
        _first_bad(status.cpu().numpy(), lo)
        host = data.cpu().numpy()
        files.extend(host[o:o + n].tobytes() for o, n in zip(offsets.tolist(), sizes.tolist()))
    return files


def batches(file_sizes, max_bytes: int) -> List[Tuple[int, int]]:
    """File ranges ``(lo, hi)`` cut at file boundaries so that a range's gathered buffer (every file padded to 16
    bytes) stays at or under ``max_bytes``; a single file above ``max_bytes`` is a range of its own."""
    out, lo, used = [], 0, 0
    for i, n in enumerate(int(s) for s in file_sizes):
        padded = (n + FILE_ALIGN - 1) // FILE_ALIGN * FILE_ALIGN
        if i > lo and used + padded > max_bytes:
            out.append((lo, i))
            lo, used = i, 0
        used += padded
    if len(file_sizes) > lo:
        out.append((lo, len(file_sizes)))
    return out


def _hash_route(algo: str):
    """``(digest bytes, batch function)`` of a checksum name: the names of ``dedup.ALGORITHMS`` keep their route
    through ``dedup.file_hash_batch``, every other name goes to ``digest.digest_batch`` (ValueError if neither
    module knows it)."""
    if algo in dedup.ALGORITHMS:
        return _algo(algo)[1], file_hash_batch
    return digest.digest_bytes(algo), digest.digest_batch


def file_checksums(blocks, block_offsets, block_sizes, table: FileTable, algo: str = "xxh3-128",
                   max_bytes: int = DEFAULT_MAX_BYTES, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """``dwarfsck --checksum=ALGO`` for every file: ``(digests, status)``, a uint8 device tensor [nfiles, digest
    bytes] in DwarFS's digest order (as ``dedup.file_hash_batch``; ``hexdigests`` prints them as dwarfsck does) and
    the int32 gather status per file (the digest of a file with ``RPP_BAD_CHUNK`` is over zeros in the bad chunk's
    place).  Gather, then hash: two passes over the bytes, on the device, in batches of at most ``max_bytes``
    gathered bytes cut at file boundaries (:func:`batches`).  The names of ``digest.ALGORITHMS`` that ``dedup`` does
    not have also run with ``device="cpu"`` (host gather, then ``rpp_digest_host``; everything is on the host)."""
    dev = torch.device(device)
    if dev.type == "cpu" and algo in dedup.ALGORITHMS:
        raise ValueError("file_checksums runs the hash kernels: it needs a GPU device")
    nbytes, hash_batch = _hash_route(algo)
    if dev.type == "cpu":
        digests = torch.zeros((table.nfiles, nbytes), dtype=torch.uint8)
        status = torch.zeros(table.nfiles, dtype=torch.int32)
        for lo, hi in batches(table.file_sizes, max_bytes):
            out, offsets, sizes, st = gather_files(blocks, block_offsets, block_sizes, table, dev, lo, hi)
            status[lo:hi] = st
            if out.numel() == 0:
                out = torch.zeros(FILE_ALIGN, dtype=torch.uint8)  # (only empty files: a buffer to point at)
            hash_batch(out, offsets, sizes, algo, out=digests[lo:hi])
        return digests, status
    blocks = padded_blocks(blocks.to(dev))
    d_boff, d_bsz = _i64(block_offsets, dev), _i64(block_sizes, dev)
    digests = torch.zeros((table.nfiles, nbytes), dtype=torch.uint8, device=dev)
    status = torch.zeros(table.nfiles, dtype=torch.int32, device=dev)
    for lo, hi in batches(table.file_sizes, max_bytes):
        plan = plan_gather(table, dev, lo, hi)
        out = torch.zeros(max(plan.out_bytes, 16), dtype=torch.uint8, device=dev)
        gather_into(blocks, d_boff, d_bsz, plan, out, status=status[lo:hi])
        hash_batch(out, plan.file_dst.astype(np.int64), plan.file_sizes.astype(np.int64), algo,
                   out=digests[lo:hi])
    return digests, status


def hexdigests(digests: torch.Tensor) -> List[str]:
    return [row.tobytes().hex() for row in digests.cpu().numpy()]


def check_files(blocks, block_offsets, block_sizes, table: FileTable, expected, algo: str = "xxh3-128",
                max_bytes: int = DEFAULT_MAX_BYTES, device="cuda") -> List[int]:
    """The indices of the files whose digest differs from ``expected`` (one digest per file: bytes, hex strings, or
    a uint8 array [nfiles, digest bytes]) or whose gather status is not ``RPP_OK``."""
    digests, status = file_checksums(blocks, block_offsets, block_sizes, table, algo, max_bytes, device)
    if isinstance(expected, torch.Tensor):
        want = expected.to(device=digests.device, dtype=torch.uint8)
    elif isinstance(expected, np.ndarray):
        want = torch.as_tensor(expected.astype(np.uint8), device=digests.device)
    else:
        rows = b"".join(bytes.fromhex(e) if isinstance(e, str) else bytes(e) for e in expected)
        want = torch.as_tensor(np.frombuffer(rows, np.uint8).copy(), device=digests.device)
    if want.numel() != digests.numel():
        raise ValueError(f"expected needs {digests.shape[0]} digests of {digests.shape[1]} bytes")
    want = want.reshape(digests.shape)
    wrong = (digests != want).any(dim=1) | (status != N.RPP_OK)
    return torch.nonzero(wrong).reshape(-1).tolist()
