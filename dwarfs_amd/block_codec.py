"""DwarFS block codec for ricepp over the MI355X kernels (Python mirror).

Mirrors src/compression/ricepp.cpp: ``ricepp_block_compressor`` (:57-182),
``ricepp_block_decompressor`` (:184-255) and the factory registered as
``"ricepp"`` with option ``block_size`` (default 128, :272-301; like the
reference's factory the value is not range-checked there: an unsupported
size raises "Unsupported configuration" from the encoder at compress time,
:97-102).  A
compressed DwarFS block is

    varint(uncompressed bytes) + thrift-compact ricepp_block_header + bitstream

(the framing is produced/parsed by the C ABI: rpp_frame_header /
rpp_parse_frame).  Besides the one-block API the reference has, this module
offers ``compress_many`` / ``decompress_many``: the MI355X way to feed the
writer's per-block jobs (src/writer/filesystem_writer.cpp:255-287) and the
reader's block-cache jobs (src/reader/internal/block_cache.cpp:628-706) --
one launch for a whole batch of blocks.
"""

from __future__ import annotations

import ctypes as C
import json
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import lz4 as Z
from . import section as S
from . import zstd as ZS
from .codec import CodecConfig, _check, _raise_status, decode_batch, encode_batch

COMPRESSION_TYPE_RICEPP = 7  # include/dwarfs/compression.h
RICEPP_VERSION = 1  # src/compression/ricepp.cpp:55


def _meta_fields(metadata: str):
    m = json.loads(metadata)
    return (str(m["endianness"]), int(m["component_count"]), int(m["unused_lsb_count"]),
            int(m["bytes_per_sample"]))


def frame_header(uncompressed: int, block_size: int, cs: int, bps: int, ulsb: int, big_endian: bool,
                 version: int = RICEPP_VERSION) -> bytes:
    f = N.RppFrame(uncompressed, block_size, cs, bps, ulsb, 1 if big_endian else 0, version)
    buf = (C.c_uint8 * 64)()
    n = N.lib().rpp_frame_header(C.byref(f), buf)
    return bytes(buf[:n])


def parse_frame(data: bytes):
    buf = np.frombuffer(data, np.uint8)
    f = N.RppFrame()
    n = N.lib().rpp_parse_frame(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(f))
    if n < 0:
        raise RuntimeError("malformed ricepp block header")
    return f, int(n)


class RiceppBlockCompressor:
    """``ricepp_block_compressor`` (src/compression/ricepp.cpp:57-182)."""

    def __init__(self, block_size: int = 128, device="cuda"):
        self.block_size = int(block_size)
        self.device = torch.device(device)

    def clone(self) -> "RiceppBlockCompressor":
        return RiceppBlockCompressor(self.block_size, self.device)

    def type(self) -> int:
        return COMPRESSION_TYPE_RICEPP

    def describe(self) -> str:
        return f"ricepp [block_size={self.block_size}]"

    def metadata_requirements(self) -> str:
        return json.dumps({
            "bytes_per_sample": ["set", [2]],
            "component_count": ["range", 1, 2],
            "endianness": ["set", ["big", "little"]],
            "unused_lsb_count": ["range", 0, 8],
        }, separators=(",", ":"))

    def get_compression_constraints(self, metadata: str) -> dict:
        _, cs, _, bps = _meta_fields(metadata)
        return {"granularity": cs * bps}

    def estimate_memory_usage(self, data_size: int) -> int:
        return data_size

    def _config(self, metadata: Optional[str], size: int) -> CodecConfig:
        if metadata is None:
            raise RuntimeError("internal error: ricepp compression requires metadata")
        endianness, cs, ulsb, bps = _meta_fields(metadata)
        if size % (cs * bps):
            raise RuntimeError(f"unexpected data configuration: {size} bytes to compress, {cs} components, "
                               f"{bps} bytes per sample")
        cfg = CodecConfig(self.block_size, cs, "big" if endianness == "big" else "little", ulsb)
        _check(cfg)  # create_encoder's "Unsupported configuration" (:97-102)
        return cfg

    def compress(self, data: bytes, metadata: Optional[str]) -> bytes:
        return self.compress_many([data], metadata)[0]

    def compress_many(self, blocks: Sequence[bytes], metadata: Optional[str]) -> List[bytes]:
        """Compresses many blocks of one category in a single launch."""
        cfgs = {self._config(metadata, len(b)) for b in blocks}
        if not blocks:
            return []
        cfg = cfgs.pop()
        n = [len(b) // 2 for b in blocks]
        offs = np.zeros(len(blocks), np.int64)
        for i in range(1, len(blocks)):
            offs[i] = offs[i - 1] + (n[i - 1] + 7) // 8 * 8
        flat = np.zeros(int(offs[-1] + n[-1]) + 8 if blocks else 8, np.uint16)
        for o, b in zip(offs, blocks):
            flat[o:o + len(b) // 2] = np.frombuffer(b, np.uint16)
        d = torch.from_numpy(flat.view(np.int16)).to(self.device)
        res = encode_batch(cfg, d, offs, n)
        torch.cuda.current_stream().synchronize()
        res.check()
        sizes = res.sizes.cpu().numpy()
        data = res.data.cpu().numpy()
        out = []
        for i, b in enumerate(blocks):
            hdr = frame_header(len(b), self.block_size, cfg.component_stream_count, 2, cfg.unused_lsb_count,
                               cfg.byteorder == "big")
            o = int(res.offsets[i])
            out.append(hdr + data[o:o + int(sizes[i])].tobytes())
        return out

    def compress_many_sections(self, blocks: Sequence[bytes], metadata: Optional[str], first_number: int = 0) -> bytes:
        """Compresses many blocks of one category and returns them as image-ready BLOCK sections (header with
        both checksums + frame + bitstream each, back to back, numbered from ``first_number``): encode,
        checksums and assembly are one device batch on one stream, and only the finished bytes come back
        (the writer's fsblock::build_section_header + write, src/writer/filesystem_writer.cpp:606-651)."""
        cfgs = {self._config(metadata, len(b)) for b in blocks}
        if not blocks:
            return b""
        cfg = cfgs.pop()
        n = [len(b) // 2 for b in blocks]
        offs = np.zeros(len(blocks), np.int64)
        for i in range(1, len(blocks)):
            offs[i] = offs[i - 1] + (n[i - 1] + 7) // 8 * 8
        flat = np.zeros(int(offs[-1] + n[-1]) + 8, np.uint16)
        for o, b in zip(offs, blocks):
            flat[o:o + len(b) // 2] = np.frombuffer(b, np.uint16)
        d = torch.from_numpy(flat.view(np.int16)).to(self.device)
        res = encode_batch(cfg, d, offs, n)
        frames = [frame_header(len(b), self.block_size, cfg.component_stream_count, 2, cfg.unused_lsb_count,
                               cfg.byteorder == "big") for b in blocks]
        d_fr, d_fl = S._rows(frames, S.FRAME_ROW, self.device)
        headers = S.section_headers_batch(res.data, res.d_offsets, res.sizes, first_number, S.SECTION_TYPE_BLOCK,
                                          COMPRESSION_TYPE_RICEPP, d_fr, d_fl)
        capacity = res.data.numel() + len(blocks) * (S.HEADER_BYTES + S.FRAME_ROW)
        asm = S.sections_assemble_batch(headers, res.data, res.d_offsets, res.sizes, capacity, d_fr, d_fl)
        torch.cuda.current_stream().synchronize()
        res.check()
        return asm.bytes()


class RiceppBlockDecompressor:
    """``ricepp_block_decompressor`` (src/compression/ricepp.cpp:184-255)."""

    def __init__(self, data: bytes, device="cuda"):
        f, n = parse_frame(data)
        if f.ricepp_version > RICEPP_VERSION:
            raise RuntimeError(f"[RICEPP] unsupported version: {f.ricepp_version}")
        self.config = CodecConfig(f.block_size, f.component_count, "big" if f.big_endian else "little",
                                  f.unused_lsb_count)
        _check(self.config)
        if f.bytes_per_sample != 2:
            raise RuntimeError(f"[RICEPP] unsupported bytes per sample: {f.bytes_per_sample}")
        self.frame = f
        self.data = data[n:]
        self.device = torch.device(device)
        self._target: Optional[bytearray] = None
        self._done = False

    def type(self) -> int:
        return COMPRESSION_TYPE_RICEPP

    def uncompressed_size(self) -> int:
        return int(self.frame.uncompressed_bytes)

    def metadata(self) -> str:
        return json.dumps({
            "bytes_per_sample": int(self.frame.bytes_per_sample),
            "component_count": int(self.frame.component_count),
            "endianness": "big" if self.frame.big_endian else "little",
            "unused_lsb_count": int(self.frame.unused_lsb_count),
        }, separators=(",", ":"))

    def start_decompression(self, target: bytearray) -> None:
        self._target = target

    def decompress_frame(self, frame_size: int = 0) -> bool:
        if self._target is None:
            raise RuntimeError("decompression not started")
        if self._done:
            return False
        out = decompress_many([self], self.device)[0]
        self._target[:] = out
        self._done = True
        return True


def decompress(data: bytes, device="cuda") -> bytes:
    """``block_decompressor::decompress`` (src/block_decompressor.cpp:41-49)."""
    return decompress_many([RiceppBlockDecompressor(data, device)], device)[0]


def decompress_many(decs: Sequence[RiceppBlockDecompressor], device="cuda") -> List[bytes]:
    """Decodes many ricepp blocks with one launch per distinct config."""
    dev = torch.device(device)
    out: List[Optional[bytes]] = [None] * len(decs)
    groups = {}
    for i, d in enumerate(decs):
        groups.setdefault(d.config, []).append(i)
    for cfg, idx in groups.items():
        offs = np.zeros(len(idx), np.int64)
        lens = [len(decs[i].data) for i in idx]
        for k in range(1, len(idx)):
            offs[k] = offs[k - 1] + (lens[k - 1] + 15) // 16 * 16
        buf = np.zeros(int(offs[-1] + lens[-1]) + 32, np.uint8)
        for o, i in zip(offs, idx):
            buf[o:o + len(decs[i].data)] = np.frombuffer(decs[i].data, np.uint8)
        ns = [decs[i].uncompressed_size() // 2 for i in idx]
        samples, status = decode_batch(cfg, torch.from_numpy(buf).to(dev), offs, lens, ns)
        torch.cuda.current_stream().synchronize()
        st = status.cpu().numpy()
        host = samples.cpu().numpy().view(np.uint16)
        pos = 0
        for k, i in enumerate(idx):
            _raise_status(int(st[k]))
            out[i] = host[pos:pos + ns[k]].tobytes()
            pos += ns[k]
    return out  # type: ignore[return-value]


def compress_many_sections(blocks: Sequence[bytes], metadata: Optional[str], first_number: int = 0,
                           block_size: int = 128, device="cuda") -> bytes:
    """``RiceppBlockCompressor(block_size).compress_many_sections``: image-ready BLOCK sections of one batch."""
    return RiceppBlockCompressor(block_size, device).compress_many_sections(blocks, metadata, first_number)


def decompress_sections(image: bytes, verify: int = 1, device="cuda") -> List[bytes]:
    """Decodes the BLOCK sections of an image fragment: ricepp (as ``compress_many_sections`` writes them), LZ4
    and LZ4HC, NONE, and ZSTD as a stock ``mkdwarfs`` writes them (one Zstandard frame per section; their block
    counts come from the host copy).  Any other compression (lzma, brotli, flac) raises.

    The headers are walked on the host, the image goes to the device in one copy, and the integrity check
    (``verify`` 1: XXH3-64 as cached_block's check_fast, src/reader/internal/cached_block.cpp:58-67; 2: also
    SHA-512/256; 0: none) and the decode run on the same stream from that copy.  A section that fails raises
    ``RuntimeError("block data integrity check failed")`` like the reference, before anything is decoded."""
    dev = torch.device(device)
    image = bytes(image)
    secs, bad_at = S.walk(image)
    if verify not in (0, 1, 2):
        raise ValueError("verify must be 0, 1 or 2")
    if bad_at is not None and not verify:
        raise RuntimeError(S.INTEGRITY_ERROR)
    if not secs and bad_at is None:
        return []
    padded = np.zeros(len(image) + 64, np.uint8)  # (the decoder reads whole 16-byte granules)
    padded[:len(image)] = np.frombuffer(image, np.uint8)
    d_image = torch.from_numpy(padded).to(dev)
    if verify:
        offsets = [at for at, _ in secs] + ([bad_at] if bad_at is not None else [])
        status = S.sections_verify_batch(d_image, len(image), offsets, verify)
        if int(status.abs().sum().item()) != 0:
            raise RuntimeError(S.INTEGRITY_ERROR)
    decs, groups = [], {}
    out: List[Optional[bytes]] = [None] * len(secs)
    lz4_secs, zstd_secs = [], []
    for i, (at, h) in enumerate(secs):
        if h.type == S.SECTION_TYPE_BLOCK and h.compression == Z.COMPRESSION_TYPE_NONE:
            out[i] = image[at + S.HEADER_BYTES:at + S.HEADER_BYTES + int(h.length)]  # stored as it is
            decs.append(None)
            continue
        if h.type == S.SECTION_TYPE_BLOCK and h.compression in (Z.COMPRESSION_TYPE_LZ4, Z.COMPRESSION_TYPE_LZ4HC):
            lz4_secs.append((i, at + S.HEADER_BYTES, int(h.length)))
            decs.append(None)
            continue
        if h.type == S.SECTION_TYPE_BLOCK and h.compression == ZS.COMPRESSION_TYPE_ZSTD:
            zstd_secs.append((i, at + S.HEADER_BYTES, int(h.length)))
            decs.append(None)
            continue
        if h.type != S.SECTION_TYPE_BLOCK or h.compression != COMPRESSION_TYPE_RICEPP:
            raise RuntimeError(f"section {h.number}: not a ricepp, lz4, zstd or uncompressed block "
                               f"(type {h.type}, compression {h.compression})")
        dec =RiceppBlockDecompressor(image[at + S.HEADER_BYTES:at + S.HEADER_BYTES + min(int(h.length), 64)], dev)
        hdr_len = min(int(h.length), 64) - len(dec.data)
        decs.append((dec, at + S.HEADER_BYTES + hdr_len, int(h.length) - hdr_len))
        groups.setdefault(dec.config, []).append(i)
    if lz4_secs:  # LZ4 and LZ4HC decode alike: one launch, straight from the image on the device
        sizes = [Z.parse_frame(image[at:at + length])[0] for _, at, length in lz4_secs]
        plain, offs, st = Z.decode_batch(d_image, [at + Z.FRAME_BYTES for _, at, _ in lz4_secs],
                                         [length - Z.FRAME_BYTES for _, _, length in lz4_secs], sizes)
        torch.cuda.current_stream().synchronize()
        host = plain.cpu().numpy()
        for (i, _, _), o, n, s in zip(lz4_secs, offs, sizes, st.cpu().numpy()):
            Z.raise_decode_status(int(s))
            out[i] = host[o:o + n].tobytes()
    if zstd_secs:  # one batch, straight from the image on the device
        frames = [ZS.ZstdBlockDecompressor(image[at:at + length], dev) for _, at, length in zstd_secs]
        sizes = [f.uncompressed_size() for f in frames]
        blocks = [ZS.count_blocks(f.data) for f in frames]
        for b in blocks:
            ZS.raise_decode_status(min(b, 0))
        plain, offs, st = ZS.decode_batch(d_image, [at for _, at, _ in zstd_secs],
                                          [length for _, _, length in zstd_secs], sizes, sum(blocks))
        torch.cuda.current_stream().synchronize()
        host = plain.cpu().numpy()
        for (i, _, _), o, n, s in zip(zstd_secs, offs, sizes, st.cpu().numpy()):
            ZS.raise_decode_status(int(s))
            out[i] = host[o:o + n].tobytes()
    for cfg, idx in groups.items():
        ns = [decs[i][0].uncompressed_size() // 2 for i in idx]
        samples, st = decode_batch(cfg, d_image, [decs[i][1] for i in idx], [decs[i][2] for i in idx], ns)
        torch.cuda.current_stream().synchronize()
        st = st.cpu().numpy()
        host = samples.cpu().numpy().view(np.uint16)
        pos = 0
        for k, i in enumerate(idx):
            _raise_status(int(st[k]))
            out[i] = host[pos:pos + ns[k]].tobytes()
            pos += ns[k]
    return out  # type: ignore[return-value]


def decode_sections_device(image: bytes, verify: int = 1, device="cuda"):
    """What :func:`decompress_sections` does (the same sections, the same integrity check, the same errors), but the
    decoded blocks stay on the device: ``(blocks, block_offsets, block_sizes)`` -- one uint8 device buffer on a
    16-byte boundary, padded to a multiple of 16 bytes, in which block b is ``blocks[block_offsets[b] :
    block_offsets[b] + block_sizes[b]]`` (int64 device tensors; every block starts on a 16-byte boundary), ready for
    ``extract.gather_files``.  The ricepp, LZ4 and ZSTD batches decode straight into their places in that buffer;
    a NONE section is a device-to-device copy out of the uploaded image.  FLAC, lzma and brotli sections raise."""
    dev = torch.device(device)
    image = bytes(image)
    secs, bad_at = S.walk(image)
    if verify not in (0, 1, 2):
        raise ValueError("verify must be 0, 1 or 2")
    if bad_at is not None and not verify:
        raise RuntimeError(S.INTEGRITY_ERROR)
    padded = np.zeros(len(image) + 64, np.uint8)  # (the decoder reads whole 16-byte granules)
    padded[:len(image)] = np.frombuffer(image, np.uint8)
    d_image = torch.from_numpy(padded).to(dev)
    if verify and (secs or bad_at is not None):
        offsets = [at for at, _ in secs] + ([bad_at] if bad_at is not None else [])
        status = S.sections_verify_batch(d_image, len(image), offsets, verify)
        if int(status.abs().sum().item()) != 0:
            raise RuntimeError(S.INTEGRITY_ERROR)
    sizes = [0] * len(secs)
    none_secs, lz4_secs, zstd_secs, groups = [], [], [], {}
    for i, (at, h) in enumerate(secs):
        at, length = at + S.HEADER_BYTES, int(h.length)
        if h.type == S.SECTION_TYPE_BLOCK and h.compression == Z.COMPRESSION_TYPE_NONE:
            none_secs.append((i, at))
            sizes[i] = length
        elif h.type == S.SECTION_TYPE_BLOCK and h.compression in (Z.COMPRESSION_TYPE_LZ4, Z.COMPRESSION_TYPE_LZ4HC):
            lz4_secs.append((i, at + Z.FRAME_BYTES, length - Z.FRAME_BYTES))
            sizes[i] = Z.parse_frame(image[at:at + length])[0]
        elif h.type == S.SECTION_TYPE_BLOCK and h.compression == ZS.COMPRESSION_TYPE_ZSTD:
            frame = ZS.ZstdBlockDecompressor(image[at:at + length], dev)
            nblocks = ZS.count_blocks(frame.data)
            ZS.raise_decode_status(min(nblocks, 0))
            zstd_secs.append((i, at, length, nblocks))
            sizes[i] = frame.uncompressed_size()
        elif h.type == S.SECTION_TYPE_BLOCK and h.compression == COMPRESSION_TYPE_RICEPP:
            dec = RiceppBlockDecompressor(image[at:at + min(length, 64)], dev)
            hdr_len = min(length, 64) - len(dec.data)
            groups.setdefault(dec.config, []).append((i, at + hdr_len, length - hdr_len))
            sizes[i] = dec.uncompressed_size()
        else:
            raise RuntimeError(f"section {h.number}: not a ricepp, lz4, zstd or uncompressed block "
                               f"(type {h.type}, compression {h.compression})")
    offs, total = Z._layout(sizes)
    blocks = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
    pending = []  # (status tensor, how its entries raise)
    for i, at in none_secs:
        blocks[int(offs[i]):int(offs[i]) + sizes[i]] = d_image[at:at + sizes[i]]
    if lz4_secs:
        idx = [i for i, _, _ in lz4_secs]
        _, _, st = Z.decode_batch(d_image, [at for _, at, _ in lz4_secs], [n for _, _, n in lz4_secs],
                                  [sizes[i] for i in idx], out=blocks, out_offsets=offs[idx])
        pending.append((st, Z.raise_decode_status))
    if zstd_secs:
        idx = [i for i, _, _, _ in zstd_secs]
        _, _, st = ZS.decode_batch(d_image, [at for _, at, _, _ in zstd_secs], [n for _, _, n, _ in zstd_secs],
                                   [sizes[i] for i in idx], sum(b for _, _, _, b in zstd_secs), out=blocks,
                                   out_offsets=offs[idx])
        pending.append((st, ZS.raise_decode_status))
    for cfg, rows in groups.items():
        idx = [i for i, _, _ in rows]
        _, st = decode_batch(cfg, d_image, [at for _, at, _ in rows], [n for _, _, n in rows],
                             [sizes[i] // 2 for i in idx], out=blocks.view(torch.int16), out_offsets=offs[idx] // 2)
        pending.append((st, _raise_status))
    torch.cuda.current_stream().synchronize()
    for st, raise_status in pending:
        for s in st.cpu().numpy():
            raise_status(int(s))
    return blocks, torch.from_numpy(offs).to(dev), torch.as_tensor(np.asarray(sizes, np.int64), device=dev)


class NullBlockCompressor:
    """``null_block_compressor`` (src/compression/null.cpp): compression type NONE, the bytes as they are."""

    def clone(self) -> "NullBlockCompressor":
        return NullBlockCompressor()

    def type(self) -> int:
        return Z.COMPRESSION_TYPE_NONE

    def describe(self) -> str:
        return "null"

    def metadata_requirements(self) -> str:
        return ""

    def compress(self, data: bytes, metadata: Optional[str] = None) -> bytes:
        return bytes(data)

    def compress_many(self, blocks: Sequence[bytes], metadata: Optional[str] = None) -> List[bytes]:
        return [bytes(b) for b in blocks]


def block_compressor(spec: str, device="cuda"):
    """``block_compressor(spec)`` for ``ricepp[:block_size=N]``, ``lz4``, ``lz4hc[:level=N]`` and ``null``
    (src/compressor_registry.cpp:50-59).  ``lz4`` and ``lz4hc`` also take ``depth=N`` (1, 2, 4, 8) and
    ``lazy=0|1``, which make the encoder's search word (``lz4hc:level=9:depth=8:lazy=1``); ``level`` maps to no
    search."""
    name, _, opts = spec.partition(":")
    if name in ("lz4", "lz4hc", "null"):
        level = [9 if name == "lz4hc" else None]  # lz4.cpp's default level

        def take_level(k, v):
            if name != "lz4hc" or k != "level" or not v.isdigit() or int(v) > 12:
                return False
            level[0] = int(v)
            return True

        kvs = [kv for kv in opts.replace(",", ":").split(":") if kv]
        if name == "null":
            for kv in kvs:
                raise RuntimeError(f"invalid option(s) for {name}: {kv}")
            return NullBlockCompressor()
        search = Z.spec_search(kvs, name, take_level)
        return Z.Lz4BlockCompressor(level[0], device, search)
    if name != "ricepp":
        raise RuntimeError(f"unknown compression: {name}")
    bs = 128
    for kv in filter(None, opts.split(",")):
        k, eq, v = kv.partition("=")
        if k != "block_size" or not eq:
            raise RuntimeError(f"invalid option(s) for ricepp: {kv}")
        bs = int(v)
    return RiceppBlockCompressor(bs, device)
