"""Loader for the native MI355X ricepp library (libricepp_amd.so).

The library exports exactly the C ABI of ``include/ricepp_amd.h``.  There is
no fallback: if the library is missing or fails to load, every entry point
raises, so a GPU run can never silently pass on a non-native path.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("RICEPP_AMD_LIB", PKG / "lib" / "libricepp_amd.so"))

RPP_OK = 0
RPP_UNSUPPORTED_CONFIG = -1
RPP_TRUNCATED_INPUT = -2
RPP_INVALID_ARGUMENT = -3
RPP_OUTPUT_TOO_SMALL = -4
RPP_HIP_ERROR = -5
RPP_INTERNAL_ERROR = -6
RPP_CHECKSUM_MISMATCH = -7
RPP_CORRUPT_INPUT = -8
RPP_BAD_CHUNK = -9
RPP_CHUNK_HOLE = 0xFFFFFFFF  # rpp_chunk.block of a hole

RPP_DECODE_AUTO = 0
RPP_DECODE_FUSED = 1
RPP_DECODE_SEGMENTED = 2
RPP_TEST_NO_FAST_LANES = 1
RPP_TEST_LOOKBACK_STALL = 2
RPP_TEST_PHASE_TIMERS = 4

STATUS_NAMES = {
    RPP_OK: "OK",
    RPP_UNSUPPORTED_CONFIG: "UNSUPPORTED_CONFIG",
    RPP_TRUNCATED_INPUT: "TRUNCATED_INPUT",
    RPP_INVALID_ARGUMENT: "INVALID_ARGUMENT",
    RPP_OUTPUT_TOO_SMALL: "OUTPUT_TOO_SMALL",
    RPP_HIP_ERROR: "HIP_ERROR",
    RPP_INTERNAL_ERROR: "INTERNAL_ERROR",
    RPP_CHECKSUM_MISMATCH: "CHECKSUM_MISMATCH",
    RPP_CORRUPT_INPUT: "CORRUPT_INPUT",
    RPP_BAD_CHUNK: "BAD_CHUNK",
}

# Every symbol declared in include/ricepp_amd.h.
EXPORTED_SYMBOLS = (
    "rpp_abi_version",
    "rpp_check_config",
    "rpp_worst_case_bytes",
    "rpp_encode_batch",
    "rpp_encode_workspace_bytes",
    "rpp_encode_batch_ws",
    "rpp_decode_batch",
    "rpp_decode_workspace_bytes",
    "rpp_decode_batch_ws",
    "rpp_decode_workspace_bytes_ex",
    "rpp_decode_batch_ex",
    "rpp_unused_lsb_batch",
    "rpp_exclusive_scan_u64",
    "rpp_pack_batch",
    "rpp_frame_header",
    "rpp_parse_frame",
    "rpp_pcm_check_format",
    "rpp_pcm_unpack",
    "rpp_pcm_pack",
    "rpp_flac_frame_header",
    "rpp_flac_parse_frame",
    "rpp_flac_stream_header",
    "rpp_flac_parse_stream",
    "rpp_flac_frame_bound",
    "rpp_flac_encode_workspace_bytes",
    "rpp_flac_encode",
    "rpp_flac_encode_ex",
    "rpp_flac_encode_batch_workspace_bytes",
    "rpp_flac_encode_batch",
    "rpp_flac_decode_workspace_bytes",
    "rpp_flac_decode",
    "rpp_flac_decode_batch_workspace_bytes",
    "rpp_flac_decode_batch",
    "rpp_xxh3_64_batch",
    "rpp_sha512_256_batch",
    "rpp_section_headers_batch",
    "rpp_sections_assemble_batch",
    "rpp_sections_verify_batch",
    "rpp_parse_section_header",
    "rpp_file_hash_algo",
    "rpp_file_hash_digest_bytes",
    "rpp_xxh3_128_batch",
    "rpp_file_hash_batch",
    "rpp_group_workspace_bytes",
    "rpp_group_first_batch",
    "rpp_group_start_slot",
    "rpp_file_dedup_workspace_bytes",
    "rpp_file_dedup_batch",
    "rpp_similarity_kind",
    "rpp_similarity_state_bytes",
    "rpp_similarity_digest_bytes",
    "rpp_similarity_chunk_bytes",
    "rpp_similarity_update_batch",
    "rpp_similarity_finalize_batch",
    "rpp_similarity_hash_workspace_bytes",
    "rpp_similarity_hash_batch",
    "rpp_similarity_host_update",
    "rpp_similarity_host_finalize",
    "rpp_segment_check_config",
    "rpp_segment_tile_frames",
    "rpp_segment_positions",
    "rpp_segment_index_slots",
    "rpp_segment_hash_workspace_bytes",
    "rpp_segment_hash_batch",
    "rpp_segment_scan_workspace_bytes",
    "rpp_segment_scan_batch",
    "rpp_segment_index_workspace_bytes",
    "rpp_segment_index_batch",
    "rpp_segment_extend_batch",
    "rpp_segment_host_hashes",
    "rpp_segment_host_index",
    "rpp_segment_host_scan",
    "rpp_segment_host_extend",
    "rpp_order_check_options",
    "rpp_order_split_pass_children",
    "rpp_order_chain_threads",
    "rpp_order_chain_stage_rows",
    "rpp_order_split_workspace_bytes",
    "rpp_order_split_batch",
    "rpp_order_chain_workspace_bytes",
    "rpp_order_chain_batch",
    "rpp_order_host_split",
    "rpp_order_host_chain",
    "rpp_order_host_nilsimsa",
    "rpp_lz4_bound",
    "rpp_lz4_chunk_bytes",
    "rpp_lz4_step_positions",
    "rpp_lz4_frame_header",
    "rpp_lz4_parse_frame",
    "rpp_lz4_decode_batch",
    "rpp_lz4_encode_workspace_bytes",
    "rpp_lz4_encode_batch",
    "rpp_lz4_host_decode",
    "rpp_lz4_host_encode",
    "rpp_zstd_frame_info",
    "rpp_zstd_count_blocks",
    "rpp_zstd_decode_workspace_bytes",
    "rpp_zstd_decode_batch",
    "rpp_zstd_host_decode",
    "rpp_zstd_bound",
    "rpp_zstd_encode_workspace_bytes",
    "rpp_zstd_encode_batch",
    "rpp_zstd_host_encode",
    "rpp_zstd_encode_batch_opt",
    "rpp_zstd_host_encode_opt",
    "rpp_lz4_encode_batch_search",
    "rpp_lz4_host_encode_search",
    "rpp_zstd_encode_batch_search",
    "rpp_zstd_host_encode_search",
    "rpp_incompressible_workspace_bytes",
    "rpp_incompressible_scan_batch",
    "rpp_incompressible_host_scan",
    "rpp_zstd_encode_workspace_bytes_long",
    "rpp_zstd_encode_batch_long",
    "rpp_zstd_host_encode_long",
    "rpp_zstd_host_long_sequences",
    "rpp_incompressible_workspace_bytes_long",
    "rpp_incompressible_scan_batch_long",
    "rpp_incompressible_host_scan_long",
    "rpp_extract_tile_bytes",
    "rpp_extract_workspace_bytes",
    "rpp_extract_gather_batch",
    "rpp_extract_host_gather",
    "rpp_digest_algo",
    "rpp_digest_bytes",
    "rpp_digest_batch",
    "rpp_digest_host",
)

RPP_HASH_XXH3_64 = 0
RPP_HASH_XXH3_128 = 1
RPP_HASH_SHA512_256 = 2

RPP_ZSTD_ENC_TABLES = 1  # the options word of rpp_zstd_encode_batch_opt / rpp_zstd_host_encode_opt
RPP_ZSTD_ENC_REPEAT = 2
RPP_SEARCH_LAZY = 0x100  # the search word of the *_search calls: depth (1, 2, 4, 8) | RPP_SEARCH_LAZY
RPP_ZSTD_LONG_MAX_BLOCK = 1 << 27  # a block's largest size under the `long` word of the *_long calls

RPP_SIMILARITY_NILSIMSA = 0
RPP_SIMILARITY_HISTOGRAM = 1


class RppConfig(C.Structure):
    """``rpp_config`` (mirrors ricepp::codec_config, codec_config.h:36-41)."""

    _fields_ = [
        ("block_size", C.c_uint32),
        ("component_stream_count", C.c_uint32),
        ("big_endian", C.c_uint32),
        ("unused_lsb_count", C.c_uint32),
    ]


class RppDecodeOptions(C.Structure):
    """``rpp_decode_options`` (explicit decode path selection, tests and diagnostics)."""

    _fields_ = [
        ("path", C.c_uint32),
        ("seg_log2", C.c_uint32),
        ("fused_waves", C.c_uint32),
        ("test_flags", C.c_uint32),
    ]


class RppFrame(C.Structure):
    _fields_ = [
        ("uncompressed_bytes", C.c_uint64),
        ("block_size", C.c_uint32),
        ("component_count", C.c_uint32),
        ("bytes_per_sample", C.c_uint32),
        ("unused_lsb_count", C.c_uint32),
        ("big_endian", C.c_uint32),
        ("ricepp_version", C.c_uint32),
    ]


class RppFlacFrame(C.Structure):
    """``rpp_flac_frame`` (the flac_block_header fields, thrift/compression.thrift:36-40)."""

    _fields_ = [
        ("uncompressed_bytes", C.c_uint64),
        ("num_channels", C.c_uint32),
        ("bits_per_sample", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class RppFlacStreamInfo(C.Structure):
    _fields_ = [
        ("min_blocksize", C.c_uint32),
        ("max_blocksize", C.c_uint32),
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("bits_per_sample", C.c_uint32),
        ("total_samples", C.c_uint64),
    ]


class RppPcmFormat(C.Structure):
    """``rpp_pcm_format`` (pcm_sample_transformer's constructor arguments,
    include/dwarfs/pcm_sample_transformer.h:36-45)."""

    _fields_ = [
        ("big_endian", C.c_uint32),
        ("is_signed", C.c_uint32),
        ("lsb_padded", C.c_uint32),
        ("bytes", C.c_uint32),
        ("bits", C.c_uint32),
    ]


class RppSectionHeader(C.Structure):
    """``rpp_section_header`` (section_header_v2's fields, include/dwarfs/fstypes.h:85-97)."""

    _fields_ = [
        ("sha2_512_256", C.c_uint8 * 32),
        ("xxh3_64", C.c_uint64),
        ("length", C.c_uint64),
        ("number", C.c_uint32),
        ("type", C.c_uint16),
        ("compression", C.c_uint16),
        ("major", C.c_uint8),
        ("minor", C.c_uint8),
    ]


class RppSegmentConfig(C.Structure):
    """``rpp_segment_config``."""

    _fields_ = [
        ("window_bits", C.c_uint32),
        ("increment_shift", C.c_uint32),
        ("granularity", C.c_uint32),
        ("reserved", C.c_uint32),
        ("filter_bits", C.c_uint64),
    ]


class RppSegmentScanResult(C.Structure):
    _fields_ = [("count", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_uint32)]


class RppChunk(C.Structure):
    """``rpp_chunk``: a file's chunk row (block ``RPP_CHUNK_HOLE``: a hole of ``size`` bytes)."""

    _fields_ = [("block", C.c_uint32), ("offset", C.c_uint32), ("size", C.c_uint64)]


class RppOrderStats(C.Structure):
    """``rpp_order_stats``."""

    _fields_ = [
        ("fallbacks", C.c_uint64),
        ("fallback_ties", C.c_uint64),
        ("chain_early_stops", C.c_uint64),
        ("depth", C.c_uint32),
        ("leaves", C.c_uint32),
        ("largest_leaf", C.c_uint32),
        ("largest_final_leaf", C.c_uint32),
        ("largest_node", C.c_uint32),
        ("duplicate_groups", C.c_uint32),
        ("unique", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


_lib = None


def lib() -> C.CDLL:
    """Returns the loaded native library; raises if it is not built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"native ricepp library not found at {LIB_PATH}; run `python __graft_entry__.py build`"
            )
        L = C.CDLL(str(LIB_PATH))
        P = C.c_void_p
        L.rpp_abi_version.restype = C.c_uint32
        L.rpp_check_config.argtypes = [C.POINTER(RppConfig)]
        L.rpp_check_config.restype = C.c_int
        L.rpp_worst_case_bytes.argtypes = [C.POINTER(RppConfig), C.c_uint64]
        L.rpp_worst_case_bytes.restype = C.c_uint64
        L.rpp_encode_batch.argtypes = [C.POINTER(RppConfig), P, P, P, C.c_uint32, P, P, P, P, P]
        L.rpp_encode_batch.restype = C.c_int
        L.rpp_encode_workspace_bytes.argtypes = [C.POINTER(RppConfig), C.c_uint64, C.c_uint64, C.c_uint32]
        L.rpp_encode_workspace_bytes.restype = C.c_uint64
        L.rpp_encode_batch_ws.argtypes = [C.POINTER(RppConfig), P, P, P, C.c_uint32, P, P, P, P, C.c_uint64,
                                          C.c_uint64, P, C.c_uint64, P]
        L.rpp_encode_batch_ws.restype = C.c_int
        L.rpp_decode_batch.argtypes = [C.POINTER(RppConfig), P, P, P, C.c_uint32, P, P, P, P, P]
        L.rpp_decode_batch.restype = C.c_int
        L.rpp_decode_workspace_bytes.argtypes = [C.POINTER(RppConfig), C.c_uint64, C.c_uint64, C.c_uint32]
        L.rpp_decode_workspace_bytes.restype = C.c_uint64
        L.rpp_decode_batch_ws.argtypes = [C.POINTER(RppConfig), P, P, P, C.c_uint32, P, P, P, P, C.c_uint64,
                                          C.c_uint64, P, C.c_uint64, P]
        L.rpp_decode_batch_ws.restype = C.c_int
        L.rpp_decode_workspace_bytes_ex.argtypes = [C.POINTER(RppConfig), C.c_uint64, C.c_uint64, C.c_uint32,
                                                    C.POINTER(RppDecodeOptions)]
        L.rpp_decode_workspace_bytes_ex.restype = C.c_uint64
        L.rpp_decode_batch_ex.argtypes = [C.POINTER(RppConfig), P, P, P, C.c_uint32, P, P, P, P, C.c_uint64,
                                          C.c_uint64, P, C.c_uint64, C.POINTER(RppDecodeOptions), P]
        L.rpp_decode_batch_ex.restype = C.c_int
        L.rpp_unused_lsb_batch.argtypes = [P, P, P, C.c_uint64, C.c_uint32, C.c_uint32, P, P, P]
        L.rpp_unused_lsb_batch.restype = C.c_int
        L.rpp_exclusive_scan_u64.argtypes = [P, C.c_uint64, P, P]
        L.rpp_exclusive_scan_u64.restype = C.c_int
        L.rpp_pack_batch.argtypes = [P, P, P, C.c_uint32, P, P, P, P]
        L.rpp_pack_batch.restype = C.c_int
        L.rpp_frame_header.argtypes = [C.POINTER(RppFrame), P]
        L.rpp_frame_header.restype = C.c_size_t
        L.rpp_parse_frame.argtypes = [P, C.c_size_t, C.POINTER(RppFrame)]
        L.rpp_parse_frame.restype = C.c_long
        L.rpp_pcm_check_format.argtypes = [C.POINTER(RppPcmFormat)]
        L.rpp_pcm_check_format.restype = C.c_int
        L.rpp_pcm_unpack.argtypes = [C.POINTER(RppPcmFormat), P, P, C.c_uint64, P]
        L.rpp_pcm_unpack.restype = C.c_int
        L.rpp_pcm_pack.argtypes = [C.POINTER(RppPcmFormat), P, P, C.c_uint64, P]
        L.rpp_pcm_pack.restype = C.c_int
        L.rpp_flac_frame_header.argtypes = [C.POINTER(RppFlacFrame), P]
        L.rpp_flac_frame_header.restype = C.c_size_t
        L.rpp_flac_parse_frame.argtypes = [P, C.c_size_t, C.POINTER(RppFlacFrame)]
        L.rpp_flac_parse_frame.restype = C.c_long
        L.rpp_flac_stream_header.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, P]
        L.rpp_flac_stream_header.restype = C.c_size_t
        L.rpp_flac_parse_stream.argtypes = [P, C.c_size_t, C.POINTER(RppFlacStreamInfo)]
        L.rpp_flac_parse_stream.restype = C.c_long
        L.rpp_flac_frame_bound.argtypes = [C.c_uint32, C.c_uint32]
        L.rpp_flac_frame_bound.restype = C.c_uint64
        L.rpp_flac_encode_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.rpp_flac_encode_workspace_bytes.restype = C.c_uint64
        L.rpp_flac_encode.argtypes = [P, C.c_uint64, C.c_uint32, C.c_uint32, P, P, P, C.c_uint64, P]
        L.rpp_flac_encode.restype = C.c_int
        L.rpp_flac_encode_ex.argtypes = [P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P,
                                         C.c_uint64, P]
        L.rpp_flac_encode_ex.restype = C.c_int
        L.rpp_flac_encode_batch_workspace_bytes.argtypes = [C.c_uint32, P, P, P]
        L.rpp_flac_encode_batch_workspace_bytes.restype = C.c_uint64
        L.rpp_flac_encode_batch.argtypes = [P, C.c_uint32, P, P, P, P, C.c_uint32, C.c_uint32, P, P, P, C.c_uint64, P]
        L.rpp_flac_encode_batch.restype = C.c_int
        L.rpp_flac_decode_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.rpp_flac_decode_workspace_bytes.restype = C.c_uint64
        L.rpp_flac_decode.argtypes = [P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, P, P,
                                      C.c_uint32, P, C.c_uint64, P, P]
        L.rpp_flac_decode.restype = C.c_int
        L.rpp_flac_decode_batch_workspace_bytes.argtypes = [C.c_uint32, P, P, P, P, P]
        L.rpp_flac_decode_batch_workspace_bytes.restype = C.c_uint64
        L.rpp_flac_decode_batch.argtypes = [P, C.c_uint32, P, P, P, P, P, P, P, P, P, P, P, C.c_uint64, P, P]
        L.rpp_flac_decode_batch.restype = C.c_int
        L.rpp_xxh3_64_batch.argtypes = [P, P, P, C.c_uint32, P, P, P, P]
        L.rpp_xxh3_64_batch.restype = C.c_int
        L.rpp_sha512_256_batch.argtypes = [P, P, P, C.c_uint32, P, P, P, P]
        L.rpp_sha512_256_batch.restype = C.c_int
        L.rpp_section_headers_batch.argtypes = [P, P, P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P]
        L.rpp_section_headers_batch.restype = C.c_int
        L.rpp_sections_assemble_batch.argtypes = [P, P, P, P, P, P, C.c_uint32, P, P, P, P, P]
        L.rpp_sections_assemble_batch.restype = C.c_int
        L.rpp_sections_verify_batch.argtypes = [P, C.c_uint64, P, C.c_uint32, C.c_uint32, P, P]
        L.rpp_sections_verify_batch.restype = C.c_int
        L.rpp_parse_section_header.argtypes = [P, C.POINTER(RppSectionHeader)]
        L.rpp_parse_section_header.restype = C.c_int
        L.rpp_file_hash_algo.argtypes = [C.c_char_p]
        L.rpp_file_hash_algo.restype = C.c_int
        L.rpp_file_hash_digest_bytes.argtypes = [C.c_int]
        L.rpp_file_hash_digest_bytes.restype = C.c_int
        L.rpp_xxh3_128_batch.argtypes = [P, P, P, C.c_uint32, P, P, P, P]
        L.rpp_xxh3_128_batch.restype = C.c_int
        L.rpp_file_hash_batch.argtypes = [C.c_int, P, P, P, P, C.c_uint32, P, P]
        L.rpp_file_hash_batch.restype = C.c_int
        L.rpp_group_workspace_bytes.argtypes = [C.c_uint32]
        L.rpp_group_workspace_bytes.restype = C.c_uint64
        L.rpp_group_first_batch.argtypes = [P, P, C.c_uint32, P, C.c_uint32, P, P, P, C.c_uint64, P]
        L.rpp_group_first_batch.restype = C.c_int
        L.rpp_group_start_slot.argtypes = [C.c_uint64, P, C.c_uint32, C.c_uint32]
        L.rpp_group_start_slot.restype = C.c_uint64
        L.rpp_file_dedup_workspace_bytes.argtypes = [C.c_uint32]
        L.rpp_file_dedup_workspace_bytes.restype = C.c_uint64
        L.rpp_file_dedup_batch.argtypes = [C.c_int, P, P, P, C.c_uint32, P, P, P, P, C.c_uint64, P]
        L.rpp_file_dedup_batch.restype = C.c_int
        L.rpp_similarity_kind.argtypes = [C.c_char_p]
        L.rpp_similarity_kind.restype = C.c_int
        L.rpp_similarity_state_bytes.argtypes = [C.c_int]
        L.rpp_similarity_state_bytes.restype = C.c_uint64
        L.rpp_similarity_digest_bytes.argtypes = [C.c_int]
        L.rpp_similarity_digest_bytes.restype = C.c_int
        L.rpp_similarity_chunk_bytes.argtypes = []
        L.rpp_similarity_chunk_bytes.restype = C.c_uint64
        L.rpp_similarity_update_batch.argtypes = [C.c_int, P, P, P, P, C.c_uint32, P, P]
        L.rpp_similarity_update_batch.restype = C.c_int
        L.rpp_similarity_finalize_batch.argtypes = [C.c_int, P, P, C.c_uint32, P, P]
        L.rpp_similarity_finalize_batch.restype = C.c_int
        L.rpp_similarity_hash_workspace_bytes.argtypes = [C.c_int, C.c_uint32]
        L.rpp_similarity_hash_workspace_bytes.restype = C.c_uint64
        L.rpp_similarity_hash_batch.argtypes = [C.c_int, P, P, P, P, C.c_uint64, C.c_uint32, P, P, P, C.c_uint64, P]
        L.rpp_similarity_hash_batch.restype = C.c_int
        L.rpp_similarity_host_update.argtypes = [C.c_int, P, P, C.c_uint64]
        L.rpp_similarity_host_update.restype = C.c_int
        L.rpp_similarity_host_finalize.argtypes = [C.c_int, P, P]
        L.rpp_similarity_host_finalize.restype = C.c_int
        SC = C.POINTER(RppSegmentConfig)
        L.rpp_segment_check_config.argtypes = [SC]
        L.rpp_segment_check_config.restype = C.c_int
        L.rpp_segment_tile_frames.argtypes = []
        L.rpp_segment_tile_frames.restype = C.c_uint64
        L.rpp_segment_positions.argtypes = [SC, C.c_uint64]
        L.rpp_segment_positions.restype = C.c_uint64
        L.rpp_segment_index_slots.argtypes = [SC, C.c_uint64]
        L.rpp_segment_index_slots.restype = C.c_uint64
        L.rpp_segment_hash_workspace_bytes.argtypes = [C.c_uint32, C.c_uint64]
        L.rpp_segment_hash_workspace_bytes.restype = C.c_uint64
        L.rpp_segment_hash_batch.argtypes = [SC, P, P, P, C.c_uint32, C.c_uint64, P, C.c_uint64, P, P, P, C.c_uint64, P]
        L.rpp_segment_hash_batch.restype = C.c_int
        L.rpp_segment_scan_workspace_bytes.argtypes = [C.c_uint32, C.c_uint64]
        L.rpp_segment_scan_workspace_bytes.restype = C.c_uint64
        L.rpp_segment_scan_batch.argtypes = [SC, P, P, P, C.c_uint32, C.c_uint64, P, P, C.c_uint64, P, P, P, C.c_uint64,
                                             P]
        L.rpp_segment_scan_batch.restype = C.c_int
        L.rpp_segment_index_workspace_bytes.argtypes = [C.c_uint32]
        L.rpp_segment_index_workspace_bytes.restype = C.c_uint64
        L.rpp_segment_index_batch.argtypes = [SC, P, P, P, C.c_uint32, C.c_uint64, P, P, P, C.c_uint64, P, P, P, P, P,
                                              C.c_uint64, P]
        L.rpp_segment_index_batch.restype = C.c_int
        L.rpp_segment_extend_batch.argtypes = [SC, P, P, P, C.c_uint32, P, P]
        L.rpp_segment_extend_batch.restype = C.c_int
        L.rpp_segment_host_hashes.argtypes = [SC, P, C.c_uint64, P]
        L.rpp_segment_host_hashes.restype = C.c_int
        L.rpp_segment_host_index.argtypes = [SC, P, C.c_uint64, P, P, P, P, P]
        L.rpp_segment_host_index.restype = C.c_int
        L.rpp_segment_host_scan.argtypes = [SC, P, C.c_uint64, P, P, C.c_uint64, P]
        L.rpp_segment_host_scan.restype = C.c_int
        L.rpp_segment_host_extend.argtypes = [SC, P, P, P, C.c_uint32, P]
        L.rpp_segment_host_extend.restype = C.c_int
        U32, U64 = C.c_uint32, C.c_uint64
        L.rpp_order_check_options.argtypes = [U32, U32]
        L.rpp_order_check_options.restype = C.c_int
        for name in ("rpp_order_split_pass_children", "rpp_order_chain_threads", "rpp_order_chain_stage_rows"):
            getattr(L, name).argtypes = []
            getattr(L, name).restype = U32
        L.rpp_order_split_workspace_bytes.argtypes = [U64]
        L.rpp_order_split_workspace_bytes.restype = U64
        L.rpp_order_split_batch.argtypes = [P, U32, P, P, P, U32, U64, U32, U32, P, P, P, U64, P]
        L.rpp_order_split_batch.restype = C.c_int
        L.rpp_order_chain_workspace_bytes.argtypes = [U64]
        L.rpp_order_chain_workspace_bytes.restype = U64
        L.rpp_order_chain_batch.argtypes = [P, U32, P, P, P, U32, P, P]
        L.rpp_order_chain_batch.restype = C.c_int
        L.rpp_order_host_split.argtypes = [P, U32, P, U32, U32, U32, P, P]
        L.rpp_order_host_split.restype = C.c_int
        L.rpp_order_host_chain.argtypes = [P, U32, P, P, U32, P]
        L.rpp_order_host_chain.restype = C.c_int
        L.rpp_order_host_nilsimsa.argtypes = [P, P, P, U32, P, U32, U32, U32, P, C.POINTER(RppOrderStats)]
        L.rpp_order_host_nilsimsa.restype = C.c_int
        L.rpp_lz4_bound.argtypes = [U64]
        L.rpp_lz4_bound.restype = U64
        for name in ("rpp_lz4_chunk_bytes", "rpp_lz4_step_positions"):
            getattr(L, name).argtypes = []
            getattr(L, name).restype = U32
        L.rpp_lz4_frame_header.argtypes = [U32, P]
        L.rpp_lz4_frame_header.restype = C.c_size_t
        L.rpp_lz4_parse_frame.argtypes = [P, C.c_size_t, C.POINTER(U32)]
        L.rpp_lz4_parse_frame.restype = C.c_long
        L.rpp_lz4_decode_batch.argtypes = [P, P, P, U32, P, P, P, P, P]
        L.rpp_lz4_decode_batch.restype = C.c_int
        L.rpp_lz4_encode_workspace_bytes.argtypes = [U64, U32]
        L.rpp_lz4_encode_workspace_bytes.restype = U64
        L.rpp_lz4_encode_batch.argtypes = [P, P, P, U32, P, P, P, P, P, U64, P, U64, P]
        L.rpp_lz4_encode_batch.restype = C.c_int
        L.rpp_lz4_host_decode.argtypes = [P, U64, P, U64]
        L.rpp_lz4_host_decode.restype = C.c_int
        L.rpp_lz4_host_encode.argtypes = [P, U64, P, U64, C.POINTER(U64), C.POINTER(U32)]
        L.rpp_lz4_host_encode.restype = C.c_int
        L.rpp_zstd_frame_info.argtypes = [P, C.c_size_t, C.POINTER(U64), C.POINTER(U64), C.POINTER(U32)]
        L.rpp_zstd_frame_info.restype = C.c_long
        L.rpp_zstd_count_blocks.argtypes = [P, C.c_size_t]
        L.rpp_zstd_count_blocks.restype = C.c_long
        L.rpp_zstd_decode_workspace_bytes.argtypes = [U64, U32]
        L.rpp_zstd_decode_workspace_bytes.restype = U64
        L.rpp_zstd_decode_batch.argtypes = [P, P, P, U32, P, P, P, P, U32, P, U64, P]
        L.rpp_zstd_decode_batch.restype = C.c_int
        L.rpp_zstd_host_decode.argtypes = [P, U64, P, U64]
        L.rpp_zstd_host_decode.restype = C.c_int
        L.rpp_zstd_bound.argtypes = [U64]
        L.rpp_zstd_bound.restype = U64
        L.rpp_zstd_encode_workspace_bytes.argtypes = [U64, U32]
        L.rpp_zstd_encode_workspace_bytes.restype = U64
        L.rpp_zstd_encode_batch.argtypes = [P, P, P, U32, P, P, P, P, P, U64, P, U64, P]
        L.rpp_zstd_encode_batch.restype = C.c_int
        L.rpp_zstd_host_encode.argtypes = [P, U64, P, U64, C.POINTER(U64), C.POINTER(U32)]
        L.rpp_zstd_host_encode.restype = C.c_int
        L.rpp_zstd_encode_batch_opt.argtypes = [P, P, P, U32, U32, P, P, P, P, P, U64, P, U64, P]
        L.rpp_zstd_encode_batch_opt.restype = C.c_int
        L.rpp_zstd_host_encode_opt.argtypes = [P, U64, U32, P, U64, C.POINTER(U64), C.POINTER(U32)]
        L.rpp_zstd_host_encode_opt.restype = C.c_int
        L.rpp_lz4_encode_batch_search.argtypes = [P, P, P, U32, U32, P, P, P, P, P, U64, P, U64, P]
        L.rpp_lz4_encode_batch_search.restype = C.c_int
        L.rpp_lz4_host_encode_search.argtypes = [P, U64, U32, P, U64, C.POINTER(U64), C.POINTER(U32)]
        L.rpp_lz4_host_encode_search.restype = C.c_int
        L.rpp_zstd_encode_batch_search.argtypes = [P, P, P, U32, U32, U32, P, P, P, P, P, U64, P, U64, P]
        L.rpp_zstd_encode_batch_search.restype = C.c_int
        L.rpp_zstd_host_encode_search.argtypes = [P, U64, U32, U32, P, U64, C.POINTER(U64), C.POINTER(U32)]
        L.rpp_zstd_host_encode_search.restype = C.c_int
        L.rpp_incompressible_workspace_bytes.argtypes = [U64, U32, U32]
        L.rpp_incompressible_workspace_bytes.restype = U64
        L.rpp_incompressible_scan_batch.argtypes = [P, P, P, U32, P, U32, C.c_double, U32, U32, U32, P, P, P, P, P, P,
                                                    U64, P, U64, P]
        L.rpp_incompressible_scan_batch.restype = C.c_int
        L.rpp_incompressible_host_scan.argtypes = [P, P, P, U32, P, U32, C.c_double, U32, U32, U32, P, P, P, P, P, P]
        L.rpp_incompressible_host_scan.restype = C.c_int
        L.rpp_zstd_encode_workspace_bytes_long.argtypes = [U64, U32, U32]
        L.rpp_zstd_encode_workspace_bytes_long.restype = U64
        L.rpp_zstd_encode_batch_long.argtypes = [P, P, P, U32, U32, U32, U32, P, P, P, P, P, U64, P, U64, P]
        L.rpp_zstd_encode_batch_long.restype = C.c_int
        L.rpp_zstd_host_encode_long.argtypes = [P, U64, U32, U32, U32, P, U64, C.POINTER(U64), C.POINTER(U32)]
        L.rpp_zstd_host_encode_long.restype = C.c_int
        L.rpp_zstd_host_long_sequences.argtypes = [P, U64, U32, U32, P, U64, C.POINTER(U64)]
        L.rpp_zstd_host_long_sequences.restype = C.c_int
        L.rpp_incompressible_workspace_bytes_long.argtypes = [U64, U32, U32, U32]
        L.rpp_incompressible_workspace_bytes_long.restype = U64
        L.rpp_incompressible_scan_batch_long.argtypes = [P, P, P, U32, P, U32, C.c_double, U32, U32, U32, U32, P, P, P,
                                                         P, P, P, U64, P, U64, P]
        L.rpp_incompressible_scan_batch_long.restype = C.c_int
        L.rpp_incompressible_host_scan_long.argtypes = [P, P, P, U32, P, U32, C.c_double, U32, U32, U32, U32, P, P, P, P,
                                                        P, P]
        L.rpp_incompressible_host_scan_long.restype = C.c_int
        L.rpp_extract_tile_bytes.argtypes = []
        L.rpp_extract_tile_bytes.restype = U64
        L.rpp_extract_workspace_bytes.argtypes = [U64, U32, U64]
        L.rpp_extract_workspace_bytes.restype = U64
        L.rpp_extract_gather_batch.argtypes = [P, U64, P, P, U32, P, P, U64, P, U32, P, U64, P, P, U64, P]
        L.rpp_extract_gather_batch.restype = C.c_int
        L.rpp_extract_host_gather.argtypes = [P, U64, P, P, U32, P, P, U64, P, U32, P, U64, P]
        L.rpp_extract_host_gather.restype = C.c_int
        L.rpp_digest_algo.argtypes = [C.c_char_p]
        L.rpp_digest_algo.restype = C.c_int
        L.rpp_digest_bytes.argtypes = [C.c_int]
        L.rpp_digest_bytes.restype = C.c_int
        L.rpp_digest_batch.argtypes = [C.c_int, P, P, P, P, U32, P, P]
        L.rpp_digest_batch.restype = C.c_int
        L.rpp_digest_host.argtypes = [C.c_int, P, P, P, P, U32, P]
        L.rpp_digest_host.restype = C.c_int
        if L.rpp_abi_version() != 1:
            raise RuntimeError("libricepp_amd.so ABI mismatch")
        _lib = L
    return _lib
