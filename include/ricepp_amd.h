/*
 * ricepp_amd.h -- C ABI of the MI355X-native ricepp block codec.
 *
 * This is the drop-in boundary: plain C types, device pointers and sizes, no
 * torch or C++ types.  It replaces the inner ricepp library API that the
 * DwarFS plugin binds (reference: /root/reference):
 *
 *   rpp_check_config      <- ricepp::create_encoder / create_decoder config
 *                            validation (ricepp/ricepp_cpuspecific_traits.h:118-151,
 *                            throws at ricepp/ricepp_cpuspecific.cpp:161,173)
 *   rpp_worst_case_bytes  <- encoder_interface::worst_case_encoded_bytes
 *                            (ricepp/include/ricepp/encoder_interface.h:38-60,
 *                            ricepp/ricepp_cpuspecific.cpp:58-66,75-77,
 *                            ricepp/include/ricepp/codec.h:142-151)
 *   rpp_encode_batch /    <- encoder_interface::encode(span<u8>, span<u16 const>)
 *   rpp_encode_batch_ws
 *                            (ricepp/ricepp_cpuspecific.cpp:68-72,101-108), one
 *                            call per DwarFS block in src/compression/ricepp.cpp:136-137,
 *                            batched over many independent blocks
 *   rpp_decode_batch /    <- decoder_interface::decode(span<u16>, span<u8 const>)
 *   rpp_decode_batch_ws
 *                            (ricepp/include/ricepp/decoder_interface.h:37-50,
 *                            ricepp/ricepp_cpuspecific.cpp:127-144), called by
 *                            src/compression/ricepp.cpp:215-232
 *   rpp_unused_lsb_batch  <- the FITS categorizer's unused-LSB detection
 *                            (src/writer/categorizer/fits_categorizer.cpp:118-178),
 *                            which picks the codec's unused_lsb_count
 *   rpp_exclusive_scan_u64 <- the writer's running image offset as it appends
 *   rpp_pack_batch           compressed blocks (src/writer/filesystem_writer.cpp:255-287)
 *   rpp_pcm_unpack /      <- pcm_sample_transformer<int32_t>::unpack / pack
 *   rpp_pcm_pack             (include/dwarfs/pcm_sample_transformer.h:40-71,
 *                            src/pcm_sample_transformer.cpp:44-228), the PCM
 *                            front end of the FLAC compressor (src/compression/flac.cpp:211,322)
 *   rpp_frame_header /    <- the DwarFS block framing of src/compression/ricepp.cpp:
 *   rpp_parse_frame          varint size + thrift-compact ricepp_block_header
 *                            (:107-127 write, :186-201,237-249 read)
 *
 * Errors: C++ exceptions cannot cross this boundary.  Status codes map back to
 * the reference's exceptions in the C++ facade (include/ricepp_amd.hpp):
 *   RPP_UNSUPPORTED_CONFIG -> std::runtime_error("Unsupported configuration")
 *   RPP_TRUNCATED_INPUT    -> std::out_of_range (bitstream_reader.h:150-152)
 *
 * Memory: every pointer passed to the *_batch calls is DEVICE memory owned by
 * the caller (hipMalloc'd).  Calls are asynchronous on `stream` (a
 * hipStream_t; NULL = default stream), which must belong to the current
 * device (rpp_decode_batch_ws / _ex return RPP_INVALID_ARGUMENT otherwise).
 * Per-block status / sizes are written to device arrays and are valid once
 * the stream has been synchronised.
 */
#ifndef RICEPP_AMD_H
#define RICEPP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPP_OK 0
#define RPP_UNSUPPORTED_CONFIG (-1)
#define RPP_TRUNCATED_INPUT (-2)
#define RPP_INVALID_ARGUMENT (-3)
#define RPP_OUTPUT_TOO_SMALL (-4)
#define RPP_HIP_ERROR (-5)
/* A device-side consistency bound tripped (a decode tile waited longer than
 * its bound for a predecessor's prefix): the block's output is invalid.  Never
 * returned for well-formed or malformed input; it reports a bug or a stalled
 * GPU instead of returning wrong samples as RPP_OK. */
#define RPP_INTERNAL_ERROR (-6)
/* A section's stored XXH3-64 or SHA-512/256 does not match its bytes
 * (rpp_sections_verify_batch): the reader's "block data integrity check
 * failed" (src/reader/internal/cached_block.cpp:58-67). */
#define RPP_CHECKSUM_MISMATCH (-7)

/* ricepp::codec_config (ricepp/include/ricepp/codec_config.h:36-41). */
typedef struct rpp_config {
  uint32_t block_size;             /* ricepp sub-block size, 1..512 */
  uint32_t component_stream_count; /* 1 or 2 */
  uint32_t big_endian;             /* stored sample byte order: 1 = big */
  uint32_t unused_lsb_count;       /* 0..15 */
} rpp_config;

/* Streams hold fewer samples than this: mkdwarfs blocks go up to 2^30 bytes
 * (-S 30, tools/src/mkdwarfs_main.cpp:135), i.e. 2^29 samples.  Streams of
 * 2^27 samples and more are encoded in segments by rpp_encode_batch_ws (the
 * workspace-free rpp_encode_batch, one wave per stream, takes fewer) and
 * decoded one wave each (not segmented). */
#define RPP_MAX_STREAM_SAMPLES (UINT64_C(1) << 30)

/* ABI version, bumped on any signature change. */
uint32_t rpp_abi_version(void);

/* RPP_OK or RPP_UNSUPPORTED_CONFIG. */
int rpp_check_config(const rpp_config* cfg);

/* ceil(cs * (16 + 4*ceil((n/cs)/bs) + 16*(n/cs)) / 8) bytes. */
uint64_t rpp_worst_case_bytes(const rpp_config* cfg, uint64_t n_samples);

/*
 * Encode `nblocks` independent ricepp streams.
 *   d_in          stored uint16 samples
 *   d_in_offsets  [nblocks] start of block b in d_in, in samples, 8-aligned
 *   d_n_samples   [nblocks] samples in block b (multiple of cs, < RPP_MAX_STREAM_SAMPLES)
 *   d_out         output bytes
 *   d_out_offsets [nblocks] byte offset of block b's output, 16-aligned;
 *                 the region must hold rpp_worst_case_bytes(n_samples[b])
 *   d_out_bytes   [nblocks] written: encoded size of block b
 *   d_status      [nblocks] written: RPP_OK or an error code
 * Returns RPP_OK if the launch was issued, else an error code.
 */
int rpp_encode_batch(const rpp_config* cfg, const uint16_t* d_in, const uint64_t* d_in_offsets,
                     const uint64_t* d_n_samples, uint32_t nblocks, uint8_t* d_out,
                     const uint64_t* d_out_offsets, uint64_t* d_out_bytes, int32_t* d_status,
                     void* stream);

/*
 * Device workspace rpp_encode_batch_ws needs for `nblocks` streams holding
 * `total_samples` samples in all, none longer than `max_stream_samples`
 * (0: no workspace needed; also for an unsupported config).
 */
uint64_t rpp_encode_workspace_bytes(const rpp_config* cfg, uint64_t total_samples, uint64_t max_stream_samples,
                                    uint32_t nblocks);

/*
 * rpp_encode_batch with a caller-owned device workspace of at least
 * rpp_encode_workspace_bytes(cfg, total_samples, max_stream_samples, nblocks)
 * bytes (total_samples >= the sum and max_stream_samples >= the maximum of
 * d_n_samples).  Streams longer than 256 chunks of cs * bs samples are encoded
 * by several waves in parallel (a segment per 256 chunks, then the segments'
 * bits are placed at their offsets), so a 16 MiB DwarFS block no longer
 * encodes at one wave's speed; a batch without such streams is exactly
 * rpp_encode_batch.  Same output as rpp_encode_batch, byte for byte.  Fully
 * asynchronous on `stream`.
 */
int rpp_encode_batch_ws(const rpp_config* cfg, const uint16_t* d_in, const uint64_t* d_in_offsets,
                        const uint64_t* d_n_samples, uint32_t nblocks, uint8_t* d_out,
                        const uint64_t* d_out_offsets, uint64_t* d_out_bytes, int32_t* d_status,
                        uint64_t total_samples, uint64_t max_stream_samples, void* d_workspace,
                        uint64_t workspace_bytes, void* stream);

/*
 * Decode `nblocks` independent ricepp streams.
 *   d_in          encoded bytes
 *   d_in_offsets  [nblocks] byte offset of block b's stream (any alignment: a
 *                 DwarFS payload right after its varint + thrift header)
 *   d_in_bytes    [nblocks] encoded size of block b
 *   d_out         decoded stored uint16 samples
 *   d_out_offsets [nblocks] start of block b's output, in samples, 8-aligned
 *   d_n_samples   [nblocks] samples to decode (multiple of cs)
 *   d_status      [nblocks] RPP_OK, RPP_TRUNCATED_INPUT (the reference's
 *                 std::out_of_range) or RPP_INVALID_ARGUMENT
 * This workspace-free form ALWAYS decodes one stream per wavefront (parse
 * and values fused; bs 16 / 32: four streams per wavefront, one per 16-lane
 * row, any stream that path leaves then one per wavefront), fully
 * asynchronously on `stream`.  That is the fast
 * path for batches of many short streams (thousands of 64 KiB blocks), but a
 * long stream then decodes at one wave's speed (a 16 MiB block: ~30 ms).
 * Batches with long streams should use rpp_decode_batch_ws, which splits
 * them over many waves.
 */
int rpp_decode_batch(const rpp_config* cfg, const uint8_t* d_in, const uint64_t* d_in_offsets,
                     const uint64_t* d_in_bytes, uint32_t nblocks, uint16_t* d_out,
                     const uint64_t* d_out_offsets, const uint64_t* d_n_samples,
                     int32_t* d_status, void* stream);

/*
 * Device workspace rpp_decode_batch_ws needs for a batch of `nblocks` streams
 * holding `total_samples` samples in all, the longest `max_stream_samples`
 * (0: none needed, or an unsupported config).
 */
uint64_t rpp_decode_workspace_bytes(const rpp_config* cfg, uint64_t total_samples, uint64_t max_stream_samples,
                                    uint32_t nblocks);

/*
 * rpp_decode_batch with the batch's sample counts and a caller-owned device
 * workspace of at least rpp_decode_workspace_bytes(cfg, total_samples,
 * max_stream_samples, nblocks) bytes, where total_samples >= the sum of
 * d_n_samples and max_stream_samples >= the largest.  Fully asynchronous on
 * `stream` (graph-capturable: no host synchronisation; a segmented call forks
 * part of its work onto a side stream private to `stream` and joins it before
 * returning).  A batch whose longest stream holds more than 1/1024 of its
 * samples (and >= 2^18) is decoded segmented: long streams are cut into units
 * of 2^18..2^23 bits parsed by one wave each from a guessed first header,
 * stitched exactly, then every sub-block of every stream is decoded by its
 * own lane; other batches one wave per stream.  If the device finds the
 * batch larger than total_samples / max_stream_samples promised, it decodes
 * the whole batch one wave per stream instead (correct, never out of the
 * workspace's bounds).
 */
int rpp_decode_batch_ws(const rpp_config* cfg, const uint8_t* d_in, const uint64_t* d_in_offsets,
                        const uint64_t* d_in_bytes, uint32_t nblocks, uint16_t* d_out,
                        const uint64_t* d_out_offsets, const uint64_t* d_n_samples, int32_t* d_status,
                        uint64_t total_samples, uint64_t max_stream_samples, void* d_workspace,
                        uint64_t workspace_bytes, void* stream);

/*
 * Explicit decode path selection (tests, diagnostics, tuning).  A NULL
 * options pointer or a zeroed struct is exactly rpp_decode_batch_ws.
 */
#define RPP_DECODE_AUTO 0      /* segmented when the batch has long streams */
#define RPP_DECODE_FUSED 1     /* one wave per stream, never segmented */
#define RPP_DECODE_SEGMENTED 2 /* every stream longer than one unit is split */
/* test_flags: fault injection and diagnostics, 0 in production */
#define RPP_TEST_NO_FAST_LANES 1u   /* extraction: every lane takes the general path */
#define RPP_TEST_LOOKBACK_STALL 2u  /* extraction: tile 1 of each stream never publishes its prefix,
                                       and the look-back gives up after 2^10 polls (-> RPP_INTERNAL_ERROR) */
#define RPP_TEST_PHASE_TIMERS 4u    /* extraction: per-phase cycle counters (diagnostic builds' tools) */
typedef struct rpp_decode_options {
  uint32_t path;        /* RPP_DECODE_AUTO / _FUSED / _SEGMENTED */
  uint32_t seg_log2;    /* units of 2^seg_log2 bits, 10..26; 0: chosen from the batch */
  uint32_t fused_waves; /* streams per workgroup of the one-wave-per-stream kernel, 1..16; 0: auto */
  uint32_t test_flags;  /* RPP_TEST_* */
} rpp_decode_options;

uint64_t rpp_decode_workspace_bytes_ex(const rpp_config* cfg, uint64_t total_samples, uint64_t max_stream_samples,
                                       uint32_t nblocks, const rpp_decode_options* opt);
int rpp_decode_batch_ex(const rpp_config* cfg, const uint8_t* d_in, const uint64_t* d_in_offsets,
                        const uint64_t* d_in_bytes, uint32_t nblocks, uint16_t* d_out,
                        const uint64_t* d_out_offsets, const uint64_t* d_n_samples, int32_t* d_status,
                        uint64_t total_samples, uint64_t max_stream_samples, void* d_workspace,
                        uint64_t workspace_bytes, const rpp_decode_options* opt, void* stream);

/*
 * Unused least-significant bits of 16-bit images (the FITS categorizer's
 * get_unused_lsb_count, src/writer/categorizer/fits_categorizer.cpp:118-178):
 * for each image, the OR of all its samples (converted from big endian when
 * big_endian != 0) and d_counts[i] = its number of trailing zero bits
 * (std::countr_zero of a uint16_t: 16 for an all-zero or empty image).
 *   d_in          stored uint16 samples
 *   d_offsets     [nimages] first sample of image i
 *   d_n_samples   [nimages] samples of image i, each <= max_samples
 *   d_work        [nimages] device scratch (overwritten)
 *   d_counts      [nimages] written: unused LSB count of image i
 * Asynchronous on `stream`; nimages <= 65535 per call.
 */
int rpp_unused_lsb_batch(const uint16_t* d_in, const uint64_t* d_offsets, const uint64_t* d_n_samples,
                         uint64_t max_samples, uint32_t nimages, uint32_t big_endian, uint32_t* d_work,
                         uint32_t* d_counts, void* stream);

/*
 * Image offsets of a batch of compressed blocks: d_out[b] = sum of d_in[0..b-1]
 * (exclusive prefix sum, uint64).  The DwarFS writer appends compressed blocks
 * back to back (src/writer/filesystem_writer.cpp:255-287); with the encoded
 * sizes of a GPU batch in device memory (all-gathered across ranks) this gives
 * every block's position in the image without a host round trip.
 * d_in may equal d_out only if n <= 1.  Asynchronous on `stream`.
 */
int rpp_exclusive_scan_u64(const uint64_t* d_in, uint64_t n, uint64_t* d_out, void* stream);

/*
 * Pack the encoded streams of a batch (e.g. rpp_encode_batch output, block b at
 * d_src + d_src_offsets[b], 16-aligned, d_sizes[b] bytes) back to back at
 * 16-byte-aligned offsets: d_dst_offsets[b] = sum of round_up(d_sizes[j], 16)
 * for j < b, block b's bytes copied to d_dst + d_dst_offsets[b], *d_total =
 * the packed length.  d_dst must hold sum(round_up(sizes, 16)) bytes (at most
 * the sum of the encode capacities); the source slots must be readable up to
 * round_up(size, 16).  Then one device->host copy of *d_total bytes moves the
 * batch, instead of its worst-case capacity (the writer's block hand-off,
 * src/writer/filesystem_writer.cpp:255-287).  Asynchronous on `stream`.
 */
int rpp_pack_batch(const uint8_t* d_src, const uint64_t* d_src_offsets, const uint64_t* d_sizes, uint32_t nblocks,
                   uint8_t* d_dst, uint64_t* d_dst_offsets, uint64_t* d_total, void* stream);

/*
 * DwarFS ricepp block framing (host memory).  rpp_frame_header writes
 * varint(uncompressed_bytes) + the thrift-compact ricepp_block_header
 * (thrift/compression.thrift:42-49) to `out` (>= 32 bytes) and returns its
 * length.  rpp_parse_frame parses the same, returns the header length or a
 * negative status.
 */
typedef struct rpp_frame {
  uint64_t uncompressed_bytes;
  uint32_t block_size;
  uint32_t component_count;
  uint32_t bytes_per_sample;
  uint32_t unused_lsb_count;
  uint32_t big_endian;
  uint32_t ricepp_version;
} rpp_frame;

size_t rpp_frame_header(const rpp_frame* f, uint8_t* out);
long rpp_parse_frame(const uint8_t* in, size_t in_len, rpp_frame* f);

/*
 * PCM sample format (pcm_sample_transformer's constructor arguments,
 * include/dwarfs/pcm_sample_transformer.h:36-45): bytes per sample 1..4,
 * significant bits 1..8*bytes, big_endian / is_signed / lsb_padded as 0/1.
 * rpp_pcm_check_format: RPP_OK; RPP_UNSUPPORTED_CONFIG for bytes outside 1..4
 * (the reference's runtime_error "unsupported number of bytes per sample: N",
 * src/pcm_sample_transformer.cpp:310-311); RPP_INVALID_ARGUMENT for bits
 * outside 1..8*bytes (asserted by the reference, :354).
 */
typedef struct rpp_pcm_format {
  uint32_t big_endian;
  uint32_t is_signed;
  uint32_t lsb_padded;
  uint32_t bytes;
  uint32_t bits;
} rpp_pcm_format;

int rpp_pcm_check_format(const rpp_pcm_format* f);

/*
 * n_samples PCM samples of `bytes` bytes each at d_src -> int32 at d_dst
 * (pcm_sample_transformer<int32_t>::unpack), and the inverse
 * (pcm_sample_transformer<int32_t>::pack).  Device memory; asynchronous on
 * `stream`.  Any alignment is accepted (4-byte packed / 16-byte int32 buffers
 * take the vector path).
 */
int rpp_pcm_unpack(const rpp_pcm_format* f, const uint8_t* d_src, int32_t* d_dst, uint64_t n_samples, void* stream);
int rpp_pcm_pack(const rpp_pcm_format* f, const int32_t* d_src, uint8_t* d_dst, uint64_t n_samples, void* stream);

/*
 * FLAC blocks (src/compression/flac.cpp).  Parity unpinned: the reference
 * codes them with libFLAC (absent here; no FLAC fixture in the reference).
 *
 * Framing, host side: varint(uncompressed bytes) + thrift-compact
 * flac_block_header (thrift/compression.thrift:36-40; written by
 * flac_block_compressor::compress, flac.cpp:284-304, parsed by
 * flac_block_decompressor, :477-484) + a native FLAC stream.  flags: bit 7
 * big endian, bit 6 signed, bit 5 LSB padding, bits 0-1 bytes per sample - 1
 * (flac.cpp:41-44).  rpp_flac_stream_header writes "fLaC" + STREAMINFO
 * (42 bytes: 4096-sample blocks, 48 kHz as flac.cpp:311, MD5 unknown);
 * rpp_flac_parse_stream reads any stream's metadata blocks and returns the
 * offset of its first frame (or an RPP_* error).
 */
typedef struct rpp_flac_frame {
  uint64_t uncompressed_bytes;
  uint32_t num_channels;
  uint32_t bits_per_sample;
  uint32_t flags;
} rpp_flac_frame;

typedef struct rpp_flac_stream_info {
  uint32_t min_blocksize, max_blocksize;
  uint32_t sample_rate, channels, bits_per_sample;
  uint64_t total_samples;
} rpp_flac_stream_info;

size_t rpp_flac_frame_header(const rpp_flac_frame* f, uint8_t* out);
long rpp_flac_parse_frame(const uint8_t* in, size_t in_len, rpp_flac_frame* f);
size_t rpp_flac_stream_header(uint32_t channels, uint32_t bps, uint64_t nsamples, uint8_t* out);
long rpp_flac_parse_stream(const uint8_t* in, size_t len, rpp_flac_stream_info* info);

/*
 * FLAC frames on the device (replaces the libFLAC stream encoder /
 * decoder calls of flac.cpp:306-349 and :442-472).
 *
 * rpp_flac_encode: nsamples interleaved frames of `channels` int32 samples
 * of `bps` significant bits (8..32; channels 1..8, flac.cpp:243-245) ->
 * FLAC frames of 4096 samples (fixed and LPC predictors, stereo
 * decorrelation, partitioned Rice codes, CRC-8 / CRC-16) back to back at d_out
 * (rpp_flac_frame_bound bytes per frame at most); *d_total = their size.
 * Workspace: rpp_flac_encode_workspace_bytes.
 *
 * rpp_flac_decode: the frames of a stream (after its metadata blocks) ->
 * nsamples interleaved frames of int32 samples; every RFC 9639 frame kind is
 * accepted.  Frame starts are found by a sync-code scan: at most
 * max_candidates of them are kept; *d_ncand receives how many there were
 * (more than max_candidates: call again with a larger workspace).  *d_status:
 * RPP_OK, RPP_TRUNCATED_INPUT or RPP_INVALID_ARGUMENT (a frame that does not
 * parse or fails its CRC).  Workspace: rpp_flac_decode_workspace_bytes.
 */
uint64_t rpp_flac_frame_bound(uint32_t channels, uint32_t bps);
uint64_t rpp_flac_encode_workspace_bytes(uint64_t nsamples, uint32_t channels, uint32_t bps);
int rpp_flac_encode(const int32_t* d_samples, uint64_t nsamples, uint32_t channels, uint32_t bps, uint8_t* d_out,
                    uint64_t* d_total, void* d_workspace, uint64_t workspace_bytes, void* stream);
/* rpp_flac_encode at a libFLAC compression level (0..8: levels 0-2 fixed
 * predictors only, 3 LPC up to order 6, 4-6 up to 8, 7-8 up to 12; Rice
 * partition orders up to 3 / 4 / 5) and with `exhaustive` (every LPC order
 * coded, the cheapest kept; else libFLAC's expected-bits estimate picks the
 * order) -- FLAC__stream_encoder_set_compression_level / _set_do_exhaustive_
 * model_search as flac.cpp:312-313 calls them.  rpp_flac_encode is level 5. */
int rpp_flac_encode_ex(const int32_t* d_samples, uint64_t nsamples, uint32_t channels, uint32_t bps, uint32_t level,
                       uint32_t exhaustive, uint8_t* d_out, uint64_t* d_total, void* d_workspace,
                       uint64_t workspace_bytes, void* stream);
/* Several blocks in one launch (DwarFS compresses one block per call,
 * flac.cpp:284-349; a batching caller, as the ricepp facade does for ricepp,
 * joins them): block b is h_nsamples[b] interleaved frames of h_channels[b]
 * int32 samples of h_bps[b] bits at d_samples + h_in_off[b] (host arrays: the
 * launch needs the frame count).  Its FLAC frames (numbered from 0) are
 * written to d_out[d_out_off[b], d_out_off[b + 1]) (d_out_off: device,
 * nblocks + 1 entries), byte-identical to rpp_flac_encode_ex of that block
 * alone.  Workspace: rpp_flac_encode_batch_workspace_bytes. */
uint64_t rpp_flac_encode_batch_workspace_bytes(uint32_t nblocks, const uint64_t* h_nsamples, const uint32_t* h_channels,
                                               const uint32_t* h_bps);
int rpp_flac_encode_batch(const int32_t* d_samples, uint32_t nblocks, const uint64_t* h_in_off,
                          const uint64_t* h_nsamples, const uint32_t* h_channels, const uint32_t* h_bps,
                          uint32_t level, uint32_t exhaustive, uint8_t* d_out, uint64_t* d_out_off, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);
uint64_t rpp_flac_decode_workspace_bytes(uint64_t nbytes, uint32_t channels, uint32_t bps, uint32_t max_blocksize,
                                         uint32_t max_candidates);
int rpp_flac_decode(const uint8_t* d_frames, uint64_t nbytes, uint32_t channels, uint32_t bps,
                    uint32_t max_blocksize, uint64_t nsamples, int32_t* d_out, int32_t* d_status,
                    uint32_t max_candidates, void* d_workspace, uint64_t workspace_bytes, uint32_t* d_ncand,
                    void* stream);
/* Several streams' frames decoded in one sequence of launches (the
 * reference decompresses one block per call, flac.cpp:405-489; a batching
 * caller joins them as the ricepp facade does): stream b is h_nbytes[b]
 * bytes of frames at d_frames + h_in_off[b] with its STREAMINFO's channels,
 * bps, max block size and h_nsamples[b] samples per channel, decoded to
 * d_out + h_out_off[b] (int32 elements) with d_status[b] and d_ncand[b] as
 * rpp_flac_decode gives them for that stream alone -- byte for byte the
 * same.  Host arrays (the launches need the sizes); nblocks <= 65535.
 * Workspace: rpp_flac_decode_batch_workspace_bytes. */
uint64_t rpp_flac_decode_batch_workspace_bytes(uint32_t nblocks, const uint64_t* h_nbytes, const uint32_t* h_channels,
                                               const uint32_t* h_bps, const uint32_t* h_max_blocksize,
                                               const uint32_t* h_max_candidates);
int rpp_flac_decode_batch(const uint8_t* d_frames, uint32_t nblocks, const uint64_t* h_in_off,
                          const uint64_t* h_nbytes, const uint32_t* h_channels, const uint32_t* h_bps,
                          const uint32_t* h_max_blocksize, const uint64_t* h_nsamples, int32_t* d_out,
                          const uint64_t* h_out_off, int32_t* d_status, const uint32_t* h_max_candidates,
                          void* d_workspace, uint64_t workspace_bytes, uint32_t* d_ncand, void* stream);

/*
 * Section checksums and headers (DwarFS section_header_v2,
 * include/dwarfs/fstypes.h:85-97: "DWARFS", major 2, minor 5, sha2_512_256 at
 * [8,40), xxh3_64 at [40,48), number [48,52), type [52,54), compression
 * [54,56), length [56,64), little endian).
 *
 *   rpp_section_headers_batch   <- fsblock::build_section_header
 *   rpp_sections_assemble_batch    (src/writer/filesystem_writer.cpp:606-651), the
 *                                  writer's two checksums per block, and the
 *                                  header + data it then writes
 *   rpp_sections_verify_batch   <- fs_section_v2::check_fast (level 1: XXH3-64,
 *                                  src/internal/fs_section.cpp:226-259, called by
 *                                  cached_block, src/reader/internal/cached_block.cpp:58-67)
 *                                  and fs_section_checker::verify (level 2: also
 *                                  SHA-512/256, src/internal/fs_section_checker.cpp)
 *
 * A message of the two hash calls is an optional prefix followed by a payload
 * span: message b = d_prefix[64 * b, 64 * b + d_prefix_len[b]) (at most 64
 * bytes; d_prefix NULL: none) followed by d_data[d_offsets[b], d_offsets[b] +
 * d_sizes[b]) at any alignment.  XXH3-64 is the 64-bit XXH3 with seed 0 and
 * the default secret (every length class; messages over 240 bytes take one
 * wave each, shorter ones one lane each); SHA-512/256 is FIPS 180-4 (one lane
 * per message, below 2^61 bytes).  d_hash[b] receives the XXH3 value,
 * d_digest[32 * b ..] the 32 digest bytes.  Like every *_batch call: device
 * pointers, asynchronous on `stream`, n == 0 returns RPP_OK at once.
 */
int rpp_xxh3_64_batch(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n,
                      const uint8_t* d_prefix, const uint32_t* d_prefix_len, uint64_t* d_hash, void* stream);
int rpp_sha512_256_batch(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n,
                         const uint8_t* d_prefix, const uint32_t* d_prefix_len, uint8_t* d_digest, void* stream);

/*
 * Complete v2 headers of n sections of one type: section b holds
 * d_frame[32 * b, 32 * b + d_frame_len[b]) (the DwarFS frame header of a
 * ricepp block, rpp_frame_header; d_frame NULL: none) followed by
 * d_payload[d_payload_offsets[b], + d_payload_sizes[b]).  d_headers[64 * b ..]
 * receives magic, version 2.5, number = first_number + b, type, compression
 * (both < 2^16), length = frame length + payload size, the XXH3-64 over
 * header[48,64) + data and then the SHA-512/256 over header[40,64) + data,
 * in the reference's order.
 */
int rpp_section_headers_batch(const uint8_t* d_payload, const uint64_t* d_payload_offsets,
                              const uint64_t* d_payload_sizes, uint32_t n, uint32_t first_number,
                              uint32_t section_type, uint32_t compression, const uint8_t* d_frame,
                              const uint32_t* d_frame_len, uint8_t* d_headers, void* stream);

/*
 * Image fragment of n sections, byte-packed as the writer appends them:
 * header b, frame b, payload b back to back at d_image + d_section_offsets[b],
 * section b + 1 right behind (no alignment on either side, unlike
 * rpp_pack_batch).  Written: d_section_sizes[b] = 64 + frame length + payload
 * size, d_section_offsets[b] = their exclusive sum (rpp_exclusive_scan_u64),
 * *d_total = the fragment's length (d_total may be NULL).  d_image must hold
 * the sum of the sections' sizes.
 */
int rpp_sections_assemble_batch(const uint8_t* d_headers, const uint8_t* d_frame, const uint32_t* d_frame_len,
                                const uint8_t* d_payload, const uint64_t* d_payload_offsets,
                                const uint64_t* d_payload_sizes, uint32_t n, uint8_t* d_image,
                                uint64_t* d_section_sizes, uint64_t* d_section_offsets, uint64_t* d_total,
                                void* stream);

/*
 * Integrity check of the n sections whose headers start at
 * d_image + d_section_offsets[b], in an image of image_bytes bytes.  level 1
 * checks the XXH3-64, level 2 the SHA-512/256 as well.  d_status[b]: RPP_OK;
 * RPP_CHECKSUM_MISMATCH; RPP_INVALID_ARGUMENT for a header without the magic
 * or with another major version; RPP_TRUNCATED_INPUT when the header or its
 * length runs past image_bytes (nothing beyond image_bytes is read).
 */
int rpp_sections_verify_batch(const uint8_t* d_image, uint64_t image_bytes, const uint64_t* d_section_offsets,
                              uint32_t n, uint32_t level, int32_t* d_status, void* stream);

/* section_header_v2's fields (host memory). */
typedef struct rpp_section_header {
  uint8_t sha2_512_256[32];
  uint64_t xxh3_64;
  uint64_t length;
  uint32_t number;
  uint16_t type;
  uint16_t compression;
  uint8_t major;
  uint8_t minor;
} rpp_section_header;

/* Parses a 64-byte section header: RPP_OK, or RPP_INVALID_ARGUMENT for a
 * wrong magic or major version (nothing is written then). */
int rpp_parse_section_header(const uint8_t in[64], rpp_section_header* out);

/*
 * Duplicate-file detection (file_scanner_::scan_dedupe and hash_file,
 * src/writer/internal/file_scanner.cpp:274-413; the algorithm of --file-hash,
 * tools/src/mkdwarfs_main.cpp:593-594, by dwarfs::checksum's names).
 *
 * Digests are in DwarFS's byte order (checksum_xxh3::finalize,
 * src/checksum.cpp:185-196): XXH3-64 as its 8 little-endian bytes, XXH3-128 as
 * low64 little endian followed by high64 little endian (the reverse of
 * xxhash's canonical form; "Hello, World!" gives
 * 9553D72C8403DB7750DD474484F21D53), SHA-512/256 as its 32 bytes.
 */
enum rpp_file_hash {
  RPP_HASH_XXH3_64 = 0,
  RPP_HASH_XXH3_128 = 1,
  RPP_HASH_SHA512_256 = 2,
};

/* "xxh3-64", "xxh3-128", "sha512-256" -> the enum; anything else (NULL too) -> a negative value.  Host only. */
int rpp_file_hash_algo(const char* name);
/* 8, 16 or 32; 0 for a value that is no algorithm.  Host only. */
int rpp_file_hash_digest_bytes(int algo);

/*
 * XXH3-128 (seed 0, default secret, every length class) of the messages of
 * rpp_xxh3_64_batch, its sibling: d_digest[16 * b ..] receives 16 bytes.
 * Messages over 240 bytes take one wave each -- the loop of XXH3-64 with a
 * second final merge -- shorter ones one lane each.
 */
int rpp_xxh3_128_batch(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n,
                       const uint8_t* d_prefix, const uint32_t* d_prefix_len, uint8_t* d_digest, void* stream);

/*
 * File b = d_data[d_offsets[b], d_offsets[b] + d_sizes[b]) hashed with `algo`
 * into d_digest[digest_bytes * b ..], tightly packed.  d_select (NULL: every
 * file): a file whose byte is 0 is not read and its digest bytes are not
 * written.  An unknown algo is RPP_INVALID_ARGUMENT.
 */
int rpp_file_hash_batch(int algo, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                        const uint8_t* d_select, uint32_t n, uint8_t* d_digest, void* stream);

/*
 * Groups n keys, key b = d_sizes[b] plus the digest_bytes (0, 8, 16 or 32)
 * bytes at d_digest + digest_bytes * b (d_digest NULL or digest_bytes 0: the
 * size alone).  d_first[b] = the smallest a <= b with key a == key b;
 * d_multi[b] (may be NULL) = 1 if key b occurs more than once, else 0.  Keys
 * with d_select[b] == 0 (d_select NULL: none) take no part: first[b] = b,
 * multi[b] = 0, their digest is not read.  The result does not depend on
 * scheduling.  d_workspace holds rpp_group_workspace_bytes(n) bytes (a table
 * of 32-bit slots, 4-aligned); a smaller one, or n above 2^30, is
 * RPP_INVALID_ARGUMENT.
 *
 * rpp_group_start_slot (host, for tests): the slot at which the probe
 * sequence of a key starts in the table for n keys.
 */
uint64_t rpp_group_workspace_bytes(uint32_t n);
int rpp_group_first_batch(const uint64_t* d_sizes, const uint8_t* d_digest, uint32_t digest_bytes,
                          const uint8_t* d_select, uint32_t n, uint32_t* d_first, uint8_t* d_multi,
                          void* d_workspace, uint64_t workspace_bytes, void* stream);
uint64_t rpp_group_start_slot(uint64_t size, const uint8_t* digest, uint32_t digest_bytes, uint32_t n);

/*
 * The scanner's whole decision for n files in one asynchronous sequence:
 * start hashes (XXH3-64 of the first 4 KiB of every file of 1 MiB and up, 0
 * below: kLargeFileThreshold, kLargeFileStartHashSize, file_scanner.cpp:59-60);
 * d_hashed[b] = 1 exactly when another file shares file b's (size, start
 * hash); those files are hashed with `algo` into d_digest[digest_bytes * b ..]
 * (the others' digest bytes are left untouched); d_first[b] = the first file
 * with file b's (size, digest), b itself for a file that was not hashed.
 * d_workspace holds rpp_file_dedup_workspace_bytes(n) bytes, 16-aligned.
 */
uint64_t rpp_file_dedup_workspace_bytes(uint32_t n);
int rpp_file_dedup_batch(int algo, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                         uint32_t n, uint8_t* d_digest, uint32_t* d_first, uint8_t* d_hashed, void* d_workspace,
                         uint64_t workspace_bytes, void* stream);

/*
 * Similarity hashes of the inode scan (inode_::scan_full / scan_fragments /
 * scan_range, src/writer/internal/inode_manager.cpp:399-537): what the fragment
 * orderer sorts or clusters by.
 *
 *   nilsimsa    (src/writer/internal/nilsimsa.cpp) 256 counters; with T the
 *               published Nilsimsa transition table and
 *               tran3(a,b,c,n) = ((T[(a+n)&255] ^ (T[b]*(2n+1))) + T[c^T[n]]) & 255,
 *               the byte w0 at position p of the message and the four bytes
 *               w1..w4 before it increment the buckets (w0,w1,w2,0) from p = 2,
 *               (w0,w1,w3,1) (w0,w2,w3,2) from p = 3 and (w0,w1,w4,3) (w0,w2,w4,4)
 *               (w0,w3,w4,5) (w4,w1,w0,6) (w4,w3,w0,7) from p = 4.  Bit i of the
 *               32-byte digest (byte i >> 3, bit i & 7: the reference's four
 *               uint64 words, little endian) is acc[i] > total / 256 with total
 *               = 0, 1, 4 for sizes below 3, 3, 4 and 8 * size - 28 above.
 *   similarity  (src/writer/internal/similarity.cpp) val = (val << 8) | byte;
 *               from p = 3 on, the uint32 counter mix32(val + 0x9e3779b9) >> 24
 *               is incremented (it wraps).  The digest is the uint32
 *               b0 << 24 | b1 << 16 | b2 << 8 | b3 of the four buckets with the
 *               highest counts, ties to the lower index, stored as 4 bytes in
 *               host order (little endian); an empty message gives 0x00010203.
 *
 * Both are sums of per-position increments, so a message's state can be built
 * from chunks in any order and by several calls.  A state is (8-aligned; all
 * zero is the initial state, so a memset initialises it; the same bytes on the
 * host and on the device):
 *   nilsimsa    uint64 acc[256] | uint64 size | uint8 window[4] (the last four
 *               bytes in message order, window[3] the latest, zero before the
 *               start) | 4 bytes of padding                       = 2064 bytes
 *   similarity  uint32 acc[256] | uint32 val | 4 bytes of padding | uint64 size
 *                                                                  = 1040 bytes
 */
enum rpp_similarity {
  RPP_SIMILARITY_NILSIMSA = 0,
  RPP_SIMILARITY_HISTOGRAM = 1, /* "similarity" */
};

/* "nilsimsa", "similarity" -> the enum; anything else (NULL too) -> a negative value.  Host only. */
int rpp_similarity_kind(const char* name);
/* 2064 or 1040; 0 for a value that is no kind.  Host only. */
uint64_t rpp_similarity_state_bytes(int kind);
/* 32 or 4; 0 for a value that is no kind.  Host only. */
int rpp_similarity_digest_bytes(int kind);
/* The bytes of a message that one workgroup accumulates before it adds its
 * counts to the state; chunks of one message run on different workgroups. */
uint64_t rpp_similarity_chunk_bytes(void);

/*
 * Feeds d_data[d_offsets[b], d_offsets[b] + d_sizes[b]) (any alignment, nothing
 * outside the span is read: no slack is needed) into state b of d_states
 * (n states of rpp_similarity_state_bytes(kind) bytes, back to back).
 * Successive calls on one state hash the concatenation of their spans
 * (scan_range's chunks, scan_fragments' ranges).  d_select (NULL: every
 * message): state b is left untouched where d_select[b] == 0.  Every entry of a
 * call has a state of its own: two entries of one call must not share a state
 * (feed them by two calls).  Sizes are read on the device; asynchronous on
 * `stream`, graph-capturable; the state does not depend on scheduling.
 */
int rpp_similarity_update_batch(int kind, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                const uint8_t* d_select, uint32_t n, void* d_states, void* stream);

/* d_digests[digest_bytes * b ..] = the digest of state b (rows with
 * d_select[b] == 0 are not written).  The states are left unchanged. */
int rpp_similarity_finalize_batch(int kind, const void* d_states, const uint8_t* d_select, uint32_t n,
                                  uint8_t* d_digests, void* stream);

/*
 * scan_full in one asynchronous sequence: fresh states in the workspace,
 * update, finalize.  A file with d_select[b] == 0, or larger than max_size when
 * max_size != 0 (the reference's cmp_greater(size, max)), is not read:
 * d_has[b] = 0 and its digest row is left as it was; every other file gets
 * d_has[b] = 1.  d_workspace holds rpp_similarity_hash_workspace_bytes(kind, n)
 * bytes, 8-aligned; a smaller one is RPP_INVALID_ARGUMENT.
 */
uint64_t rpp_similarity_hash_workspace_bytes(int kind, uint32_t n);
int rpp_similarity_hash_batch(int kind, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                              const uint8_t* d_select, uint64_t max_size, uint32_t n, uint8_t* d_digests,
                              uint8_t* d_has, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* The same hashes on the host, in plain C++ over the same state layout (host
 * memory): what a caller without a GPU uses, and what the device states are
 * compared with byte for byte. */
int rpp_similarity_host_update(int kind, void* state, const uint8_t* data, uint64_t size);
int rpp_similarity_host_finalize(int kind, const void* state, uint8_t* out);

/*
 * The segmenter's match search (src/writer/segmenter.cpp,
 * include/dwarfs/writer/internal/cyclic_hash.h): the three data-parallel parts
 * of segment_and_add_data.  Choosing among matches, emitting chunks, appending
 * to blocks and the look-back bookkeeping stay with the caller; candidates come
 * from the index as it stands when a scan is launched.
 *
 *   frames   a frame is `granularity` (g) bytes; W = 1 << window_bits frames,
 *            L = W * g bytes, step = max(1, W >> increment_shift) frames.
 *   hash     of the window at frame p: over the bytes x_i = data[p g + i],
 *            a = sum x_i, b = sum (L - i) x_i, both mod 2^16; the value is
 *            a | b << 16 (rsync_hash; sliding by a byte is a += in - out,
 *            b += a - L out).
 *   filter   filter_bits = 2^k >= 64 bits: bit h & 63 of the uint64 word
 *            (h >> 6) & (words - 1); the same bytes on the host and on the
 *            device (little endian).
 *   index    of a block of F frames: slot j = 0 .. (F - W) / step holds the
 *            window at frame offset j * step (the reference's slot m = j + W /
 *            step, offset m * step - W) and its hash.  A slot is entered unless
 *            its window is L equal bytes v and an earlier slot of the same
 *            block holds an all-v window (is_existing_repeating_sequence, by
 *            content).  Every entered hash is ORed into the block's filter and
 *            into the global filter.
 *   scan     every position p in 0 .. n - W of an extent of n frames whose hash
 *            tests positive in the filter, as (p, hash), in ascending p.
 *   extend   segment_match::verify_and_extend, see rpp_segment_extend_batch.
 *
 * window_bits outside 1..20, a granularity outside 1..64 or a filter_bits that
 * is not a power of two in 64 .. 2^32 is RPP_UNSUPPORTED_CONFIG.  An extent or
 * block must be shorter than 2^32 frames.
 */
typedef struct rpp_segment_config {
  uint32_t window_bits;
  uint32_t increment_shift;
  uint32_t granularity;
  uint32_t reserved;
  uint64_t filter_bits;
} rpp_segment_config;

typedef struct rpp_segment_hit {
  uint32_t pos; /* frames from the start of the extent */
  uint32_t hash;
} rpp_segment_hit;

typedef struct rpp_segment_scan_result {
  uint64_t count;  /* hits found, also beyond the capacity */
  int32_t status;  /* RPP_OK; RPP_OUTPUT_TOO_SMALL: count > capacity; RPP_INVALID_ARGUMENT: see below */
  uint32_t reserved;
} rpp_segment_scan_result;

/* All in frames; the extent's bytes start at extent_offset of the extent data,
 * the block's at block_offset of the block data. */
typedef struct rpp_segment_candidate {
  uint64_t extent_offset;
  uint64_t block_offset;
  uint32_t pos;          /* the hit in the extent */
  uint32_t off;          /* the slot's offset in the block */
  uint32_t begin, end;   /* the extent's frames the match may cover */
  uint32_t block_frames; /* frames in the block */
  uint32_t reserved;
} rpp_segment_candidate;

typedef struct rpp_segment_match {
  uint32_t off, pos, size; /* size 0: no match, off and pos as given */
} rpp_segment_match;

int rpp_segment_check_config(const rpp_segment_config* cfg);
/* Positions one workgroup hashes; an extent is cut into tiles of this many. */
uint64_t rpp_segment_tile_frames(void);
/* frames - W + 1 window positions, (frames - W) / step + 1 slots; 0 for a
 * shorter (or too long) extent or block and for a bad config.  Host only. */
uint64_t rpp_segment_positions(const rpp_segment_config* cfg, uint64_t frames);
uint64_t rpp_segment_index_slots(const rpp_segment_config* cfg, uint64_t frames);

/*
 * Extent b is d_data[d_offsets[b], d_offsets[b] + d_sizes[b] * g): offsets in
 * bytes (any alignment), sizes in frames, both read on the device; nothing
 * outside an extent is read.  total_frames is a host-side upper bound of the
 * sum of the sizes (it sizes the workspace and the launch).  Asynchronous on
 * `stream`, no host round trip, graph-capturable.  Workspaces are 16-aligned.
 *
 * hash_batch: d_hashes[d_hash_start[b] + p] = the hash at position p of extent
 * b; d_hash_start (n + 1 entries, written) is the exclusive scan of the extents'
 * position counts.  *d_status is RPP_OK, RPP_OUTPUT_TOO_SMALL (more positions
 * than hash_capacity) or RPP_INVALID_ARGUMENT (an extent of 2^32 frames or
 * more, or sizes beyond total_frames); with an error nothing else is written.
 */
uint64_t rpp_segment_hash_workspace_bytes(uint32_t n, uint64_t total_frames);
int rpp_segment_hash_batch(const rpp_segment_config* cfg, const uint8_t* d_data, const uint64_t* d_offsets,
                           const uint64_t* d_sizes, uint32_t n, uint64_t total_frames, uint32_t* d_hashes,
                           uint64_t hash_capacity, uint64_t* d_hash_start, int32_t* d_status, void* d_workspace,
                           uint64_t workspace_bytes, void* stream);

/*
 * scan_batch: the hits of extent b are d_hits[d_hit_start[b] .. d_hit_start[b +
 * 1]), ascending in p (d_hit_start: n + 1 entries, may be NULL).  At most
 * `capacity` hits are written, the first ones; d_result->count is the full
 * count and d_result->status tells an overflow.  The order and the bytes do
 * not depend on scheduling.
 */
uint64_t rpp_segment_scan_workspace_bytes(uint32_t n, uint64_t total_frames);
int rpp_segment_scan_batch(const rpp_segment_config* cfg, const uint8_t* d_data, const uint64_t* d_offsets,
                           const uint64_t* d_sizes, uint32_t n, uint64_t total_frames, const uint64_t* d_filter,
                           rpp_segment_hit* d_hits, uint64_t capacity, uint64_t* d_hit_start,
                           rpp_segment_scan_result* d_result, void* d_workspace, uint64_t workspace_bytes,
                           void* stream);

/*
 * index_batch: block b's slots are entries d_slot_start[b] .. d_slot_start[b +
 * 1] of d_hash / d_offset (frames) / d_entered (d_slot_start: n + 1 entries,
 * written).  Entered hashes are ORed into d_block_filters[b * words ..] and
 * into d_global_filter (words = filter_bits / 64; neither is cleared).
 * max_block_frames is a host-side upper bound of the block sizes.  *d_status
 * as for hash_batch, with slot_capacity in place of hash_capacity.
 */
uint64_t rpp_segment_index_workspace_bytes(uint32_t n);
int rpp_segment_index_batch(const rpp_segment_config* cfg, const uint8_t* d_data, const uint64_t* d_offsets,
                            const uint64_t* d_sizes, uint32_t n, uint64_t max_block_frames, uint32_t* d_hash,
                            uint32_t* d_offset, uint8_t* d_entered, uint64_t slot_capacity, uint64_t* d_slot_start,
                            uint64_t* d_block_filters, uint64_t* d_global_filter, int32_t* d_status,
                            void* d_workspace, uint64_t workspace_bytes, void* stream);

/*
 * extend_batch: for candidate c (a candidate with off + W > block_frames, pos +
 * W > end or begin > pos is no match and nothing of it is read): if the L
 * window bytes differ, size = 0; otherwise begin = max(begin, pos - off), end =
 * min(end, pos + block_frames - off), prefix = the common suffix of
 * extent[begin, pos) and the block before off, suffix = the common prefix of
 * extent[pos + W, end) and the block from off + W, both in bytes rounded down
 * to whole frames; the match is (off - prefix, pos - prefix, W + prefix +
 * suffix).  Extent frames [begin, end) and the whole block must be readable.
 */
int rpp_segment_extend_batch(const rpp_segment_config* cfg, const uint8_t* d_extent_data, const uint8_t* d_block_data,
                             const rpp_segment_candidate* d_candidates, uint32_t n, rpp_segment_match* d_matches,
                             void* stream);

/* The same on the host for one extent or block (host memory), written as the
 * rolling update and a sequential index build.  host_hashes writes
 * rpp_segment_positions() values, host_index rpp_segment_index_slots() slots
 * (the filters are ORed into); host_scan returns RPP_OUTPUT_TOO_SMALL when
 * *count > capacity. */
int rpp_segment_host_hashes(const rpp_segment_config* cfg, const uint8_t* data, uint64_t frames, uint32_t* out);
int rpp_segment_host_index(const rpp_segment_config* cfg, const uint8_t* block, uint64_t frames, uint32_t* hash,
                           uint32_t* offset, uint8_t* entered, uint64_t* block_filter, uint64_t* global_filter);
int rpp_segment_host_scan(const rpp_segment_config* cfg, const uint8_t* data, uint64_t frames, const uint64_t* filter,
                          rpp_segment_hit* hits, uint64_t capacity, uint64_t* count);
int rpp_segment_host_extend(const rpp_segment_config* cfg, const uint8_t* extent_data, const uint8_t* block_data,
                            const rpp_segment_candidate* candidates, uint32_t n, rpp_segment_match* matches);

/*
 * Nilsimsa fragment ordering (src/writer/internal/similarity_ordering.cpp,
 * --order=nilsimsa): the two distance loops on the device, and the whole
 * algorithm on the host.
 *
 *   elements  n_elems rows of four uint64 words (the 32-byte nilsimsa digest as
 *             rpp_similarity_hash_batch writes it, read as little-endian words
 *             w0..w3; 16-aligned on the device), a uint64 size and a uint32
 *             rank each (all ranks distinct; a precedes b iff rank[a] <
 *             rank[b]; NULL: the element's own number).
 *   distance  sum of popcount(a.w[i] ^ b.w[i]).
 *   split     cluster_by_distance of one node: its elements are visited in list
 *             order; the first child, in creation order, whose centroid is
 *             within max_distance takes the element, else a new child while
 *             there are fewer than max_children, else the child at the smallest
 *             distance (the earliest at a tie).  Then the child's centroid adds
 *             the element: member count + 1, the 256 bit counters add the
 *             element's bits, centroid bit = counter > members / 2.
 *   chain     order_by_shortest_path over `count` entries with a `from` and a
 *             `to` row each: for i = 0 .. count - 2, among k = i + 1 .. count -
 *             1 the first k with distance(from(i), to(k)) <= 1 if there is one,
 *             else the first k at the minimum, is swapped with entry i + 1.
 *   order     duplicates, cluster tree from max_distance 128 halving down to 1,
 *             leaf chains, tree chains, collect: rpp_order_host_nilsimsa.
 *
 * The device entry points take lists that are already sorted; sorting,
 * regrouping a level by (node, child) and the tree bookkeeping are the
 * caller's.  Asynchronous on `stream`; the results do not depend on
 * scheduling.  max_children == 0 or max_cluster_size == 0 is
 * RPP_UNSUPPORTED_CONFIG (fragment_order_parser.cpp:89-97).
 */
typedef struct rpp_order_stats {
  uint64_t fallbacks;          /* elements placed by the full-node rule */
  uint64_t fallback_ties;      /* ... of them, with two children at the smallest distance */
  uint64_t chain_early_stops;  /* chain steps that ended on a distance <= 1 */
  uint32_t depth;              /* split levels, 1 (the root only) .. 8; 0 for an empty index */
  uint32_t leaves;             /* clusters that were not split again */
  uint32_t largest_leaf;
  uint32_t largest_final_leaf; /* the largest leaf made at max_distance == 1 */
  uint32_t largest_node;       /* the most children of one node */
  uint32_t duplicate_groups;
  uint32_t unique;             /* elements left after the duplicates */
  uint32_t reserved;
} rpp_order_stats;

int rpp_order_check_options(uint32_t max_children, uint32_t max_cluster_size);
/* The children one pass of the split compares an element with, the entries one
 * pass of the chain covers, and the longest segment the chain keeps in LDS. */
uint32_t rpp_order_split_pass_children(void);
uint32_t rpp_order_chain_threads(void);
uint32_t rpp_order_chain_stage_rows(void);

/*
 * split_batch: node j's elements are d_index[d_node_start[j] .. d_node_start[j +
 * 1]) (n_nodes + 1 starts).  d_child[slot] = the child, numbered in creation
 * order, that the element of that slot went to; d_nchildren[j] = the node's
 * child count.  Node j keeps its children's centroids and counters in child
 * slots d_child_base[j] .. + min(elements, max_children) of the workspace, which
 * has child_slots slots = rpp_order_split_workspace_bytes(child_slots) bytes,
 * 16-aligned, and needs no initialisation; the nodes' slot ranges must not
 * overlap.  A node whose range does not fit, or that holds an id >= n_elems,
 * gets d_nchildren[j] = 0xffffffff and nothing outside its own ranges is
 * touched.  One launch; a tree level depends on the level before, so the
 * caller launches level by level.  max_distance > 256 is RPP_INVALID_ARGUMENT.
 */
uint64_t rpp_order_split_workspace_bytes(uint64_t child_slots);
int rpp_order_split_batch(const uint64_t* d_bits, uint32_t n_elems, const uint32_t* d_index,
                          const uint32_t* d_node_start, const uint64_t* d_child_base, uint32_t n_nodes,
                          uint64_t child_slots, uint32_t max_children, uint32_t max_distance, uint32_t* d_child,
                          uint32_t* d_nchildren, void* d_workspace, uint64_t workspace_bytes, void* stream);

/*
 * chain_batch: segment s is entries d_seg_start[s] .. d_seg_start[s + 1]
 * (n_segments + 1 starts); entry e has the rows d_from_ids[e] and d_to_ids[e]
 * (the same pointer for a leaf).  d_perm[d_seg_start[s] + i] = the entry,
 * counted from the segment's start, that the chain leaves at place i.  A
 * segment of 0 or 1 entries is the identity; one with an id >= n_elems is
 * filled with 0xffffffff.  A segment longer than rpp_order_chain_stage_rows()
 * is chained in global memory, in d_perm itself:
 * rpp_order_chain_workspace_bytes is 0 for every size.
 */
uint64_t rpp_order_chain_workspace_bytes(uint64_t total_entries);
int rpp_order_chain_batch(const uint64_t* d_bits, uint32_t n_elems, const uint32_t* d_from_ids,
                          const uint32_t* d_to_ids, const uint32_t* d_seg_start, uint32_t n_segments, uint32_t* d_perm,
                          void* stream);

/* The same on the host (host memory), written as the reference's sequential
 * loops: one node's split, one segment's chain, and the whole order of `index`
 * (n_index ids, any order, no id twice) into out[n_index]; stats may be NULL. */
int rpp_order_host_split(const uint64_t* bits, uint32_t n_elems, const uint32_t* index, uint32_t m,
                         uint32_t max_children, uint32_t max_distance, uint32_t* child, uint32_t* nchildren);
int rpp_order_host_chain(const uint64_t* bits, uint32_t n_elems, const uint32_t* from_ids, const uint32_t* to_ids,
                         uint32_t count, uint32_t* perm);
int rpp_order_host_nilsimsa(const uint64_t* bits, const uint64_t* sizes, const uint32_t* rank, uint32_t n_elems,
                            const uint32_t* index, uint32_t n_index, uint32_t max_children,
                            uint32_t max_cluster_size, uint32_t* out, rpp_order_stats* stats);

/*
 * lz4: the LZ4 block codec (src/compression/lz4.cpp), compression types LZ4 = 3
 * and LZ4HC = 4 (include/dwarfs/compression.h:34-42), which decode alike.
 *
 *   payload   uint32 little-endian uncompressed size (rpp_lz4_frame_header /
 *             rpp_lz4_parse_frame, lz4.cpp:88-106,127-169), then one LZ4 block
 *             (the block format, not the frame format).
 *   block     sequences: a token (high nibble literal length, low nibble match
 *             length - 4; a nibble of 15 is followed by bytes that are added,
 *             up to and including the first below 255), the literals, a 2-byte
 *             little-endian offset 1..65535, the match length's bytes.  The
 *             last sequence ends after its literals.  A match may overlap its
 *             destination (offset < length: a repeated pattern).
 *   decode    one wave per stream.  RPP_CORRUPT_INPUT when a token, an
 *             extension byte, a literal or an offset would be read at or past
 *             the stream's end; when a copy would pass the stated uncompressed
 *             size; when an offset is 0 or reaches before the output's start;
 *             when the stream ends before exactly the stated size has been
 *             produced.  The last is stricter than the reference, which accepts
 *             a short stream silently (lz4.cpp:143-152); a valid image never
 *             holds one.  Nothing outside [out, out + size) is written and
 *             nothing outside the stream is read, whatever the bytes are; what
 *             the sequences before the failing one produced stays written.  The
 *             end-of-block rules that LZ4_decompress_safe enforces are not
 *             checked.
 *   encode    deterministic, without atomics: chunks of rpp_lz4_chunk_bytes(),
 *             searched in steps of rpp_lz4_step_positions() positions (lookups
 *             of a step before its inserts), greedy, emitted as ONE block whose
 *             literal runs span chunk boundaries; the complete definition is in
 *             dwarfs_amd/csrc/lz4_host.cpp.  The last 5 bytes are literals, the
 *             last match starts at least 12 bytes before the end, a block below
 *             13 bytes is one literal run.  Not liblz4's bytes; any LZ4 decoder
 *             reads them.  Blocks hold at most RPP_LZ4_MAX_BLOCK bytes (-S 30;
 *             LZ4_compress_default takes an int): a longer one gets
 *             RPP_INVALID_ARGUMENT in its status.
 *
 * The *_batch calls take device pointers and are asynchronous on `stream`.
 */
#define RPP_CORRUPT_INPUT (-8)
#define RPP_LZ4_MAX_BLOCK (UINT64_C(1) << 30)

/* Worst-case encoded bytes of an n-byte block: LZ4_compressBound's n + n / 255 + 16. */
uint64_t rpp_lz4_bound(uint64_t n);
/* The encoder's chunk size and the positions of one search step. */
uint32_t rpp_lz4_chunk_bytes(void);
uint32_t rpp_lz4_step_positions(void);

/* Writes the 4-byte size prefix to out and returns 4. */
size_t rpp_lz4_frame_header(uint32_t uncompressed_bytes, uint8_t* out);
/* Returns 4, the LZ4 block's offset in the payload; RPP_TRUNCATED_INPUT for a payload below 4 bytes. */
long rpp_lz4_parse_frame(const uint8_t* data, size_t size, uint32_t* uncompressed_bytes);

/*
 * Decodes nblocks LZ4 blocks: stream b is d_in[d_in_offsets[b] .. + d_in_bytes[b])
 * (any alignment) and produces exactly d_out_bytes[b] bytes at d_out +
 * d_out_offsets[b]; d_status[b] is RPP_OK or RPP_CORRUPT_INPUT.
 */
int rpp_lz4_decode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                         uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets,
                         const uint64_t* d_out_bytes, int32_t* d_status, void* stream);

/*
 * Encodes nblocks blocks: block b is d_in[d_in_offsets[b] .. + d_in_bytes[b]) and
 * its LZ4 block goes to d_out + d_out_offsets[b], a region of rpp_lz4_bound(n)
 * bytes; d_out_bytes[b] is its size, d_flags[b] is 1 when 4 + size >= n (the
 * writer's bad_compression_ratio_error: store the block as NONE) and else 0.  The
 * caller owns the 16-aligned workspace of rpp_lz4_encode_workspace_bytes(
 * total_bytes, nblocks) bytes, total_bytes >= the sum of d_in_bytes; if the device
 * finds the sum larger, every status is RPP_INVALID_ARGUMENT and nothing is
 * encoded.  No initialisation of the workspace is needed.
 */
uint64_t rpp_lz4_encode_workspace_bytes(uint64_t total_bytes, uint32_t nblocks);
int rpp_lz4_encode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                         uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets, uint64_t* d_out_bytes,
                         uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                         uint64_t workspace_bytes, void* stream);

/* The two kernels' contracts as sequential host code (host memory): the CPU path
 * and the yardstick.  rpp_lz4_host_encode writes exactly the kernel's bytes;
 * capacity must be at least rpp_lz4_bound(n), else RPP_OUTPUT_TOO_SMALL. */
int rpp_lz4_host_decode(const uint8_t* in, uint64_t in_bytes, uint8_t* out, uint64_t out_bytes);
int rpp_lz4_host_encode(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                        uint32_t* bad_ratio);

/*
 * zstd: the Zstandard block codec (src/compression/zstd.cpp:424-483),
 * compression type ZSTD = 2 (include/dwarfs/compression.h:34-42).
 *
 *   payload   ONE Zstandard frame (RFC 8878), as ZSTD_compress2 writes it
 *             (zstd.cpp:424-441): single-segment or with a Window_Descriptor,
 *             any Frame_Content_Size width, no dictionary (a Dictionary_ID of 0
 *             is accepted).  The reader takes the buffer size from the frame
 *             header (rpp_zstd_frame_info) and states it to the decoder.
 *   decode    three launches: index (one lane per frame: frame and block
 *             headers, who supplies a Treeless tree or a Repeat table), entropy
 *             (one wave per block: Huffman literals, 4 streams in 4 lanes, and
 *             FSE sequences into records in the workspace), execute (one wave per
 *             frame: repeat offsets, literal and match copies).  Raw, RLE and
 *             Compressed blocks; Raw, RLE, Compressed and Treeless literals;
 *             Predefined, RLE, FSE_Compressed and Repeat tables.  The complete
 *             list of what is RPP_CORRUPT_INPUT is at the top of
 *             dwarfs_amd/csrc/zstd_host.cpp; it includes three rules of the RFC
 *             that libzstd 1.4.8 does not enforce (reserved mode bits, unused
 *             sequence bits, an offset of 0 through the repeat rule), any byte
 *             behind the frame, and a frame that does not produce exactly the
 *             stated size.  A frame without Frame_Content_Size is decoded; the
 *             stated size stands in.  The Content_Checksum's 4 bytes must be
 *             there when flagged and are skipped, NOT verified (XXH64; every
 *             section carries XXH3-64 already).  Nothing outside a frame's input
 *             is read and nothing outside its output region is written, whatever
 *             the bytes are; a refused frame's output region is unspecified.
 *             Frames and contents hold less than 4 GiB each: a larger one gets
 *             RPP_INVALID_ARGUMENT in its status.
 *
 *   encode    a deterministic encoder of its own: ONE frame per block, one
 *             Zstandard block per 32 KiB chunk of the LZ4 encoder's match
 *             search (same sequences), Huffman literals and FSE sequences with
 *             the three Predefined tables.  Four launches behind the search's
 *             two: entropy (one wave per chunk), place (one wave per frame),
 *             emit (one wave per chunk).  The complete definition is at the top
 *             of dwarfs_amd/csrc/zstd_encode_host.cpp.  Not libzstd's bytes; any
 *             Zstandard decoder reads them.  Limits: predefined tables only and
 *             no repeat offsets unless the options word of the *_opt calls
 *             asks for them, 32 KiB blocks, a 64 KiB match window, no
 *             compression level, no Content_Checksum.  Blocks hold at most
 *             RPP_LZ4_MAX_BLOCK bytes: a longer one gets RPP_INVALID_ARGUMENT
 *             in its status.
 *
 * The *_batch calls take device pointers and are asynchronous on `stream`.
 */
#define RPP_ZSTD_FLAG_SINGLE_SEGMENT 1u
#define RPP_ZSTD_FLAG_CHECKSUM 2u
#define RPP_ZSTD_FLAG_CONTENT_SIZE 4u

/* Parses the frame header (host memory): its length, or RPP_CORRUPT_INPUT.  *content_size is 0 without
 * RPP_ZSTD_FLAG_CONTENT_SIZE in *flags; *window is the content size for a single-segment frame.  Any of the
 * three may be NULL. */
long rpp_zstd_frame_info(const uint8_t* data, size_t size, uint64_t* content_size, uint64_t* window,
                         uint32_t* flags);
/* Walks the block headers of a frame (host memory): the number of blocks, or RPP_CORRUPT_INPUT when a header
 * cannot be read, a block passes the end or has the Reserved type. */
long rpp_zstd_count_blocks(const uint8_t* data, size_t size);

/*
 * Decodes nframes frames: frame b is d_in[d_in_offsets[b] .. + d_in_bytes[b]) (any
 * alignment, no padding needed) and produces exactly d_out_bytes[b] bytes at
 * d_out + d_out_offsets[b]; d_status[b] is RPP_OK, RPP_CORRUPT_INPUT, or
 * RPP_OUTPUT_TOO_SMALL for a frame that does not fit the workspace.  max_blocks
 * is the caller's promise of the blocks of all frames together (the sum of
 * rpp_zstd_count_blocks), and the 16-aligned workspace holds
 * rpp_zstd_decode_workspace_bytes(total_out_bytes, max_blocks) bytes,
 * total_out_bytes >= the sum of d_out_bytes (about 5 bytes per output byte).
 * Slots are dealt out frame by frame: a frame with more blocks, or more output,
 * than is left takes none, gets RPP_OUTPUT_TOO_SMALL, and nothing of it is
 * decoded; the frames behind it go on.  A frame that rpp_zstd_count_blocks
 * refuses is promised one block.  Frames that are refused at a block, or for
 * what follows the last block, get their slots after all other frames, from what
 * these leave: where the blocks before the failing one fit there, what they
 * produce is written as rpp_zstd_host_decode writes it, else nothing of the
 * frame is decoded; RPP_CORRUPT_INPUT either way, and never at the cost of
 * another frame's slots.  max_blocks < nframes returns
 * RPP_OUTPUT_TOO_SMALL at once; nframes == 0 returns RPP_OK at once.  No
 * initialisation of the workspace is needed.
 */
uint64_t rpp_zstd_decode_workspace_bytes(uint64_t total_out_bytes, uint32_t max_blocks);
int rpp_zstd_decode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                          uint32_t nframes, uint8_t* d_out, const uint64_t* d_out_offsets,
                          const uint64_t* d_out_bytes, int32_t* d_status, uint32_t max_blocks, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);

/* The kernels' contract as sequential host code (host memory): the CPU path and the yardstick. */
int rpp_zstd_host_decode(const uint8_t* in, uint64_t in_bytes, uint8_t* out, uint64_t out_bytes);

/* Worst-case bytes of an n-byte block's frame: every chunk stored Raw, plus the frame header. */
uint64_t rpp_zstd_bound(uint64_t n);

/*
 * Encodes nblocks blocks: block b is d_in[d_in_offsets[b] .. + d_in_bytes[b]) and
 * its frame goes to d_out + d_out_offsets[b], a region of rpp_zstd_bound(n) bytes;
 * d_out_bytes[b] is its size, d_flags[b] is 1 when size >= n (the writer's
 * bad_compression_ratio_error, zstd.cpp:435: store the block as NONE) and else 0.
 * The caller owns the 16-aligned workspace of rpp_zstd_encode_workspace_bytes(
 * total_bytes, nblocks) bytes, total_bytes >= the sum of d_in_bytes; if the device
 * finds the sum larger, every status is RPP_INVALID_ARGUMENT and nothing is
 * encoded.  nblocks == 0 returns RPP_OK at once.  No initialisation of the
 * workspace is needed.
 */
uint64_t rpp_zstd_encode_workspace_bytes(uint64_t total_bytes, uint32_t nblocks);
int rpp_zstd_encode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                          uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets, uint64_t* d_out_bytes,
                          uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);

/* The encode kernels' contract as sequential host code (host memory): exactly their bytes.  capacity must be
 * at least rpp_zstd_bound(n), else RPP_OUTPUT_TOO_SMALL. */
int rpp_zstd_host_encode(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                         uint32_t* bad_ratio);

/*
 * The encoder's options word.  0 writes the bytes of rpp_zstd_encode_batch and rpp_zstd_host_encode, which
 * both are the options-0 calls of the functions below.  Any other bit set: RPP_INVALID_ARGUMENT.
 *   RPP_ZSTD_ENC_TABLES  per block and table (LL, OF, ML) the mode RLE (one code in the block),
 *                        FSE_Compressed (the block's own distribution, accuracy log 5 or 6, when its
 *                        description pays for itself by an integer estimate) or Predefined; never Repeat_Mode.
 *   RPP_ZSTD_ENC_REPEAT  Repeated_Offset1 and Repeated_Offset2 codes for an offset equal to that of one of
 *                        the two sequences before it in the same 32 KiB chunk; never Repeated_Offset3, and
 *                        a chunk's first sequence is written in full.
 * The rules are stated in dwarfs_amd/csrc/zstd_enc_common.h and at the top of zstd_encode_host.cpp.  The
 * bound (rpp_zstd_bound), the workspace (rpp_zstd_encode_workspace_bytes) and every other part of the
 * contract are those of the functions above.
 */
#define RPP_ZSTD_ENC_TABLES 1u
#define RPP_ZSTD_ENC_REPEAT 2u
int rpp_zstd_encode_batch_opt(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                              uint32_t nblocks, uint32_t options, uint8_t* d_out, const uint64_t* d_out_offsets,
                              uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                              void* d_workspace, uint64_t workspace_bytes, void* stream);
int rpp_zstd_host_encode_opt(const uint8_t* in, uint64_t n, uint32_t options, uint8_t* out, uint64_t capacity,
                             uint64_t* out_bytes, uint32_t* bad_ratio);

/*
 * The search word of the LZ4 and Zstandard encoders: depth | RPP_SEARCH_LAZY, depth 1, 2, 4 or 8.  0 is the
 * search of the calls above (one candidate per hash value, the first position that matches), which are the
 * search-0 calls of the functions below; any other word is RPP_INVALID_ARGUMENT.
 *   depth            a hash value keeps its `depth` highest positions; a position scores each of them (the
 *                    common prefix, up to 64 bytes) and matches the best one, of equals the nearest.
 *   RPP_SEARCH_LAZY  a position is passed over when the next position of the same 64-position step scores
 *                    strictly higher.
 * Depth 1 without RPP_SEARCH_LAZY writes the bytes of search 0 (from another kernel).  The complete definition
 * is at the top of dwarfs_amd/csrc/lz4_host.cpp.  The match window stays 64 KiB, candidates come from earlier
 * steps only, and no compression level maps to a word.  Bounds, workspaces, flags, statuses and every other
 * part of the contracts are those of rpp_lz4_encode_batch, rpp_zstd_encode_batch_opt and the host calls.
 */
#define RPP_SEARCH_LAZY 0x100u
int rpp_lz4_encode_batch_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                uint32_t nblocks, uint32_t search, uint8_t* d_out, const uint64_t* d_out_offsets,
                                uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                                void* d_workspace, uint64_t workspace_bytes, void* stream);
int rpp_lz4_host_encode_search(const uint8_t* in, uint64_t n, uint32_t search, uint8_t* out, uint64_t capacity,
                               uint64_t* out_bytes, uint32_t* bad_ratio);
int rpp_zstd_encode_batch_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                 uint32_t nblocks, uint32_t options, uint32_t search, uint8_t* d_out,
                                 const uint64_t* d_out_offsets, uint64_t* d_out_bytes, uint32_t* d_flags,
                                 int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                                 uint64_t workspace_bytes, void* stream);
int rpp_zstd_host_encode_search(const uint8_t* in, uint64_t n, uint32_t options, uint32_t search, uint8_t* out,
                                uint64_t capacity, uint64_t* out_bytes, uint32_t* bad_ratio);

/*
 * The incompressible categorizer of the scan (src/writer/categorizer/incompressible_categorizer.cpp): which
 * pieces of a file are not worth a compressor.  An extent (a contiguous run of file data) is cut by the caller
 * into pieces of block_size bytes (the last one may be shorter); piece p is d_in + d_in_offsets[p], d_in_bytes[p]
 * bytes (at most RPP_LZ4_MAX_BLOCK), and extent e holds the pieces d_piece_base[e] .. d_piece_base[e + 1]
 * (nextents + 1 entries that do not decrease and end at or below npieces; equal entries: an empty extent).
 *   d_sizes[p]     the size of the one frame that rpp_zstd_encode_batch_search(options, search) writes for the
 *                  piece, header included.  This encoder's size, not libzstd's; no frame is written.
 *   d_verdicts[p]  1 (incompressible) iff double(size) >= max_ratio * double(n), else 0
 *   d_totals       per extent RPP_INCOMPRESSIBLE_TOTALS numbers: total_in, total_out, blocks,
 *                  incompressible_blocks, and the single-fragment verdict (blocks > 0 and
 *                  double(total_out) >= max_ratio * double(total_in))
 *   d_frag_rows    rows of (category, bytes), two uint64 each; npieces rows.  With generate_fragments, extent e's
 *                  run-length list over its pieces (neighbours of one verdict merged; category 0 the default,
 *                  1 incompressible) stands in the rows d_piece_base[e] .. + d_frag_count[e]; the rows behind
 *                  them are not written.  Without it d_frag_count[e] is 0 and no row is written.
 *   d_status[p]    RPP_OK, or RPP_INVALID_ARGUMENT for a piece that is too large or when the pieces hold more
 *                  than total_bytes (then every piece); such a piece has size 0 and verdict 0.
 * An unknown options bit or search word is RPP_INVALID_ARGUMENT; npieces == 0 is RPP_OK and writes nothing; a
 * 16-aligned workspace below rpp_incompressible_workspace_bytes(total_bytes, npieces, nextents) bytes is
 * RPP_OUTPUT_TOO_SMALL.  Asynchronous on the stream.  rpp_incompressible_host_scan computes the same numbers on the
 * host (it refuses a d_piece_base that decreases or passes npieces; the kernels clamp).  The complete definition
 * is at the top of dwarfs_amd/csrc/scan/incompressible_host.cpp.
 */
#define RPP_INCOMPRESSIBLE_TOTALS 5
uint64_t rpp_incompressible_workspace_bytes(uint64_t total_bytes, uint32_t npieces, uint32_t nextents);
int rpp_incompressible_scan_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                  uint32_t npieces, const uint32_t* d_piece_base, uint32_t nextents, double max_ratio,
                                  uint32_t generate_fragments, uint32_t options, uint32_t search, uint64_t* d_sizes,
                                  uint32_t* d_verdicts, uint64_t* d_totals, uint64_t* d_frag_rows,
                                  uint32_t* d_frag_count, int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                                  uint64_t workspace_bytes, void* stream);
int rpp_incompressible_host_scan(const uint8_t* in, const uint64_t* in_offsets, const uint64_t* in_bytes,
                                 uint32_t npieces, const uint32_t* piece_base, uint32_t nextents, double max_ratio,
                                 uint32_t generate_fragments, uint32_t options, uint32_t search, uint64_t* sizes,
                                 uint32_t* verdicts, uint64_t* totals, uint64_t* frag_rows, uint32_t* frag_count,
                                 int32_t* status);

/*
 * Long-distance matching for the Zstandard encoder: a third opt-in word beside `options` and `search`, the mirror
 * of the reference's `long` option (src/compression/zstd.cpp:69, :404-406).  long_mode 0 is the *_search call:
 * the same kernels, the same launches, the same bytes.  long_mode 1 adds matches of at least 64 bytes against
 * anything earlier in the same block (a table of the first occurrence of every 32-byte window on a 32-byte grid),
 * merged with the short search's sequences; a block then holds at most RPP_ZSTD_LONG_MAX_BLOCK bytes, and a larger
 * one has the status of an over-size block.  Any other long_mode is RPP_INVALID_ARGUMENT.  LZ4 cannot express
 * these offsets and has no such word.  The complete definition is at the top of
 * dwarfs_amd/csrc/zstd_long_host.cpp.  Frames are stock RFC 8878 with a window of the block's size; rpp_zstd_bound,
 * flags, statuses and every other part of the contracts are those of the *_search calls.  The workspace of the
 * batch calls is rpp_zstd_encode_workspace_bytes_long(total_bytes, nblocks, long_mode) bytes (with long_mode 0
 * rpp_zstd_encode_workspace_bytes), that of the scan rpp_incompressible_workspace_bytes_long.
 * rpp_zstd_host_long_sequences is a debug export of the host side: the (position, length, offset) triples, three
 * uint32 each, that the frame of (search, long_mode) is written from; *count gets their number, and a capacity
 * (in triples) below it is RPP_OUTPUT_TOO_SMALL.
 */
#define RPP_ZSTD_LONG_MAX_BLOCK (UINT64_C(1) << 27)
uint64_t rpp_zstd_encode_workspace_bytes_long(uint64_t total_bytes, uint32_t nblocks, uint32_t long_mode);
int rpp_zstd_encode_batch_long(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                               uint32_t nblocks, uint32_t options, uint32_t search, uint32_t long_mode, uint8_t* d_out,
                               const uint64_t* d_out_offsets, uint64_t* d_out_bytes, uint32_t* d_flags,
                               int32_t* d_status, uint64_t total_bytes, void* d_workspace, uint64_t workspace_bytes,
                               void* stream);
int rpp_zstd_host_encode_long(const uint8_t* in, uint64_t n, uint32_t options, uint32_t search, uint32_t long_mode,
                              uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint32_t* bad_ratio);
int rpp_zstd_host_long_sequences(const uint8_t* in, uint64_t n, uint32_t search, uint32_t long_mode,
                                 uint32_t* triples, uint64_t capacity, uint64_t* count);
uint64_t rpp_incompressible_workspace_bytes_long(uint64_t total_bytes, uint32_t npieces, uint32_t nextents,
                                                 uint32_t long_mode);
int rpp_incompressible_scan_batch_long(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                       uint32_t npieces, const uint32_t* d_piece_base, uint32_t nextents,
                                       double max_ratio, uint32_t generate_fragments, uint32_t options,
                                       uint32_t search, uint32_t long_mode, uint64_t* d_sizes, uint32_t* d_verdicts,
                                       uint64_t* d_totals, uint64_t* d_frag_rows, uint32_t* d_frag_count,
                                       int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                                       uint64_t workspace_bytes, void* stream);
int rpp_incompressible_host_scan_long(const uint8_t* in, const uint64_t* in_offsets, const uint64_t* in_bytes,
                                      uint32_t npieces, const uint32_t* piece_base, uint32_t nextents, double max_ratio,
                                      uint32_t generate_fragments, uint32_t options, uint32_t search,
                                      uint32_t long_mode, uint64_t* sizes, uint32_t* verdicts, uint64_t* totals,
                                      uint64_t* frag_rows, uint32_t* frag_count, int32_t* status);

/*
 * File extraction: chunks of decoded blocks become files (the readers that walk every file's chunk list,
 * src/utility/filesystem_extractor.cpp and dwarfsck --checksum, tools/src/dwarfsck_main.cpp do_checksum).  A file is
 * a list of chunks (thrift/metadata.thrift, `chunk`); a chunk row is this project's own: `size` is 64-bit because a
 * row with block == RPP_CHUNK_HOLE is a hole, `size` zero bytes without a source.
 *   blocks      block b is d_blocks[d_block_offsets[b] .. + d_block_sizes[b]), any alignment inside a buffer of
 *               blocks_bytes bytes whose address is 16-aligned and whose allocation is padded to a multiple of 16:
 *               loads are aligned and stay inside [0, round_up(blocks_bytes, 16)).
 *   files       CSR: file f holds the chunks d_file_first_chunk[f] .. d_file_first_chunk[f + 1] (nfiles + 1 entries
 *               from 0 to nchunks that do not decrease); chunk c's bytes go to d_out[d_chunk_dst[c] .. + size).
 *               d_chunk_dst has nchunks + 1 entries and does not decrease: the exclusive scan of the chunk sizes laid
 *               over the files' places in d_out (its last entry is the end of the last chunk).  d_out is 16-aligned.
 *   bad chunk   a chunk is bad when block >= nblocks and it is no hole; when offset + size > d_block_sizes[block]
 *               (in 64 bits) or the block itself passes blocks_bytes; when d_chunk_dst[c] + size > out_bytes or
 *               > d_chunk_dst[c + 1] (it would run into its neighbour).  Its file's d_file_status is RPP_BAD_CHUNK
 *               and its destination bytes are left as they are; every other chunk, of the same file too, is copied.
 *   d_file_status  nfiles entries, RPP_OK or RPP_BAD_CHUNK; the call writes every one.
 * Bytes of d_out that no chunk covers are not written.  The 16-aligned workspace holds
 * rpp_extract_workspace_bytes(nchunks, nfiles, out_bytes) bytes and needs no initialisation; a smaller one, a null
 * pointer where bytes are needed, a misaligned d_blocks, d_out or workspace, or nchunks > 0 with nfiles == 0 is
 * RPP_INVALID_ARGUMENT.  nchunks == 0 clears the statuses and is RPP_OK.  rpp_extract_tile_bytes is the gather
 * kernel's tile of output bytes (for tests and tools).  rpp_extract_host_gather is the definition (host memory, any
 * alignment; it also refuses a file table that decreases or does not span 0 .. nchunks, where the kernels clamp); its
 * rules are at the top of dwarfs_amd/csrc/extract/extract_host.cpp.  Where d_chunk_dst decreases, which bytes of
 * d_out the device call writes is unspecified, but no store leaves a good chunk's destination and no load its block.
 */
#define RPP_BAD_CHUNK (-9)
#define RPP_CHUNK_HOLE 0xFFFFFFFFu
typedef struct rpp_chunk {
  uint32_t block;
  uint32_t offset;
  uint64_t size;
} rpp_chunk;
uint64_t rpp_extract_tile_bytes(void);
uint64_t rpp_extract_workspace_bytes(uint64_t nchunks, uint32_t nfiles, uint64_t out_bytes);
int rpp_extract_gather_batch(const uint8_t* d_blocks, uint64_t blocks_bytes, const uint64_t* d_block_offsets,
                             const uint64_t* d_block_sizes, uint32_t nblocks, const rpp_chunk* d_chunks,
                             const uint64_t* d_chunk_dst, uint64_t nchunks, const uint64_t* d_file_first_chunk,
                             uint32_t nfiles, uint8_t* d_out, uint64_t out_bytes, int32_t* d_file_status,
                             void* d_workspace, uint64_t workspace_bytes, void* stream);
int rpp_extract_host_gather(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* block_offsets,
                            const uint64_t* block_sizes, uint32_t nblocks, const rpp_chunk* chunks,
                            const uint64_t* chunk_dst, uint64_t nchunks, const uint64_t* file_first_chunk,
                            uint32_t nfiles, uint8_t* out, uint64_t out_bytes, int32_t* file_status);

/*
 * File digests by name: what `dwarfsck --checksum=ALGO` and `mkdwarfs --file-hash=ALGO` accept beyond the two XXH3
 * hashes (dwarfs::checksum, src/checksum.cpp: any digest that EVP_get_digestbyname finds).  Thirteen digests are
 * computed here -- MD5, SHA-1, SHA-224/256/384/512, SHA-512/224, SHA3-224/256/384/512 and unkeyed BLAKE2b-512 and
 * BLAKE2s-256 with default parameters -- and the three of rpp_file_hash are forwarded.  The enum has a numbering
 * of its own: a value of one enum means nothing to the other group's calls.  Digests are in each standard's byte
 * order, which is what EVP_DigestFinal_ex returns.
 *
 *   rpp_digest_algo    the enum of a name, or a negative value (NULL too).  OpenSSL's names ("md5", "sha1",
 *                      "sha224", "sha256", "sha384", "sha512", "sha512-224", "sha512-256", "sha3-224", "sha3-256",
 *                      "sha3-384", "sha3-512", "blake2b512", "blake2s256") match in any letter case, as
 *                      EVP_get_digestbyname matches them; "xxh3-64" and "xxh3-128" match exactly, as checksum.cpp
 *                      compares them.  Host only.
 *   rpp_digest_bytes   the digest's size in bytes; 0 for a value that is no algorithm.  Host only.
 *   rpp_digest_batch   the contract of rpp_file_hash_batch: file b = d_data[d_offsets[b], + d_sizes[b]) goes to
 *                      d_digest[rpp_digest_bytes(algo) * b ..], tightly packed; with d_select (NULL: every file) a
 *                      file whose byte is 0 is not read and its row is not written.  n == 0 is RPP_OK; an unknown
 *                      algo, or a null pointer with work to do, is RPP_INVALID_ARGUMENT before anything is launched.
 *                      One lane per file (the chain of a Merkle-Damgard or sponge hash does not split); whole blocks
 *                      of a payload on a 16-byte boundary (8 for SHA-3) are read by 16-byte loads, everything else
 *                      byte by byte.  Files are below 2^61 bytes.
 *   rpp_digest_host    the definition on host memory, on the same round functions (the padding rules are at the top
 *                      of dwarfs_amd/csrc/digest/digest_host.cpp).  It has the thirteen and "sha512-256"; the two
 *                      XXH3 hashes have no host form and are RPP_INVALID_ARGUMENT.
 */
enum rpp_digest_id {
  RPP_DIGEST_MD5 = 0,
  RPP_DIGEST_SHA1 = 1,
  RPP_DIGEST_SHA224 = 2,
  RPP_DIGEST_SHA256 = 3,
  RPP_DIGEST_SHA384 = 4,
  RPP_DIGEST_SHA512 = 5,
  RPP_DIGEST_SHA512_224 = 6,
  RPP_DIGEST_SHA3_224 = 7,
  RPP_DIGEST_SHA3_256 = 8,
  RPP_DIGEST_SHA3_384 = 9,
  RPP_DIGEST_SHA3_512 = 10,
  RPP_DIGEST_BLAKE2B512 = 11,
  RPP_DIGEST_BLAKE2S256 = 12,
  RPP_DIGEST_XXH3_64 = 13,
  RPP_DIGEST_XXH3_128 = 14,
  RPP_DIGEST_SHA512_256 = 15,
  RPP_DIGEST_COUNT = 16,
};
int rpp_digest_algo(const char* name);
int rpp_digest_bytes(int algo);
int rpp_digest_batch(int algo, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                     const uint8_t* d_select, uint32_t n, uint8_t* d_digest, void* stream);
int rpp_digest_host(int algo, const uint8_t* data, const uint64_t* offsets, const uint64_t* sizes,
                    const uint8_t* select, uint32_t n, uint8_t* digest);

#ifdef __cplusplus
}
#endif

#endif /* RICEPP_AMD_H */
