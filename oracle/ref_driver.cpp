// ref_driver.cpp -- a C ABI over the public entry points of the reference (mhx/dwarfs), compiled together with
// the reference's own translation units into oracle/_ref/libdwarfs_ref.so by oracle/ref_build.py.
//
// TEST INFRASTRUCTURE ONLY.  Nothing of the reference is restated here: the codec goes through
// ricepp::create_encoder<uint16_t> / create_decoder<uint16_t>, the hashes through the reference's classes.  The
// reference's headers are included at build time only; neither they nor the library are part of this repository.
//
// Status codes are those of oracle/ricepp_oracle.c; exceptions become status codes.

#include <bit>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <exception>
#include <span>
#include <stdexcept>
#include <vector>

#include <ricepp/codec_config.h>
#include <ricepp/create_decoder.h>
#include <ricepp/create_encoder.h>

#include <dwarfs/writer/internal/cyclic_hash.h>
#include <dwarfs/writer/internal/nilsimsa.h>
#include <dwarfs/writer/internal/similarity.h>

#ifndef REF_BUILD_FLAGS
#define REF_BUILD_FLAGS "unknown"
#endif

namespace {

constexpr int kOk = 0;
constexpr int kUnsupportedConfig = -1;
constexpr int kTruncatedInput = -2;
constexpr int kInvalidArgument = -3;
constexpr int kOutputTooSmall = -4;
constexpr int kException = -5;

struct ref_config {
  uint32_t block_size;
  uint32_t component_stream_count;
  uint32_t big_endian;
  uint32_t unused_lsb_count;
};

ricepp::codec_config to_config(ref_config const* c) {
  return {.block_size = c->block_size,
          .component_stream_count = c->component_stream_count,
          .byteorder = c->big_endian ? std::endian::big : std::endian::little,
          .unused_lsb_count = c->unused_lsb_count};
}

template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (std::out_of_range const&) {
    return kTruncatedInput;
  } catch (std::runtime_error const& e) {
    return std::strcmp(e.what(), "Unsupported configuration") == 0 ? kUnsupportedConfig : kException;
  } catch (std::exception const&) {
    return kException;
  }
}

// What the reference leaves undefined and a release build would run into: block size 0 (chunk(0) never
// advances), an unused_lsb_count of 16 or more (the traits assert less in a debug build), and fewer pixels than
// component streams (codec::encode reads input[i] for every stream, an empty input included).
int check_defined(ref_config const* c, size_t n) {
  if (c->block_size == 0 || c->unused_lsb_count >= 16) return kUnsupportedConfig;
  if (c->component_stream_count > 0 && n < c->component_stream_count) return kInvalidArgument;
  return kOk;
}

} // namespace

extern "C" {

char const* ref_build_flags() { return REF_BUILD_FLAGS; }

int ref_ricepp_worst_case_bytes(ref_config const* c, size_t n, size_t* out) {
  return guarded([&] {
    if (c->block_size == 0 || c->unused_lsb_count >= 16) return kUnsupportedConfig;
    auto enc = ricepp::create_encoder<uint16_t>(to_config(c));
    *out = enc->worst_case_encoded_bytes(n);
    return kOk;
  });
}

// The encoder writes through an unchecked iterator into a buffer of its own worst-case size, which is computed
// from floor(n / component_stream_count): the span overload is given a buffer with room for the odd pixel too.
int ref_ricepp_encode(ref_config const* c, uint16_t const* in, size_t n, uint8_t* out, size_t out_cap,
                      size_t* out_len) {
  return guarded([&] {
    if (int st = check_defined(c, n)) return st;
    auto enc = ricepp::create_encoder<uint16_t>(to_config(c));
    std::vector<uint8_t> buf(enc->worst_case_encoded_bytes(n) + 64);
    auto written = enc->encode(std::span<uint8_t>{buf}, std::span<uint16_t const>{in, n});
    if (written.size() > out_cap) return kOutputTooSmall;
    std::memcpy(out, written.data(), written.size());
    *out_len = written.size();
    return kOk;
  });
}

int ref_ricepp_decode(ref_config const* c, uint8_t const* in, size_t in_len, uint16_t* out, size_t n) {
  return guarded([&] {
    if (c->block_size == 0 || c->unused_lsb_count >= 16) return kUnsupportedConfig;
    auto dec = ricepp::create_decoder<uint16_t>(to_config(c));
    dec->decode(std::span<uint16_t>{out, n}, std::span<uint8_t const>{in, in_len});
    return kOk;
  });
}

// One update per entry of `sizes` (consecutive pieces of `data`), then finalize; the 256 bits as 32 bytes,
// bit i at byte i / 8, bit i % 8.
int ref_nilsimsa(uint8_t const* data, size_t const* sizes, size_t nsizes, uint8_t* digest32) {
  return guarded([&] {
    dwarfs::writer::internal::nilsimsa h;
    for (size_t i = 0; i < nsizes; ++i) {
      h.update(data, sizes[i]);
      data += sizes[i];
    }
    dwarfs::writer::internal::nilsimsa::hash_type hash;
    h.finalize(hash);
    for (size_t i = 0; i < 32; ++i) digest32[i] = static_cast<uint8_t>(hash[i / 8] >> (8 * (i % 8)));
    return kOk;
  });
}

int ref_similarity(uint8_t const* data, size_t const* sizes, size_t nsizes, uint32_t* value) {
  return guarded([&] {
    dwarfs::writer::internal::similarity h;
    for (size_t i = 0; i < nsizes; ++i) {
      h.update(data, sizes[i]);
      data += sizes[i];
    }
    *value = h.finalize();
    return kOk;
  });
}

// rsync_hash as the segmenter drives it: update(in) over the first window, then update(out, in) once per byte;
// the value after the fill and after every `granularity` further bytes is reported.
int ref_rsync_hashes(uint8_t const* data, size_t nbytes, size_t window_bytes, size_t granularity, uint32_t* out,
                     size_t out_cap, size_t* count) {
  return guarded([&] {
    if (window_bytes == 0 || granularity == 0) return kInvalidArgument;
    *count = 0;
    if (nbytes < window_bytes) return kOk;
    dwarfs::writer::internal::rsync_hash h;
    size_t k = 0;
    for (size_t i = 0; i < window_bytes; ++i) h.update(data[i]);
    if (k >= out_cap) return kOutputTooSmall;
    out[k++] = h();
    for (size_t i = window_bytes; i < nbytes; ++i) {
      h.update(data[i - window_bytes], data[i]);
      if ((i + 1 - window_bytes) % granularity == 0) {
        if (k >= out_cap) return kOutputTooSmall;
        out[k++] = h();
      }
    }
    *count = k;
    return kOk;
  });
}

uint32_t ref_rsync_repeating_window(uint8_t byte, size_t length) {
  return dwarfs::writer::internal::rsync_hash::repeating_window(byte, length);
}

} // extern "C"
