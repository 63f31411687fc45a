// digest_host.cpp -- the names and sizes of the digests, and their definition
// on host memory, built on the round functions of digest_common.h that the
// kernels of digest_kernels.hip run as well.  Plain C++: the sanitizer test
// (tests/cpp/digest_test.cpp) compiles this file alone.
//
// Padding rules (a message of `len` bytes, below 2^61).
//   MD5             RFC 1321.  64-byte blocks of little-endian 32-bit words.  Byte 0x80, zeros up to 56 mod 64, the
//                   bit length as 8 little-endian bytes: (len + 9 + 63) / 64 blocks, so a message with len % 64 in
//                   56..63 takes one block more.  Digest: the four state words, little endian.
//   SHA-1, SHA-224, SHA-256
//                   FIPS 180-4.  The same layout with big-endian words and a big-endian bit length.  Digest: the
//                   state words big endian; SHA-224 is the first seven words of SHA-256 run from its own IV.
//   SHA-384, SHA-512, SHA-512/224, SHA-512/256
//                   128-byte blocks of big-endian 64-bit words.  Byte 0x80, zeros up to 112 mod 128, the bit length
//                   as 16 big-endian bytes: (len + 17 + 127) / 128 blocks, one more for len % 128 in 112..127.
//                   Each has its own IV (FIPS 180-4 sections 5.3.4-5.3.6); the digest is the first 48, 64, 28 or 32
//                   bytes of the big-endian state (SHA-512/224 ends in the middle of the fourth word).
//   SHA3-224/256/384/512
//                   FIPS 202.  Rate r = 144, 136, 104, 72 bytes, absorbed as little-endian lanes.  Byte 0x06 (the
//                   domain bits 01 and the first pad bit) at len, 0x80 into the last byte of that block -- one byte
//                   0x86 where len % r == r - 1 -- so len / r + 1 blocks: a message that ends on a rate boundary
//                   takes a whole block of padding.  Digest: the first bytes of the state, little-endian lanes.
//   BLAKE2b-512, BLAKE2s-256
//                   RFC 7693, unkeyed, default parameters (h[0] ^= 0x01010000 ^ digest bytes).  128- / 64-byte
//                   blocks of little-endian words; the last block is padded with zeros and compressed with the
//                   final flag and the counter t = len, every other block with t = the bytes so far.
//                   max(1, ceil(len / block)) blocks: a message that ends on a block boundary has no empty block
//                   behind it, and the empty message is one block of zeros with t = 0.  Digest: h, little endian.
#include <string.h>

#include "digest_common.h"

namespace {

using namespace rpp_digest;

char lower(char c) { return c >= 'A' && c <= 'Z' ? (char)(c - 'A' + 'a') : c; }

bool same_name(const char* a, const char* b, bool any_case) {
  for (;; ++a, ++b) {
    if (any_case ? lower(*a) != lower(*b) : *a != *b) return false;
    if (!*a) return true;
  }
}

// false: `algo` has no definition here (the two XXH3 hashes, or no algorithm)
bool digest_one(int algo, const uint8_t* p, uint64_t len, uint8_t* out) {
  if (algo < 0 || algo >= RPP_DIGEST_COUNT) return false;
  const uint32_t units = (uint32_t)kAlgos[algo].bytes / 4;
  switch (algo) {
    case RPP_DIGEST_MD5: md_digest<Md5>(p, len, algo, units, out); return true;
    case RPP_DIGEST_SHA1: md_digest<Sha1>(p, len, algo, units, out); return true;
    case RPP_DIGEST_SHA224:
    case RPP_DIGEST_SHA256: md_digest<Sha256>(p, len, algo, units, out); return true;
    case RPP_DIGEST_SHA384:
    case RPP_DIGEST_SHA512:
    case RPP_DIGEST_SHA512_224:
    case RPP_DIGEST_SHA512_256: md_digest<Sha512>(p, len, algo, units, out); return true;
    case RPP_DIGEST_SHA3_224: keccak_digest<144>(p, len, units, out); return true;
    case RPP_DIGEST_SHA3_256: keccak_digest<136>(p, len, units, out); return true;
    case RPP_DIGEST_SHA3_384: keccak_digest<104>(p, len, units, out); return true;
    case RPP_DIGEST_SHA3_512: keccak_digest<72>(p, len, units, out); return true;
    case RPP_DIGEST_BLAKE2B512: blake2_digest<uint64_t>(p, len, units, out); return true;
    case RPP_DIGEST_BLAKE2S256: blake2_digest<uint32_t>(p, len, units, out); return true;
  }
  return false;
}

}  // namespace

extern "C" int rpp_digest_algo(const char* name) {
  if (!name) return -1;
  for (int a = 0; a < RPP_DIGEST_COUNT; ++a) {
    const bool exact = a == RPP_DIGEST_XXH3_64 || a == RPP_DIGEST_XXH3_128;
    if (same_name(name, kAlgos[a].name, !exact)) return a;
  }
  return -1;
}

extern "C" int rpp_digest_bytes(int algo) { return algo >= 0 && algo < RPP_DIGEST_COUNT ? kAlgos[algo].bytes : 0; }

extern "C" int rpp_digest_host(int algo, const uint8_t* data, const uint64_t* offsets, const uint64_t* sizes,
                               const uint8_t* select, uint32_t n, uint8_t* digest) {
  const int nbytes = rpp_digest_bytes(algo);
  if (nbytes == 0 || algo == RPP_DIGEST_XXH3_64 || algo == RPP_DIGEST_XXH3_128) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!data || !offsets || !sizes || !digest) return RPP_INVALID_ARGUMENT;
  for (uint32_t b = 0; b < n; ++b) {
    if (select && !select[b]) continue;
    if (!digest_one(algo, data + offsets[b], sizes[b], digest + (size_t)nbytes * b)) return RPP_INVALID_ARGUMENT;
  }
  return RPP_OK;
}
