// digest_common.h -- the round functions and message drivers of the named
// digests (the rpp_digest_* group of include/ricepp_amd.h), shared by the host
// definition (digest_host.cpp) and the kernels (digest_kernels.hip) so that the
// two cannot drift apart.  Plain C++: no inline assembly, and every shift and
// rotate has a compile-time constant amount.
//
// Five compression functions: the MD5 rounds (RFC 1321), the SHA-1 rounds and
// the SHA-256 and SHA-512 rounds (FIPS 180-4), Keccak-f[1600] (FIPS 202) and
// the BLAKE2 rounds in both word sizes (RFC 7693).  One message is one serial
// chain; its schedule (16 words, or the 25 lanes of the Keccak state) is a
// local array whose every index is a compile-time constant, so that on the
// device it lives in registers.  Tables that a rolled loop indexes (the SHA-2
// round constants, Keccak's) are in constant memory on the device.
#ifndef RPP_DIGEST_COMMON_H
#define RPP_DIGEST_COMMON_H

#include <stdint.h>

#include <utility>

#include "ricepp_amd.h"

#if defined(__HIPCC__)
#define RPP_DIGEST_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RPP_DIGEST_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define RPP_DIGEST_TABLE static __device__ __constant__ const
#else
#define RPP_DIGEST_TABLE static constexpr
#endif

namespace rpp_digest {

// ---- names and sizes (rpp_digest_algo's table: OpenSSL's names in lower case, and the two DwarFS names) ----

struct AlgoInfo {
  const char* name;
  int bytes;
};
constexpr AlgoInfo kAlgos[RPP_DIGEST_COUNT] = {
    {"md5", 16},        {"sha1", 20},       {"sha224", 28},     {"sha256", 32},   {"sha384", 48},     {"sha512", 64},
    {"sha512-224", 28}, {"sha3-224", 28},   {"sha3-256", 32},   {"sha3-384", 48}, {"sha3-512", 64},   {"blake2b512", 64},
    {"blake2s256", 32}, {"xxh3-64", 8},     {"xxh3-128", 16},   {"sha512-256", 32}};

// ---- compile-time loops: f(std::integral_constant<int, 0>) ... f(<N - 1>) ----

template <class F, int... I>
RPP_DIGEST_HD void for_each_index(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
RPP_DIGEST_HD void static_for(F&& f) {
  for_each_index(std::make_integer_sequence<int, N>{}, f);
}

template <int N>
RPP_DIGEST_HD uint32_t rotl32(uint32_t x) {
  return (x << N) | (x >> (32 - N));
}
template <int N>
RPP_DIGEST_HD uint32_t rotr32(uint32_t x) {
  return (x >> N) | (x << (32 - N));
}
template <int N>
RPP_DIGEST_HD uint64_t rotr64(uint64_t x) {
  return (x >> N) | (x << (64 - N));
}
template <int N>
RPP_DIGEST_HD uint64_t rotl64(uint64_t x) {
  if constexpr (N == 0) return x;
  else return (x << N) | (x >> (64 - N));
}
template <int N>
RPP_DIGEST_HD uint32_t rotr_w(uint32_t x) {
  return rotr32<N>(x);
}
template <int N>
RPP_DIGEST_HD uint64_t rotr_w(uint64_t x) {
  return rotr64<N>(x);
}

// ---- loads ----

RPP_DIGEST_HD uint32_t bswap(uint32_t v) { return __builtin_bswap32(v); }
RPP_DIGEST_HD uint64_t bswap(uint64_t v) { return __builtin_bswap64(v); }

struct u64pair {
  uint64_t a, b;
};
// 16 bytes at a 16-byte boundary / 8 bytes at an 8-byte boundary
RPP_DIGEST_HD u64pair ld128(const uint8_t* p) {
  u64pair v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
  return v;
}
RPP_DIGEST_HD uint64_t ld64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
  return v;
}
RPP_DIGEST_HD bool aligned_to(const uint8_t* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// a whole 16-word block at a 16-byte boundary, by 16-byte loads
template <bool BigEndian>
RPP_DIGEST_HD void load_block(const uint8_t* p, uint32_t (&w)[16]) {
  static_for<4>([&](auto i) {
    const u64pair v = ld128(p + 16 * i);
    w[4 * i] = (uint32_t)v.a;
    w[4 * i + 1] = (uint32_t)(v.a >> 32);
    w[4 * i + 2] = (uint32_t)v.b;
    w[4 * i + 3] = (uint32_t)(v.b >> 32);
  });
  if constexpr (BigEndian) static_for<16>([&](auto i) { w[i] = bswap(w[i]); });
}
template <bool BigEndian>
RPP_DIGEST_HD void load_block(const uint8_t* p, uint64_t (&w)[16]) {
  static_for<8>([&](auto i) {
    const u64pair v = ld128(p + 16 * i);
    w[2 * i] = BigEndian ? bswap(v.a) : v.a;
    w[2 * i + 1] = BigEndian ? bswap(v.b) : v.b;
  });
}

// Word of the padded message at byte `pos`: the message's bytes, `pad` at byte len, zeros behind it.  Read byte
// by byte: the path of the padded tail and of a payload that is not on a 16-byte boundary.
template <class W, bool BigEndian>
RPP_DIGEST_HD W padded_word(const uint8_t* p, uint64_t len, uint64_t pos, uint32_t pad) {
  W w = 0;
  static_for<(int)sizeof(W)>([&](auto k) {
    const uint64_t at = pos + k;
    const W byte = at < len ? p[at] : (at == len ? pad : 0u);
    if constexpr (BigEndian) w = (W)(w << 8) | byte;
    else w |= byte << (8 * k);
  });
  return w;
}

RPP_DIGEST_HD void put32(uint8_t* out, uint32_t v) { __builtin_memcpy(out, &v, 4); }

// the first `units` 32-bit units of a digest of at most MaxUnits, unit j = f(j) as its little-endian bytes
template <int MaxUnits, class F>
RPP_DIGEST_HD void emit_units(uint8_t* out, uint32_t units, F&& f) {
  static_for<MaxUnits>([&](auto j) {
    if ((uint32_t)j < units) put32(out + 4 * j, f(j));
  });
}

template <class W>
RPP_DIGEST_HD void set8(W (&st)[8], W a, W b, W c, W d, W e, W f, W g, W h) {
  st[0] = a, st[1] = b, st[2] = c, st[3] = d, st[4] = e, st[5] = f, st[6] = g, st[7] = h;
}

// ---- MD5 (RFC 1321): little-endian words, 64-bit little-endian bit length ----

constexpr uint32_t kMd5K[64] = {
    0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
    0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
    0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
    0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
    0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
    0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
    0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
    0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
constexpr int kMd5S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};

struct Md5 {
  using word = uint32_t;
  static constexpr bool kBigEndian = false;
  static constexpr int kLenBytes = 8, kStateWords = 4, kMaxUnits = 4;

  static RPP_DIGEST_HD void init(word (&st)[8], int) {
    set8<word>(st, 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0, 0, 0, 0);
  }
  static RPP_DIGEST_HD void set_length(word (&w)[16], uint64_t len) {
    w[14] = (uint32_t)(len << 3);
    w[15] = (uint32_t)(len >> 29);
  }
  static RPP_DIGEST_HD void compress(word (&st)[8], word (&w)[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    static_for<64>([&](auto ic) {
      constexpr int i = ic;
      constexpr uint32_t k = kMd5K[i];
      constexpr int s = kMd5S[4 * (i / 16) + i % 4];
      constexpr int g = i < 16 ? i : i < 32 ? (5 * i + 1) % 16 : i < 48 ? (3 * i + 5) % 16 : (7 * i) % 16;
      uint32_t f;
      if constexpr (i < 16) f = (b & c) | (~b & d);
      else if constexpr (i < 32) f = (d & b) | (~d & c);
      else if constexpr (i < 48) f = b ^ c ^ d;
      else f = c ^ (b | ~d);
      f += a + k + w[g];
      a = d;
      d = c;
      c = b;
      b += rotl32<s>(f);
    });
    st[0] += a, st[1] += b, st[2] += c, st[3] += d;
  }
  template <int J>
  static RPP_DIGEST_HD uint32_t unit(const word (&st)[8], std::integral_constant<int, J>) {
    return st[J];
  }
};

// ---- SHA-1 (FIPS 180-4 section 6.1): big-endian words, 64-bit big-endian bit length ----

struct Sha1 {
  using word = uint32_t;
  static constexpr bool kBigEndian = true;
  static constexpr int kLenBytes = 8, kStateWords = 5, kMaxUnits = 5;

  static RPP_DIGEST_HD void init(word (&st)[8], int) {
    set8<word>(st, 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u, 0, 0, 0);
  }
  static RPP_DIGEST_HD void set_length(word (&w)[16], uint64_t len) {
    w[14] = (uint32_t)(len >> 29);
    w[15] = (uint32_t)(len << 3);
  }
  static RPP_DIGEST_HD void compress(word (&st)[8], word (&w)[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
    static_for<80>([&](auto tc) {
      constexpr int t = tc;
      if constexpr (t >= 16)
        w[t & 15] = rotl32<1>(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15]);
      uint32_t f;
      if constexpr (t < 20) f = ((b & c) | (~b & d)) + 0x5a827999u;
      else if constexpr (t < 40) f = (b ^ c ^ d) + 0x6ed9eba1u;
      else if constexpr (t < 60) f = ((b & c) | (b & d) | (c & d)) + 0x8f1bbcdcu;
      else f = (b ^ c ^ d) + 0xca62c1d6u;
      const uint32_t tmp = rotl32<5>(a) + f + e + w[t & 15];
      e = d;
      d = c;
      c = rotl32<30>(b);
      b = a;
      a = tmp;
    });
    st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e;
  }
  template <int J>
  static RPP_DIGEST_HD uint32_t unit(const word (&st)[8], std::integral_constant<int, J>) {
    return bswap(st[J]);
  }
};

// ---- SHA-224 / SHA-256 (FIPS 180-4 sections 5.3.2, 5.3.3, 6.2) ----

RPP_DIGEST_TABLE uint32_t kSha256K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

struct Sha256 {
  using word = uint32_t;
  static constexpr bool kBigEndian = true;
  static constexpr int kLenBytes = 8, kStateWords = 8, kMaxUnits = 8;

  static RPP_DIGEST_HD void init(word (&st)[8], int algo) {
    if (algo == RPP_DIGEST_SHA224)
      set8<word>(st, 0xc1059ed8u, 0x367cd507u, 0x3070dd17u, 0xf70e5939u, 0xffc00b31u, 0x68581511u, 0x64f98fa7u,
                 0xbefa4fa4u);
    else
      set8<word>(st, 0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu,
                 0x5be0cd19u);
  }
  static RPP_DIGEST_HD void set_length(word (&w)[16], uint64_t len) { Sha1::set_length(w, len); }

  template <int I>
  static RPP_DIGEST_HD void round(uint32_t (&s)[8], uint32_t k, uint32_t wi) {
    // (the working variables rotate through s by index instead of moving)
    uint32_t &a = s[(0 - I) & 7], &b = s[(1 - I) & 7], &c = s[(2 - I) & 7], &d = s[(3 - I) & 7], &e = s[(4 - I) & 7],
             &f = s[(5 - I) & 7], &g = s[(6 - I) & 7], &h = s[(7 - I) & 7];
    const uint32_t t1 = h + (rotr32<6>(e) ^ rotr32<11>(e) ^ rotr32<25>(e)) + ((e & f) ^ (~e & g)) + k + wi;
    const uint32_t t2 = (rotr32<2>(a) ^ rotr32<13>(a) ^ rotr32<22>(a)) + ((a & b) ^ (a & c) ^ (b & c));
    d += t1;
    h = t1 + t2;
  }
  static RPP_DIGEST_HD void compress(word (&st)[8], word (&w)[16]) {
    uint32_t s[8];
    static_for<8>([&](auto i) { s[i] = st[i]; });
    static_for<16>([&](auto i) { round<i>(s, kSha256K[i], w[i]); });
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 16; t < 64; t += 16) {
      static_for<16>([&](auto ic) {
        constexpr int i = ic;
        const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
        w[i] += (rotr32<7>(w15) ^ rotr32<18>(w15) ^ (w15 >> 3)) + w[(i + 9) & 15] +
                (rotr32<17>(w2) ^ rotr32<19>(w2) ^ (w2 >> 10));
        round<i>(s, kSha256K[t + i], w[i]);
      });
    }
    static_for<8>([&](auto i) { st[i] += s[i]; });
  }
  template <int J>
  static RPP_DIGEST_HD uint32_t unit(const word (&st)[8], std::integral_constant<int, J>) {
    return bswap(st[J]);
  }
};

// ---- SHA-384 / SHA-512 / SHA-512/224 / SHA-512/256 (FIPS 180-4 sections 5.3.4-5.3.6, 6.4): 128-bit bit length ----

RPP_DIGEST_TABLE uint64_t kSha512K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

struct Sha512 {
  using word = uint64_t;
  static constexpr bool kBigEndian = true;
  static constexpr int kLenBytes = 16, kStateWords = 8, kMaxUnits = 16;

  static RPP_DIGEST_HD void init(word (&st)[8], int algo) {
    switch (algo) {
      case RPP_DIGEST_SHA384:
        set8<word>(st, 0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull, 0x152fecd8f70e5939ull,
                   0x67332667ffc00b31ull, 0x8eb44a8768581511ull, 0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull);
        break;
      case RPP_DIGEST_SHA512_224:
        set8<word>(st, 0x8c3d37c819544da2ull, 0x73e1996689dcd4d6ull, 0x1dfab7ae32ff9c82ull, 0x679dd514582f9fcfull,
                   0x0f6d2b697bd44da8ull, 0x77e36f7304c48942ull, 0x3f9d85a86a1d36c8ull, 0x1112e6ad91d692a1ull);
        break;
      case RPP_DIGEST_SHA512_256:
        set8<word>(st, 0x22312194fc2bf72cull, 0x9f555fa3c84c64c2ull, 0x2393b86b6f53b151ull, 0x963877195940eabdull,
                   0x96283ee2a88effe3ull, 0xbe5e1e2553863992ull, 0x2b0199fc2c85b8aaull, 0x0eb72ddc81c52ca2ull);
        break;
      default:
        set8<word>(st, 0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                   0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull);
    }
  }
  static RPP_DIGEST_HD void set_length(word (&w)[16], uint64_t len) {
    w[14] = len >> 61;
    w[15] = len << 3;
  }
  template <int I>
  static RPP_DIGEST_HD void round(uint64_t (&s)[8], uint64_t k, uint64_t wi) {
    uint64_t &a = s[(0 - I) & 7], &b = s[(1 - I) & 7], &c = s[(2 - I) & 7], &d = s[(3 - I) & 7], &e = s[(4 - I) & 7],
             &f = s[(5 - I) & 7], &g = s[(6 - I) & 7], &h = s[(7 - I) & 7];
    const uint64_t t1 = h + (rotr64<14>(e) ^ rotr64<18>(e) ^ rotr64<41>(e)) + ((e & f) ^ (~e & g)) + k + wi;
    const uint64_t t2 = (rotr64<28>(a) ^ rotr64<34>(a) ^ rotr64<39>(a)) + ((a & b) ^ (a & c) ^ (b & c));
    d += t1;
    h = t1 + t2;
  }
  static RPP_DIGEST_HD void compress(word (&st)[8], word (&w)[16]) {
    uint64_t s[8];
    static_for<8>([&](auto i) { s[i] = st[i]; });
    static_for<16>([&](auto i) { round<i>(s, kSha512K[i], w[i]); });
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 16; t < 80; t += 16) {
      static_for<16>([&](auto ic) {
        constexpr int i = ic;
        const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
        w[i] += (rotr64<1>(w15) ^ rotr64<8>(w15) ^ (w15 >> 7)) + w[(i + 9) & 15] +
                (rotr64<19>(w2) ^ rotr64<61>(w2) ^ (w2 >> 6));
        round<i>(s, kSha512K[t + i], w[i]);
      });
    }
    static_for<8>([&](auto i) { st[i] += s[i]; });
  }
  // (unit 2i is the high half of word i: SHA-512/224 ends inside word 3)
  template <int J>
  static RPP_DIGEST_HD uint32_t unit(const word (&st)[8], std::integral_constant<int, J>) {
    return bswap((uint32_t)(J & 1 ? st[J / 2] : st[J / 2] >> 32));
  }
};

// One message through a Merkle-Damgard hash H: the blocks of the message, then 0x80, zeros up to the length
// field, and the bit length (messages are below 2^61 bytes).
template <class H>
RPP_DIGEST_HD void md_digest(const uint8_t* p, uint64_t len, int algo, uint32_t units, uint8_t* out) {
  using W = typename H::word;
  constexpr uint64_t kBlock = 16 * sizeof(W);
  W st[8], w[16];
  H::init(st, algo);
  const uint64_t nblocks = (len + 1 + H::kLenBytes + kBlock - 1) / kBlock;
  for (uint64_t blk = 0; blk < nblocks; ++blk) {
    const uint64_t pos = blk * kBlock;
    if (pos + kBlock <= len && aligned_to(p + pos, 16)) {
      load_block<H::kBigEndian>(p + pos, w);
    } else {
      static_for<16>([&](auto i) { w[i] = padded_word<W, H::kBigEndian>(p, len, pos + sizeof(W) * i, 0x80u); });
      if (blk + 1 == nblocks) H::set_length(w, len);
    }
    H::compress(st, w);
  }
  emit_units<H::kMaxUnits>(out, units, [&](auto j) { return H::unit(st, j); });
}

// ---- SHA-3 (FIPS 202): Keccak-f[1600], pad10*1 behind the domain bits 01: 0x06 ... 0x80 ----

RPP_DIGEST_TABLE uint64_t kKeccakRc[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
    0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
// rho's rotation of lane x + 5y
constexpr int kKeccakRho[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};

// lanes a[x + 5y]
RPP_DIGEST_HD void keccak_f1600(uint64_t (&a)[25]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int r = 0; r < 24; ++r) {
    uint64_t c[5], b[25];
    static_for<5>([&](auto x) { c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20]; });
    static_for<25>([&](auto ic) {
      constexpr int i = ic, x = i % 5, y = i / 5;
      const uint64_t v = a[i] ^ c[(x + 4) % 5] ^ rotl64<1>(c[(x + 1) % 5]);  // theta
      b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64<kKeccakRho[i]>(v);           // rho, pi
    });
    static_for<25>([&](auto ic) {
      constexpr int i = ic, x = i % 5, y = i / 5;
      a[i] = b[i] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);  // chi
    });
    a[0] ^= kKeccakRc[r];  // iota
  }
}

// `NW` 64-bit words at an 8-byte boundary: 16-byte loads from the first 16-byte boundary on
template <int NW>
RPP_DIGEST_HD void load_rate(const uint8_t* p, uint64_t (&w)[NW]) {
  auto pairs = [&](auto first) {
    constexpr int f = first;
    if constexpr (f) w[0] = ld64(p);
    static_for<(NW - f) / 2>([&](auto i) {
      const u64pair v = ld128(p + 8 * f + 16 * i);
      w[f + 2 * i] = v.a;
      w[f + 2 * i + 1] = v.b;
    });
    if constexpr ((NW - f) % 2) w[NW - 1] = ld64(p + 8 * (NW - 1));
  };
  if (aligned_to(p, 16)) pairs(std::integral_constant<int, 0>{});
  else pairs(std::integral_constant<int, 1>{});
}

template <int Rate>
RPP_DIGEST_HD void keccak_digest(const uint8_t* p, uint64_t len, uint32_t units, uint8_t* out) {
  constexpr int NW = Rate / 8;
  uint64_t a[25], w[NW];
  static_for<25>([&](auto i) { a[i] = 0; });
  for (uint64_t pos = 0;; pos += Rate) {
    const bool last = len - pos < Rate;  // (pos <= len: the block that holds the padding)
    if (!last && aligned_to(p + pos, 8)) {
      load_rate<NW>(p + pos, w);
    } else {
      static_for<NW>([&](auto i) { w[i] = padded_word<uint64_t, false>(p, len, pos + 8 * i, 0x06u); });
      if (last) w[NW - 1] ^= 0x80ull << 56;
    }
    static_for<NW>([&](auto i) { a[i] ^= w[i]; });
    keccak_f1600(a);
    if (last) break;
  }
  emit_units<16>(out, units, [&](auto j) { return (uint32_t)(a[j / 2] >> (32 * (j & 1))); });
}

// ---- BLAKE2b-512 / BLAKE2s-256 (RFC 7693), unkeyed, default parameters ----

constexpr int kBlake2Sigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

template <class W>
struct Blake2;
template <>
struct Blake2<uint64_t> {
  static constexpr int kRounds = 12, kR1 = 32, kR2 = 24, kR3 = 16, kR4 = 63, kMaxUnits = 16;
  static constexpr uint64_t kParam = 0x01010000u ^ 64u;  // digest 64 bytes, no key, fanout 1, depth 1
  static constexpr uint64_t kIv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                      0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                      0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
};
template <>
struct Blake2<uint32_t> {
  static constexpr int kRounds = 10, kR1 = 16, kR2 = 12, kR3 = 8, kR4 = 7, kMaxUnits = 8;
  static constexpr uint32_t kParam = 0x01010000u ^ 32u;
  static constexpr uint32_t kIv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                      0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

// `t` = the message bytes up to and including this block
template <class W>
RPP_DIGEST_HD void blake2_compress(W (&h)[8], const W (&m)[16], uint64_t t, bool last) {
  using B = Blake2<W>;
  W v[16];
  static_for<8>([&](auto ic) {
    constexpr int i = ic;
    constexpr W iv = B::kIv[i];
    v[i] = h[i];
    v[i + 8] = iv;
  });
  v[12] ^= (W)t;
  if constexpr (sizeof(W) == 4) v[13] ^= (W)(t >> 32);
  if (last) v[14] = ~v[14];
  static_for<B::kRounds>([&](auto rc) {
    constexpr int r = rc % 10;
    static_for<8>([&](auto gc) {
      constexpr int g = gc;
      // columns, then diagonals
      constexpr int ia = g % 4, ib = 4 + (g < 4 ? g : (g + 1) % 4), ic = 8 + (g < 4 ? g : (g + 2) % 4),
                    id = 12 + (g < 4 ? g : (g + 3) % 4);
      constexpr int sx = kBlake2Sigma[r][2 * g], sy = kBlake2Sigma[r][2 * g + 1];
      W &a = v[ia], &b = v[ib], &c = v[ic], &d = v[id];
      a += b + m[sx];
      d = rotr_w<B::kR1>((W)(d ^ a));
      c += d;
      b = rotr_w<B::kR2>((W)(b ^ c));
      a += b + m[sy];
      d = rotr_w<B::kR3>((W)(d ^ a));
      c += d;
      b = rotr_w<B::kR4>((W)(b ^ c));
    });
  });
  static_for<8>([&](auto i) { h[i] ^= v[i] ^ v[i + 8]; });
}

// The last block, zero-padded, is the final one; a message that ends on a block boundary has no empty block
// behind it, and the empty message is one block of zeros.
template <class W>
RPP_DIGEST_HD void blake2_digest(const uint8_t* p, uint64_t len, uint32_t units, uint8_t* out) {
  using B = Blake2<W>;
  constexpr uint64_t kBlock = 16 * sizeof(W);
  W h[8], m[16];
  static_for<8>([&](auto ic) {
    constexpr int i = ic;
    constexpr W iv = B::kIv[i];
    h[i] = iv;
  });
  h[0] ^= B::kParam;
  const uint64_t nblocks = len ? (len + kBlock - 1) / kBlock : 1;
  for (uint64_t blk = 0; blk < nblocks; ++blk) {
    const uint64_t pos = blk * kBlock;
    const bool last = blk + 1 == nblocks;
    if (pos + kBlock <= len && aligned_to(p + pos, 16)) {
      load_block<false>(p + pos, m);
    } else {
      static_for<16>([&](auto i) { m[i] = padded_word<W, false>(p, len, pos + sizeof(W) * i, 0u); });
    }
    blake2_compress<W>(h, m, last ? len : pos + kBlock, last);
  }
  emit_units<B::kMaxUnits>(out, units, [&](auto jc) {
    constexpr int j = jc;
    if constexpr (sizeof(W) == 8) return (uint32_t)(h[j / 2] >> (32 * (j & 1)));
    else return (uint32_t)h[j];
  });
}

}  // namespace rpp_digest

#endif  // RPP_DIGEST_COMMON_H
