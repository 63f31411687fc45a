// section_kernels.hip -- DwarFS section headers on MI355X: XXH3-64 and
// SHA-512/256 over batches of messages, the 64-byte section_header_v2
// (include/dwarfs/fstypes.h:85-97), byte-packed section assembly and the
// reader's integrity checks (the rpp_xxh3_64_batch ... rpp_sections_verify_batch
// group of include/ricepp_amd.h).
//
// The writer computes both checksums per block on its own thread
// (fsblock::build_section_header, src/writer/filesystem_writer.cpp:606-651):
// XXH3-64 over header[48,64) + payload, then SHA-512/256 over header[40,64) +
// payload.  The reader checks the XXH3 before it decompresses a block
// (cached_block, src/reader/internal/cached_block.cpp:58-67 ->
// fs_section_v2::check_fast, src/internal/fs_section.cpp:226-259).
//
// A message is up to three spans read as one byte string: two short leading
// spans (header fields, <= 64 bytes; the DwarFS frame header, <= 32 bytes) and
// a payload of any size and alignment.  Only the first 96 bytes of a message can
// lie in the leading spans, so they are read byte by byte and everything else
// by 16-byte loads from the payload.
//
//   XXH3 long (> 240 bytes)   one wave per message, 1 KiB (16 stripes) per step:
//       lane l loads the 16 bytes at 16*l of the block = accumulators 2(l%4),
//       2(l%4)+1 of stripe l/4, with the secret at 8*(l/4) + 16*(l%4); the
//       acc[j^1] += data swap stays in the lane; the 16 lanes sharing l%4 are
//       summed by a butterfly (stripe contributions add modulo 2^64), then the
//       scramble; the next block's load is issued before the reduction.
//   XXH3 short (<= 240)       one lane per message.
//   SHA-512/256               one lane per message (the chain does not split),
//       128-byte blocks by 16-byte loads, big-endian words by byte permutes.
//   Lane-per-message kernels give every message its own wave while the batch
//   is small (message i -> wave i % W, lane i / W), so few messages run on many
//   SIMDs instead of in the lanes of one.
//
// The same kernels hash files for the scanner's duplicate detection
// (file_scanner_::scan_dedupe, src/writer/internal/file_scanner.cpp:274-413;
// the rpp_file_hash_batch ... rpp_file_dedup_batch group): XXH3-128 shares the
// long loop and has short formulas of its own, a select mask skips messages,
// and two small kernels group equal (size, digest) keys in a hash table.
//
// Every shift and rotate has a compile-time constant amount.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ricepp_amd.h"

namespace {

constexpr uint64_t P32_1 = 0x9E3779B1ull, P32_2 = 0x85EBCA77ull, P32_3 = 0xC2B2AE3Dull;
constexpr uint64_t P64_1 = 0x9E3779B185EBCA87ull, P64_2 = 0xC2B2AE3D27D4EB4Full, P64_3 = 0x165667B19E3779F9ull,
                   P64_4 = 0x85EBCA77C2B2AE63ull, P64_5 = 0x27D4EB2F165667C5ull;
constexpr uint64_t MX1 = 0x165667919E3779F9ull, MX2 = 0x9FB21C651E98DF25ull;

// XXH3's default secret (kSecret of xxhash.h), 192 bytes
constexpr char kSecretHex[] =
    "b8fe6c3923a44bbe7c01812cf721ad1cded46de9839097db7240a4a4b7b3671fcb79e64eccc0e578825ad07dccff7221"
    "b8084674f743248ee03590e6813a264c3c2852bb91c300cb88d0658b1b532ea371644897a20df94e3819ef46a9deacd8"
    "a8fa763fe39c343ff9dcbbc7c70b4f1d8a51e04bcdb45931c89f7ec9d9787364eac5ac8334d3ebc3c581a0fffa1363eb"
    "170ddd51b7f0da49d316552629d4689e2b16be587d47a1fc8ff8b8d17ad031ce45cb3a8f95160428afd7fbcabb4b407e";
static_assert(sizeof(kSecretHex) == 2 * 192 + 1, "the default secret has 192 bytes");

struct Secret {
  uint8_t b[192];
};
constexpr uint8_t hex_digit(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
constexpr Secret make_secret() {
  Secret s{};
  for (int i = 0; i < 192; ++i) s.b[i] = (uint8_t)(hex_digit(kSecretHex[2 * i]) * 16 + hex_digit(kSecretHex[2 * i + 1]));
  return s;
}
__device__ __constant__ Secret d_secret = make_secret();

// SHA-512/256 (FIPS 180-4 sections 5.3.6.2, 4.2.3)
__device__ __constant__ uint64_t d_sha_iv[8] = {
    0x22312194fc2bf72cull, 0x9f555fa3c84c64c2ull, 0x2393b86b6f53b151ull, 0x963877195940eabdull,
    0x96283ee2a88effe3ull, 0xbe5e1e2553863992ull, 0x2b0199fc2c85b8aaull, 0x0eb72ddc81c52ca2ull};
__device__ __constant__ uint64_t d_sha_k[80] = {
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

constexpr uint32_t kHeaderBytes = 64;  // sizeof(section_header_v2)
constexpr uint32_t kFrameRow = 32;     // a frame-header row (varint + thrift <= 32 bytes)
constexpr uint32_t kOffSha = 8, kOffXxh = 40, kOffNumber = 48, kOffLength = 56;
constexpr uint32_t kLaneWavesMax = 4096;  // 256 CUs x 4 SIMDs x 4 waves
constexpr uint32_t kLongWaves = 4;        // messages (waves) per workgroup of the long XXH3 kernel
constexpr uint32_t kCopyThreads = 256;

// ---- a batch of messages ----

// How message b of a batch is found, and where its result goes.
//   sections == 0: payload = data + offs[b], sizes[b] bytes; leading spans seg0
//     (row b of seg0_stride bytes, seg0_len[b] or seg0_fixed bytes of it) and
//     seg1 (row b of 32 bytes, seg1_len[b] bytes); the result is written to
//     out + out_stride * b.
//   sections == 1 (verify): the message is image[offs[b] + from, offs[b] + 64 +
//     length) of a section whose status[b] is RPP_OK; the result is compared
//     with the header's stored value and status[b] set on a mismatch.
struct Job {
  const uint8_t* data;
  const uint64_t* offs;
  const uint64_t* sizes;
  const uint8_t* seg0;
  const uint32_t* seg0_len;
  uint32_t seg0_stride, seg0_fixed;
  const uint8_t* seg1;
  const uint32_t* seg1_len;
  uint8_t* out;
  uint32_t out_stride;
  uint32_t sections, from;
  int32_t* status;
  // file hashing: message b is skipped (not read, nothing written) where select[b] == 0 or its size is below
  // min_size; a nonzero clamp hashes the first min(size, clamp) bytes only
  const uint8_t* select;
  uint64_t min_size, clamp;
};

struct Msg {
  const uint8_t *p0, *p1, *pay;
  uint32_t l0, pre;  // bytes in p0; bytes in p0 and p1 together
  uint64_t len;      // the whole message
};

__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
struct u64pair {
  uint64_t a, b;
};
__device__ __forceinline__ u64pair ld128(const uint8_t* p) {
  u64pair v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

__device__ __forceinline__ bool load_msg(const Job& j, uint32_t b, Msg& m) {
  if (j.select && !j.select[b]) return false;
  if (j.sections) {
    if (j.status[b] != RPP_OK) return false;
    const uint8_t* h = j.data + j.offs[b];
    m.p0 = m.p1 = nullptr;
    m.l0 = m.pre = 0;
    m.pay = h + j.from;
    m.len = (kHeaderBytes - j.from) + ld64(h + kOffLength);
    return true;
  }
  uint32_t l0 = 0, l1 = 0;
  if (j.seg0) {
    l0 = j.seg0_len ? j.seg0_len[b] : j.seg0_fixed;
    l0 = l0 < j.seg0_stride ? l0 : j.seg0_stride;
  }
  if (j.seg1) {
    l1 = j.seg1_len[b];
    l1 = l1 < kFrameRow ? l1 : kFrameRow;
  }
  m.p0 = j.seg0 + (size_t)j.seg0_stride * b;
  m.p1 = j.seg1 + (size_t)kFrameRow * b;
  m.l0 = l0;
  m.pre = l0 + l1;
  uint64_t size = j.sizes[b];
  if (size < j.min_size) return false;
  if (j.clamp && size > j.clamp) size = j.clamp;
  m.pay = j.data + j.offs[b];
  m.len = (uint64_t)m.pre + size;
  return true;
}

__device__ __forceinline__ uint32_t msg_byte(const Msg& m, uint64_t pos) {
  if (pos >= m.pre) return m.pay[pos - m.pre];
  const uint32_t p = (uint32_t)pos;
  return p < m.l0 ? m.p0[p] : m.p1[p - m.l0];
}

// little-endian reads of N bytes at `pos` (pos + N <= len)
__device__ __forceinline__ uint64_t msg_r64(const Msg& m, uint64_t pos) {
  if (pos >= m.pre) return ld64(m.pay + (pos - m.pre));
  uint64_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) v |= (uint64_t)msg_byte(m, pos + i) << (8 * i);
  return v;
}
__device__ __forceinline__ uint32_t msg_r32(const Msg& m, uint64_t pos) {
  if (pos >= m.pre) return ld32(m.pay + (pos - m.pre));
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) v |= msg_byte(m, pos + i) << (8 * i);
  return v;
}
__device__ __forceinline__ u64pair msg_r128(const Msg& m, uint64_t pos) {
  if (pos >= m.pre) return ld128(m.pay + (pos - m.pre));
  return u64pair{msg_r64(m, pos), msg_r64(m, pos + 8)};
}

__device__ __forceinline__ uint64_t sec64(uint32_t off) { return ld64(d_secret.b + off); }
__device__ __forceinline__ uint32_t sec32(uint32_t off) { return ld32(d_secret.b + off); }

// lane-per-message kernels: message of (wave w of W, lane l)
__device__ __forceinline__ uint64_t lane_message(uint32_t nwaves) {
  return (uint64_t)threadIdx.x * nwaves + blockIdx.x;
}
uint32_t lane_waves(uint32_t n) {
  const uint32_t full = (n + 63) / 64, spread = n < kLaneWavesMax ? n : kLaneWavesMax;
  return full > spread ? full : spread;
}

// ---- XXH3-64, seed 0, default secret ----

__device__ __forceinline__ uint64_t rotl49_24(uint64_t h) {
  return ((h << 49) | (h >> 15)) ^ ((h << 24) | (h >> 40));
}
__device__ __forceinline__ uint64_t fold64(uint64_t a, uint64_t b) { return (a * b) ^ __umul64hi(a, b); }
__device__ __forceinline__ uint64_t aval(uint64_t h) {
  h ^= h >> 37;
  h *= MX1;
  return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t aval64(uint64_t h) {
  h ^= h >> 33;
  h *= P64_2;
  h ^= h >> 29;
  h *= P64_3;
  return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t rrmxmx(uint64_t h, uint64_t n) {
  h ^= rotl49_24(h);
  h *= MX2;
  h ^= (h >> 35) + n;
  h *= MX2;
  return h ^ (h >> 28);
}
__device__ __forceinline__ uint64_t mix16(const Msg& m, uint64_t pos, uint32_t s) {
  const u64pair d = msg_r128(m, pos);
  return fold64(d.a ^ sec64(s), d.b ^ sec64(s + 8));
}
__device__ __forceinline__ uint64_t mul32x32(uint64_t k) { return (k & 0xFFFFFFFFull) * (k >> 32); }

// len <= 240
__device__ uint64_t xxh3_short(const Msg& m) {
  const uint64_t len = m.len;
  if (len == 0) return aval64(sec64(56) ^ sec64(64));
  if (len <= 3) {
    const uint32_t c1 = msg_byte(m, 0), c2 = msg_byte(m, len >> 1), c3 = msg_byte(m, len - 1);
    const uint32_t comb = (c1 << 16) | (c2 << 24) | c3 | ((uint32_t)len << 8);
    return aval64((uint64_t)comb ^ (uint64_t)(sec32(0) ^ sec32(4)));
  }
  if (len <= 8) {
    const uint64_t hi = msg_r32(m, 0), lo = msg_r32(m, len - 4);
    return rrmxmx((lo + (hi << 32)) ^ (sec64(8) ^ sec64(16)), len);
  }
  if (len <= 16) {
    const uint64_t lo = msg_r64(m, 0) ^ (sec64(24) ^ sec64(32));
    const uint64_t hi = msg_r64(m, len - 8) ^ (sec64(40) ^ sec64(48));
    return aval(len + __builtin_bswap64(lo) + hi + fold64(lo, hi));
  }
  uint64_t acc = len * P64_1;
  if (len <= 128) {
    const uint32_t rounds = (uint32_t)((len - 1) >> 5);
    for (uint32_t i = 0; i <= rounds; ++i)
      acc += mix16(m, 16 * i, 32 * i) + mix16(m, len - 16 * (i + 1), 32 * i + 16);
    return aval(acc);
  }
  for (uint32_t i = 0; i < 8; ++i) acc += mix16(m, 16 * i, 16 * i);
  acc = aval(acc);
  const uint32_t rounds = (uint32_t)(len >> 4);
  for (uint32_t i = 8; i < rounds; ++i) acc += mix16(m, 16 * i, 16 * (i - 8) + 3);
  acc += mix16(m, len - 16, 119);
  return aval(acc);
}

__device__ __forceinline__ void emit_xxh(const Job& j, uint32_t b, uint64_t h) {
  if (j.sections) {
    if (ld64(j.data + j.offs[b] + kOffXxh) != h) j.status[b] = RPP_CHECKSUM_MISMATCH;
  } else {
    __builtin_memcpy(j.out + (size_t)j.out_stride * b, &h, 8);
  }
}

__global__ __launch_bounds__(64) void rpp_xxh3_short_kernel(Job job, uint32_t n, uint32_t nwaves) {
  const uint64_t id = lane_message(nwaves);
  if (id >= n) return;
  const uint32_t b = (uint32_t)id;
  Msg m;
  if (!load_msg(job, b, m) || m.len > 240) return;
  emit_xxh(job, b, xxh3_short(m));
}

// ---- XXH3-128, seed 0, default secret: {low64, high64} ----

__device__ __forceinline__ u64pair mix32(u64pair acc, const Msg& m, uint64_t p1, uint64_t p2, uint32_t s) {
  const u64pair d1 = msg_r128(m, p1), d2 = msg_r128(m, p2);
  acc.a += fold64(d1.a ^ sec64(s), d1.b ^ sec64(s + 8));
  acc.a ^= d2.a + d2.b;
  acc.b += fold64(d2.a ^ sec64(s + 16), d2.b ^ sec64(s + 24));
  acc.b ^= d1.a + d1.b;
  return acc;
}

// len <= 240
__device__ u64pair xxh3_128_short(const Msg& m) {
  const uint64_t len = m.len;
  if (len == 0) return u64pair{aval64(sec64(64) ^ sec64(72)), aval64(sec64(80) ^ sec64(88))};
  if (len <= 3) {
    const uint32_t c1 = msg_byte(m, 0), c2 = msg_byte(m, len >> 1), c3 = msg_byte(m, len - 1);
    const uint32_t lo = (c1 << 16) | (c2 << 24) | c3 | ((uint32_t)len << 8);
    const uint32_t sw = __builtin_bswap32(lo), hi = (sw << 13) | (sw >> 19);
    return u64pair{aval64((uint64_t)(lo ^ sec32(0) ^ sec32(4))), aval64((uint64_t)(hi ^ sec32(8) ^ sec32(12)))};
  }
  if (len <= 8) {
    const uint64_t in_lo = msg_r32(m, 0), in_hi = msg_r32(m, len - 4);
    const uint64_t keyed = (in_lo + (in_hi << 32)) ^ (sec64(16) ^ sec64(24));
    const uint64_t mul = P64_1 + (len << 2);
    uint64_t lo = keyed * mul, hi = __umul64hi(keyed, mul);
    hi += lo << 1;
    lo ^= hi >> 3;
    lo ^= lo >> 35;
    lo *= MX2;
    lo ^= lo >> 28;
    return u64pair{lo, aval(hi)};
  }
  if (len <= 16) {
    const uint64_t in_lo = msg_r64(m, 0);
    uint64_t in_hi = msg_r64(m, len - 8);
    const uint64_t x = in_lo ^ in_hi ^ (sec64(32) ^ sec64(40));
    uint64_t mlo = x * P64_1, mhi = __umul64hi(x, P64_1);
    mlo += (len - 1) << 54;
    in_hi ^= sec64(48) ^ sec64(56);
    mhi += in_hi + (in_hi & 0xFFFFFFFFull) * (P32_2 - 1);
    mlo ^= __builtin_bswap64(mhi);
    return u64pair{aval(mlo * P64_2), aval(__umul64hi(mlo, P64_2) + mhi * P64_2)};
  }
  u64pair acc{len * P64_1, 0};
  if (len <= 128) {
    // (the pairs from the middle outwards: unlike the 64-bit sum, the order matters)
    for (uint32_t i = (uint32_t)((len - 1) >> 5) + 1; i-- > 0;) acc = mix32(acc, m, 16 * i, len - 16 * (i + 1), 32 * i);
  } else {
    for (uint32_t i = 0; i < 4; ++i) acc = mix32(acc, m, 32 * i, 32 * i + 16, 32 * i);
    acc.a = aval(acc.a);
    acc.b = aval(acc.b);
    const uint32_t rounds = (uint32_t)(len >> 5);
    for (uint32_t i = 4; i < rounds; ++i) acc = mix32(acc, m, 32 * i, 32 * i + 16, 3 + 32 * (i - 4));
    acc = mix32(acc, m, len - 16, len - 32, 103);
  }
  return u64pair{aval(acc.a + acc.b), 0 - aval(acc.a * P64_1 + acc.b * P64_4 + len * P64_2)};
}

// DwarFS's digest order (checksum_xxh3::finalize, src/checksum.cpp:185-196):
// the low 64 bits little endian, then the high 64
__device__ __forceinline__ void emit_xxh128(const Job& j, uint32_t b, u64pair h) {
  __builtin_memcpy(j.out + (size_t)j.out_stride * b, &h, 16);
}

__global__ __launch_bounds__(64) void rpp_xxh3_128_short_kernel(Job job, uint32_t n, uint32_t nwaves) {
  const uint64_t id = lane_message(nwaves);
  if (id >= n) return;
  const uint32_t b = (uint32_t)id;
  Msg m;
  if (!load_msg(job, b, m) || m.len > 240) return;
  emit_xxh128(job, b, xxh3_128_short(m));
}

// sum over the 16 lanes that share lane % 4
__device__ __forceinline__ uint64_t stripe_sum(uint64_t v) {
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// len > 240: one wave per message.  The 128-bit value (Wide) runs the same
// loop; its low half is the 64-bit merge, its high half a second merge over
// the secret's tail (offset 192 - 64 - 11) started from ~(len * PRIME64_2).
template <bool Wide>
__device__ __forceinline__ void xxh3_long(const Job& job, uint32_t n) {
  const uint32_t lane = threadIdx.x % 64, b = blockIdx.x * kLongWaves + threadIdx.x / 64;
  if (b >= n) return;  // (wave-uniform, like every exit below)
  Msg m;
  if (!load_msg(job, b, m) || m.len <= 240) return;
  const uint64_t len = m.len;
  const uint32_t q = lane % 4, stripe = lane / 4;
  const uint32_t soff = 8 * stripe + 16 * q;
  const uint64_t s0 = sec64(soff), s1 = sec64(soff + 8);
  const uint64_t sc0 = sec64(128 + 16 * q), sc1 = sec64(136 + 16 * q);
  // accumulators 2q and 2q+1, the same in the 16 lanes of a column
  uint64_t a0 = q == 0 ? P32_3 : q == 1 ? P64_2 : q == 2 ? P64_4 : P64_5;
  uint64_t a1 = q == 0 ? P64_1 : q == 1 ? P64_3 : q == 2 ? P32_2 : P32_1;
  const uint64_t nblocks = (len - 1) >> 10;
  const uint64_t lpos = 16 * lane;
  u64pair d{0, 0};
  if (nblocks) d = msg_r128(m, lpos);
  for (uint64_t blk = 0; blk < nblocks; ++blk) {
    u64pair nx{0, 0};
    // (positions from 1024 on are in the payload: the leading spans hold <= 96 bytes)
    if (blk + 1 < nblocks) nx = ld128(m.pay + (((blk + 1) << 10) + lpos - m.pre));
    const uint64_t c0 = stripe_sum(d.b + mul32x32(d.a ^ s0));
    const uint64_t c1 = stripe_sum(d.a + mul32x32(d.b ^ s1));
    a0 += c0;
    a1 += c1;
    a0 = (a0 ^ (a0 >> 47) ^ sc0) * P32_1;
    a1 = (a1 ^ (a1 >> 47) ^ sc1) * P32_1;
    d = nx;
  }
  // the partial block's full stripes, and the last stripe (at len - 64, secret
  // offset 121) in the lanes of the first unused stripe slot (nstripes <= 15)
  const uint64_t base = nblocks << 10;
  const uint32_t nstripes = (uint32_t)((len - 1) & 1023) >> 6;
  uint64_t c0 = 0, c1 = 0;
  if (stripe <= nstripes) {
    const bool last = stripe == nstripes;
    const u64pair t = msg_r128(m, last ? len - 64 + 16 * q : base + lpos);
    const uint64_t t0 = last ? sec64(121 + 16 * q) : s0, t1 = last ? sec64(129 + 16 * q) : s1;
    c0 = t.b + mul32x32(t.a ^ t0);
    c1 = t.a + mul32x32(t.b ^ t1);
  }
  a0 += stripe_sum(c0);
  a1 += stripe_sum(c1);
  uint64_t f = fold64(a0 ^ sec64(11 + 16 * q), a1 ^ sec64(19 + 16 * q));
  f += __shfl_xor(f, 1, 64);
  f += __shfl_xor(f, 2, 64);
  if constexpr (Wide) {
    uint64_t g = fold64(a0 ^ sec64(117 + 16 * q), a1 ^ sec64(125 + 16 * q));
    g += __shfl_xor(g, 1, 64);
    g += __shfl_xor(g, 2, 64);
    if (lane == 0) emit_xxh128(job, b, u64pair{aval(len * P64_1 + f), aval(~(len * P64_2) + g)});
  } else {
    if (lane == 0) emit_xxh(job, b, aval(len * P64_1 + f));
  }
}

__global__ __launch_bounds__(64 * kLongWaves) void rpp_xxh3_long_kernel(Job job, uint32_t n) {
  xxh3_long<false>(job, n);
}
__global__ __launch_bounds__(64 * kLongWaves) void rpp_xxh3_128_long_kernel(Job job, uint32_t n) {
  xxh3_long<true>(job, n);
}

// ---- SHA-512/256 ----

template <int N>
__device__ __forceinline__ uint64_t rotr(uint64_t x) {
  return (x >> N) | (x << (64 - N));
}

// big-endian word of the padded message at byte `pos`
__device__ __forceinline__ uint64_t sha_word(const Msg& m, uint64_t pos) {
  if (pos + 8 <= m.len) return __builtin_bswap64(msg_r64(m, pos));
  uint64_t w = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t p = pos + k;
    const uint64_t byte = p < m.len ? msg_byte(m, p) : (p == m.len ? 0x80u : 0u);
    w = (w << 8) | byte;
  }
  return w;
}

#define RPP_SHA_ROUND(i, k)                                                                \
  {                                                                                        \
    const uint64_t t1 = hh + (rotr<14>(e) ^ rotr<18>(e) ^ rotr<41>(e)) + ((e & f) ^ (~e & g)) + (k) + w[i]; \
    const uint64_t t2 = (rotr<28>(a) ^ rotr<34>(a) ^ rotr<39>(a)) + ((a & b) ^ (a & c) ^ (b & c));          \
    hh = g;                                                                                \
    g = f;                                                                                 \
    f = e;                                                                                 \
    e = d + t1;                                                                            \
    d = c;                                                                                 \
    c = b;                                                                                 \
    b = a;                                                                                 \
    a = t1 + t2;                                                                           \
  }

__device__ __forceinline__ void sha_compress(uint64_t (&st)[8], uint64_t (&w)[16]) {
  uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], hh = st[7];
#pragma unroll
  for (int i = 0; i < 16; ++i) RPP_SHA_ROUND(i, d_sha_k[i])
#pragma unroll 1
  for (int t = 16; t < 80; t += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      w[i] += (rotr<1>(w15) ^ rotr<8>(w15) ^ (w15 >> 7)) + w[(i + 9) & 15] + (rotr<19>(w2) ^ rotr<61>(w2) ^ (w2 >> 6));
      RPP_SHA_ROUND(i, d_sha_k[t + i])
    }
  }
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
  st[4] += e;
  st[5] += f;
  st[6] += g;
  st[7] += hh;
}

__global__ __launch_bounds__(64) void rpp_sha512_256_kernel(Job job, uint32_t n, uint32_t nwaves) {
  const uint64_t id = lane_message(nwaves);
  if (id >= n) return;
  const uint32_t b = (uint32_t)id;
  Msg m;
  if (!load_msg(job, b, m)) return;
  uint64_t st[8], w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = d_sha_iv[i];
  // 0x80, zeros to 112 mod 128, the 128-bit bit length (messages are below 2^61 bytes)
  const uint64_t nblocks = (m.len + 17 + 127) >> 7;
  for (uint64_t blk = 0; blk < nblocks; ++blk) {
    const uint64_t pos = blk << 7;
    if (pos >= m.pre && pos + 128 <= m.len) {
      const uint8_t* p = m.pay + (pos - m.pre);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const u64pair v = ld128(p + 16 * i);
        w[2 * i] = __builtin_bswap64(v.a);
        w[2 * i + 1] = __builtin_bswap64(v.b);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) w[i] = sha_word(m, pos + 8 * i);
      if (blk + 1 == nblocks) {
        w[14] = m.len >> 61;
        w[15] = m.len << 3;
      }
    }
    sha_compress(st, w);
  }
  uint64_t dg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dg[i] = __builtin_bswap64(st[i]);
  if (job.sections) {
    const uint8_t* h = job.data + job.offs[b] + kOffSha;
    bool same = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) same = same && ld64(h + 8 * i) == dg[i];
    if (!same) job.status[b] = RPP_CHECKSUM_MISMATCH;
  } else {
    __builtin_memcpy(job.out + (size_t)job.out_stride * b, dg, 32);
  }
}

// ---- section headers ----

// everything of section_header_v2 but the two checksums
__global__ void rpp_section_fields_kernel(const uint64_t* payload_sizes, const uint32_t* frame_len, uint32_t n,
                                          uint32_t first_number, uint32_t type, uint32_t compression,
                                          uint8_t* headers) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  uint8_t* h = headers + (size_t)kHeaderBytes * b;
  const uint8_t magic[8] = {'D', 'W', 'A', 'R', 'F', 'S', 2, 5};  // MAJOR_VERSION, MINOR_VERSION (fstypes.h:46-47)
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = magic[i];
  uint32_t fl = frame_len ? frame_len[b] : 0u;
  fl = fl < kFrameRow ? fl : kFrameRow;
  const uint32_t number = first_number + b;
  const uint32_t tc = (type & 0xFFFFu) | (compression << 16);
  const uint64_t length = payload_sizes[b] + fl;
  __builtin_memcpy(h + kOffNumber, &number, 4);
  __builtin_memcpy(h + kOffNumber + 4, &tc, 4);
  __builtin_memcpy(h + kOffLength, &length, 8);
}

// fs_section_v2's header checks, and the section's extent against the image
__global__ void rpp_section_parse_kernel(const uint8_t* image, uint64_t image_bytes, const uint64_t* offs, uint32_t n,
                                         int32_t* status) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint64_t off = offs[b];
  int32_t st = RPP_OK;
  if (off > image_bytes || image_bytes - off < kHeaderBytes) {
    st = RPP_TRUNCATED_INPUT;
  } else {
    const uint8_t* h = image + off;
    const uint8_t magic[7] = {'D', 'W', 'A', 'R', 'F', 'S', 2};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) ok = ok && h[i] == magic[i];
    if (!ok)
      st = RPP_INVALID_ARGUMENT;
    else if (ld64(h + kOffLength) > image_bytes - off - kHeaderBytes)
      st = RPP_TRUNCATED_INPUT;
  }
  status[b] = st;
}

// ---- byte-packed assembly ----

__global__ void rpp_section_sizes_kernel(const uint64_t* payload_sizes, const uint32_t* frame_len, uint32_t n,
                                         uint64_t* section_sizes) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  uint32_t fl = frame_len ? frame_len[b] : 0u;
  fl = fl < kFrameRow ? fl : kFrameRow;
  section_sizes[b] = kHeaderBytes + fl + payload_sizes[b];
}

// dst[0, n) = src[0, n) for any alignment of either, by the threads t, t + step, ...
// of a group: bytes up to dst's first 16-byte boundary, aligned 16-byte stores
// fed by unaligned loads, then the last bytes.  Touches nothing outside either span.
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint64_t n, uint64_t t, uint64_t step) {
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
  head = head < n ? head : n;
  const uint64_t n16 = (n - head) >> 4, tail0 = head + (n16 << 4);
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  for (uint64_t i = t; i < n16; i += step) {
    u32x4 v;
    __builtin_memcpy(&v, src + head + (i << 4), 16);
    *reinterpret_cast<u32x4*>(dst + head + (i << 4)) = v;
  }
  // (at most 15 + 15 bytes)
  for (uint64_t i = t; i < head + (n - tail0); i += step) {
    const uint64_t p = i < head ? i : tail0 + (i - head);
    dst[p] = src[p];
  }
}

// section b = header | frame | payload at image + section_offsets[b]; blockIdx.y
// splits a section's bytes over several workgroups
__global__ __launch_bounds__(kCopyThreads) void rpp_section_copy_kernel(
    const uint8_t* headers, const uint8_t* frame, const uint32_t* frame_len, const uint8_t* payload,
    const uint64_t* payload_offs, const uint64_t* payload_sizes, const uint64_t* section_offs, uint32_t n,
    uint8_t* image, uint64_t* total) {
  const uint32_t b = blockIdx.x;
  const uint64_t t = (uint64_t)blockIdx.y * kCopyThreads + threadIdx.x, step = (uint64_t)gridDim.y * kCopyThreads;
  uint32_t fl = frame ? frame_len[b] : 0u;
  fl = fl < kFrameRow ? fl : kFrameRow;
  uint8_t* dst = image + section_offs[b];
  const uint64_t psize = payload_sizes[b];
  copy_bytes(dst, headers + (size_t)kHeaderBytes * b, kHeaderBytes, t, step);
  if (fl) copy_bytes(dst + kHeaderBytes, frame + (size_t)kFrameRow * b, fl, t, step);
  copy_bytes(dst + kHeaderBytes + fl, payload + payload_offs[b], psize, t, step);
  if (total && b == n - 1 && t == 0) *total = section_offs[b] + kHeaderBytes + fl + psize;
}

// ---- grouping equal keys (file_scanner_::scan_dedupe's unique_size_ / by_hash_ maps) ----
//
// A key is sizes[b] plus `words` 64-bit words of digest row b.  Open addressing
// over `mask + 1` >= 2n slots of key indices, linear probing from key_slot().
// A slot's occupant only ever changes to a smaller index with the same key and
// a slot never empties, so a key's probe sequence always ends at the same slot:
// all equal keys settle in one slot, which ends up holding their smallest index
// whatever the order the lanes ran in.

constexpr uint32_t kEmptySlot = 0xFFFFFFFFu;
constexpr uint32_t kGroupThreads = 256;

struct Keys {
  const uint64_t* sizes;
  const uint8_t* digest;  // rows of 8 * words bytes
  uint32_t words;
  const uint8_t* select;
};

__host__ __device__ inline uint64_t key_mix(uint64_t h, uint64_t w) {
  h = (h ^ w) * P64_2;
  return h ^ (h >> 29);
}
// start slot of a key, before masking
__host__ __device__ inline uint64_t key_finish(uint64_t h) {
  h *= P64_3;
  return h ^ (h >> 32);
}

__device__ __forceinline__ uint64_t key_slot(const Keys& k, uint32_t b) {
  uint64_t h = key_mix(P64_1, k.sizes[b]);
  for (uint32_t w = 0; w < k.words; ++w) h = key_mix(h, ld64(k.digest + 8 * ((size_t)k.words * b + w)));
  return key_finish(h);
}
__device__ __forceinline__ bool key_equal(const Keys& k, uint32_t a, uint32_t b) {
  bool same = k.sizes[a] == k.sizes[b];
  for (uint32_t w = 0; w < k.words; ++w)
    same = same && ld64(k.digest + 8 * ((size_t)k.words * a + w)) == ld64(k.digest + 8 * ((size_t)k.words * b + w));
  return same;
}

__global__ __launch_bounds__(kGroupThreads) void rpp_group_insert_kernel(Keys k, uint32_t n, uint32_t* table,
                                                                          uint32_t mask) {
  const uint32_t b = blockIdx.x * kGroupThreads + threadIdx.x;
  if (b >= n || (k.select && !k.select[b])) return;
  uint32_t slot = (uint32_t)key_slot(k, b) & mask;
  // (at most n slots are ever occupied, of more than n: the walk meets an empty one)
  for (uint32_t probes = 0; probes <= mask; ++probes) {
    const uint32_t cur = atomicCAS(table + slot, kEmptySlot, b);
    if (cur == kEmptySlot) return;
    if (cur < n && key_equal(k, cur, b)) {
      atomicMin(table + slot, b);
      return;
    }
    slot = (slot + 1) & mask;
  }
}

// (a launch of its own: every insert is done)
__global__ __launch_bounds__(kGroupThreads) void rpp_group_lookup_kernel(Keys k, uint32_t n, const uint32_t* table,
                                                                          uint32_t mask, uint32_t* first,
                                                                          uint8_t* multi) {
  const uint32_t b = blockIdx.x * kGroupThreads + threadIdx.x;
  if (b >= n) return;
  uint32_t f = b;
  if (!k.select || k.select[b]) {
    uint32_t slot = (uint32_t)key_slot(k, b) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes) {
      const uint32_t cur = table[slot];
      if (cur >= n) break;  // (empty: cannot happen after the insert)
      if (key_equal(k, cur, b)) {
        f = cur;
        break;
      }
      slot = (slot + 1) & mask;
    }
  }
  first[b] = f;
  if (f != b && multi) {
    multi[b] = 1;
    multi[f] = 1;
  }
}

// slots of the table for n keys: the power of two >= 2n (and >= 4)
uint64_t group_slots(uint32_t n) {
  uint64_t s = 4;
  while (s < 2ull * n) s <<= 1;
  return s;
}

int launched() { return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR; }

int launch_group(const Keys& k, uint32_t n, uint32_t* first, uint8_t* multi, void* ws, hipStream_t s) {
  const uint64_t slots = group_slots(n);
  uint32_t* table = static_cast<uint32_t*>(ws);
  if (hipMemsetAsync(table, 0xFF, slots * sizeof(uint32_t), s) != hipSuccess) return RPP_HIP_ERROR;
  if (multi && hipMemsetAsync(multi, 0, n, s) != hipSuccess) return RPP_HIP_ERROR;
  const uint32_t grid = (n + kGroupThreads - 1) / kGroupThreads, mask = (uint32_t)(slots - 1);
  hipLaunchKernelGGL(rpp_group_insert_kernel, dim3(grid), dim3(kGroupThreads), 0, s, k, n, table, mask);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  hipLaunchKernelGGL(rpp_group_lookup_kernel, dim3(grid), dim3(kGroupThreads), 0, s, k, n, table, mask, first, multi);
  return launched();
}

int launch_xxh3_128(const Job& job, uint32_t n, hipStream_t s) {
  const uint32_t nw = lane_waves(n);
  hipLaunchKernelGGL(rpp_xxh3_128_short_kernel, dim3(nw), dim3(64), 0, s, job, n, nw);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  hipLaunchKernelGGL(rpp_xxh3_128_long_kernel, dim3((n + kLongWaves - 1) / kLongWaves), dim3(64 * kLongWaves), 0, s,
                     job, n);
  return launched();
}

int launch_xxh3(const Job& job, uint32_t n, hipStream_t s) {
  const uint32_t nw = lane_waves(n);
  hipLaunchKernelGGL(rpp_xxh3_short_kernel, dim3(nw), dim3(64), 0, s, job, n, nw);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  hipLaunchKernelGGL(rpp_xxh3_long_kernel, dim3((n + kLongWaves - 1) / kLongWaves), dim3(64 * kLongWaves), 0, s, job,
                     n);
  return launched();
}

int launch_sha(const Job& job, uint32_t n, hipStream_t s) {
  const uint32_t nw = lane_waves(n);
  hipLaunchKernelGGL(rpp_sha512_256_kernel, dim3(nw), dim3(64), 0, s, job, n, nw);
  return launched();
}

Job plain_job(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes, const uint8_t* d_prefix,
              const uint32_t* d_prefix_len, void* out, uint32_t out_stride) {
  Job j{};
  j.data = d_data;
  j.offs = d_offsets;
  j.sizes = d_sizes;
  j.seg0 = d_prefix;
  j.seg0_len = d_prefix_len;
  j.seg0_stride = 64;
  j.out = static_cast<uint8_t*>(out);
  j.out_stride = out_stride;
  return j;
}

}  // namespace

extern "C" int rpp_xxh3_64_batch(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n,
                                 const uint8_t* d_prefix, const uint32_t* d_prefix_len, uint64_t* d_hash,
                                 void* stream) {
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_hash || (d_prefix && !d_prefix_len)) return RPP_INVALID_ARGUMENT;
  return launch_xxh3(plain_job(d_data, d_offsets, d_sizes, d_prefix, d_prefix_len, d_hash, 8), n, (hipStream_t)stream);
}

extern "C" int rpp_sha512_256_batch(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                    uint32_t n, const uint8_t* d_prefix, const uint32_t* d_prefix_len,
                                    uint8_t* d_digest, void* stream) {
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_digest || (d_prefix && !d_prefix_len)) return RPP_INVALID_ARGUMENT;
  return launch_sha(plain_job(d_data, d_offsets, d_sizes, d_prefix, d_prefix_len, d_digest, 32), n,
                    (hipStream_t)stream);
}

extern "C" int rpp_xxh3_128_batch(const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                  uint32_t n, const uint8_t* d_prefix, const uint32_t* d_prefix_len,
                                  uint8_t* d_digest, void* stream) {
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_digest || (d_prefix && !d_prefix_len)) return RPP_INVALID_ARGUMENT;
  return launch_xxh3_128(plain_job(d_data, d_offsets, d_sizes, d_prefix, d_prefix_len, d_digest, 16), n,
                         (hipStream_t)stream);
}

// ---- duplicate-file detection (file_scanner_::scan_dedupe, src/writer/internal/file_scanner.cpp:274-413) ----

namespace {

constexpr uint64_t kLargeFileThreshold = 1024 * 1024;  // file_scanner.cpp:59
constexpr uint64_t kLargeFileStartHashSize = 4096;     // file_scanner.cpp:60
constexpr uint32_t kGroupMaxKeys = 1u << 30;

int launch_file_hash(int algo, Job job, uint32_t n, hipStream_t s) {
  job.out_stride = (uint32_t)rpp_file_hash_digest_bytes(algo);
  switch (algo) {
    case RPP_HASH_XXH3_64: return launch_xxh3(job, n, s);
    case RPP_HASH_XXH3_128: return launch_xxh3_128(job, n, s);
    case RPP_HASH_SHA512_256: return launch_sha(job, n, s);
  }
  return RPP_INVALID_ARGUMENT;
}

uint64_t align16u(uint64_t v) { return (v + 15) & ~15ull; }

}  // namespace

extern "C" int rpp_file_hash_algo(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "xxh3-64")) return RPP_HASH_XXH3_64;
  if (!strcmp(name, "xxh3-128")) return RPP_HASH_XXH3_128;
  if (!strcmp(name, "sha512-256")) return RPP_HASH_SHA512_256;
  return -1;
}

extern "C" int rpp_file_hash_digest_bytes(int algo) {
  switch (algo) {
    case RPP_HASH_XXH3_64: return 8;
    case RPP_HASH_XXH3_128: return 16;
    case RPP_HASH_SHA512_256: return 32;
  }
  return 0;
}

extern "C" int rpp_file_hash_batch(int algo, const uint8_t* d_data, const uint64_t* d_offsets,
                                   const uint64_t* d_sizes, const uint8_t* d_select, uint32_t n, uint8_t* d_digest,
                                   void* stream) {
  if (rpp_file_hash_digest_bytes(algo) == 0) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_digest) return RPP_INVALID_ARGUMENT;
  Job j = plain_job(d_data, d_offsets, d_sizes, nullptr, nullptr, d_digest, 0);
  j.select = d_select;
  return launch_file_hash(algo, j, n, (hipStream_t)stream);
}

extern "C" uint64_t rpp_group_workspace_bytes(uint32_t n) { return group_slots(n) * sizeof(uint32_t); }

extern "C" uint64_t rpp_group_start_slot(uint64_t size, const uint8_t* digest, uint32_t digest_bytes, uint32_t n) {
  uint64_t h = key_mix(P64_1, size);
  for (uint32_t w = 0; digest && w < digest_bytes / 8; ++w) {
    uint64_t v;
    memcpy(&v, digest + 8 * w, 8);
    h = key_mix(h, v);
  }
  return key_finish(h) & 0xFFFFFFFFu & (group_slots(n) - 1);
}

extern "C" int rpp_group_first_batch(const uint64_t* d_sizes, const uint8_t* d_digest, uint32_t digest_bytes,
                                     const uint8_t* d_select, uint32_t n, uint32_t* d_first, uint8_t* d_multi,
                                     void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (digest_bytes != 0 && digest_bytes != 8 && digest_bytes != 16 && digest_bytes != 32) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_sizes || !d_first || !d_workspace || n > kGroupMaxKeys || workspace_bytes < rpp_group_workspace_bytes(n))
    return RPP_INVALID_ARGUMENT;
  const Keys k{d_sizes, d_digest, d_digest ? digest_bytes / 8 : 0u, d_select};
  return launch_group(k, n, d_first, d_multi, d_workspace, (hipStream_t)stream);
}

// workspace: the table | one start hash per file
extern "C" uint64_t rpp_file_dedup_workspace_bytes(uint32_t n) {
  return align16u(rpp_group_workspace_bytes(n)) + sizeof(uint64_t) * (uint64_t)n;
}

extern "C" int rpp_file_dedup_batch(int algo, const uint8_t* d_data, const uint64_t* d_offsets,
                                    const uint64_t* d_sizes, uint32_t n, uint8_t* d_digest, uint32_t* d_first,
                                    uint8_t* d_hashed, void* d_workspace, uint64_t workspace_bytes, void* stream) {
  const uint32_t dbytes = (uint32_t)rpp_file_hash_digest_bytes(algo);
  if (dbytes == 0) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_digest || !d_first || !d_hashed || !d_workspace || n > kGroupMaxKeys ||
      workspace_bytes < rpp_file_dedup_workspace_bytes(n))
    return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* d_start = static_cast<uint8_t*>(d_workspace) + align16u(rpp_group_workspace_bytes(n));
  // the scanner's start hash: XXH3-64 of the first 4 KiB of a file of 1 MiB and up, 0 below
  if (hipMemsetAsync(d_start, 0, sizeof(uint64_t) * (size_t)n, s) != hipSuccess) return RPP_HIP_ERROR;
  Job j = plain_job(d_data, d_offsets, d_sizes, nullptr, nullptr, d_start, 8);
  j.min_size = kLargeFileThreshold;
  j.clamp = kLargeFileStartHashSize;
  int st = launch_xxh3(j, n, s);
  if (st != RPP_OK) return st;
  // files sharing (size, start hash) are hashed (d_first is scratch here) ...
  st = launch_group(Keys{d_sizes, d_start, 1, nullptr}, n, d_first, d_hashed, d_workspace, s);
  if (st != RPP_OK) return st;
  j = plain_job(d_data, d_offsets, d_sizes, nullptr, nullptr, d_digest, 0);
  j.select = d_hashed;
  st = launch_file_hash(algo, j, n, s);
  if (st != RPP_OK) return st;
  // ... and those with equal (size, digest) share the first one's inode
  return launch_group(Keys{d_sizes, d_digest, dbytes / 8, d_hashed}, n, d_first, nullptr, d_workspace, s);
}

extern "C" int rpp_section_headers_batch(const uint8_t* d_payload, const uint64_t* d_payload_offsets,
                                         const uint64_t* d_payload_sizes, uint32_t n, uint32_t first_number,
                                         uint32_t section_type, uint32_t compression, const uint8_t* d_frame,
                                         const uint32_t* d_frame_len, uint8_t* d_headers, void* stream) {
  if (n == 0) return RPP_OK;
  if (!d_payload || !d_payload_offsets || !d_payload_sizes || !d_headers || (d_frame && !d_frame_len) ||
      section_type > 0xFFFFu || compression > 0xFFFFu)
    return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rpp_section_fields_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_payload_sizes,
                     d_frame ? d_frame_len : nullptr, n, first_number, section_type, compression, d_headers);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  // XXH3-64 over header[48,64) + frame + payload into header[40,48) ...
  Job j{};
  j.data = d_payload;
  j.offs = d_payload_offsets;
  j.sizes = d_payload_sizes;
  j.seg0 = d_headers + kOffNumber;
  j.seg0_stride = kHeaderBytes;
  j.seg0_fixed = kHeaderBytes - kOffNumber;
  j.seg1 = d_frame;
  j.seg1_len = d_frame_len;
  j.out = d_headers + kOffXxh;
  j.out_stride = kHeaderBytes;
  const int st = launch_xxh3(j, n, s);
  if (st != RPP_OK) return st;
  // ... which the SHA-512/256 over header[40,64) + frame + payload covers, into header[8,40)
  j.seg0 = d_headers + kOffXxh;
  j.seg0_fixed = kHeaderBytes - kOffXxh;
  j.out = d_headers + kOffSha;
  return launch_sha(j, n, s);
}

extern "C" int rpp_sections_assemble_batch(const uint8_t* d_headers, const uint8_t* d_frame,
                                           const uint32_t* d_frame_len, const uint8_t* d_payload,
                                           const uint64_t* d_payload_offsets, const uint64_t* d_payload_sizes,
                                           uint32_t n, uint8_t* d_image, uint64_t* d_section_sizes,
                                           uint64_t* d_section_offsets, uint64_t* d_total, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (!d_total) return RPP_OK;
    return hipMemsetAsync(d_total, 0, sizeof(uint64_t), s) == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
  }
  if (!d_headers || !d_payload || !d_payload_offsets || !d_payload_sizes || !d_image || !d_section_sizes ||
      !d_section_offsets || (d_frame && !d_frame_len))
    return RPP_INVALID_ARGUMENT;
  hipLaunchKernelGGL(rpp_section_sizes_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_payload_sizes,
                     d_frame ? d_frame_len : nullptr, n, d_section_sizes);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  const int st = rpp_exclusive_scan_u64(d_section_sizes, n, d_section_offsets, stream);
  if (st != RPP_OK) return st;
  // few sections: several workgroups share each one's bytes
  uint32_t split = 2048 / n;
  split = split < 1 ? 1 : split > 64 ? 64 : split;
  hipLaunchKernelGGL(rpp_section_copy_kernel, dim3(n, split), dim3(kCopyThreads), 0, s, d_headers, d_frame,
                     d_frame_len, d_payload, d_payload_offsets, d_payload_sizes, d_section_offsets, n, d_image,
                     d_total);
  return launched();
}

extern "C" int rpp_sections_verify_batch(const uint8_t* d_image, uint64_t image_bytes,
                                         const uint64_t* d_section_offsets, uint32_t n, uint32_t level,
                                         int32_t* d_status, void* stream) {
  if (level < 1 || level > 2) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_image || !d_section_offsets || !d_status) return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rpp_section_parse_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_image, image_bytes,
                     d_section_offsets, n, d_status);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  Job j{};
  j.data = d_image;
  j.offs = d_section_offsets;
  j.sections = 1;
  j.from = kOffNumber;
  j.status = d_status;
  int st = launch_xxh3(j, n, s);
  if (st != RPP_OK || level < 2) return st;
  j.from = kOffXxh;
  return launch_sha(j, n, s);
}

extern "C" int rpp_parse_section_header(const uint8_t in[64], rpp_section_header* out) {
  if (!in || !out) return RPP_INVALID_ARGUMENT;
  if (memcmp(in, "DWARFS", 6) != 0 || in[6] != 2) return RPP_INVALID_ARGUMENT;
  auto le = [&](uint32_t at, uint32_t nbytes) {
    uint64_t v = 0;
    for (uint32_t i = nbytes; i-- > 0;) v = (v << 8) | in[at + i];
    return v;
  };
  out->major = in[6];
  out->minor = in[7];
  memcpy(out->sha2_512_256, in + kOffSha, 32);
  out->xxh3_64 = le(kOffXxh, 8);
  out->number = (uint32_t)le(kOffNumber, 4);
  out->type = (uint16_t)le(kOffNumber + 4, 2);
  out->compression = (uint16_t)le(kOffNumber + 6, 2);
  out->length = le(kOffLength, 8);
  return RPP_OK;
}
