// lz4_host.cpp -- the host side of the LZ4 block codec: the DwarFS framing
// (src/compression/lz4.cpp:88-106 write, :127-169 read: a uint32 little-endian
// uncompressed size in front of one LZ4 block), the size bound, and the
// sequential restatements of the two kernels of lz4_kernels.hip.  Plain C++:
// the sanitizer test (tests/cpp/lz4_test.cpp) compiles this file alone.
//
// Decode contract (both the kernel and rpp_lz4_host_decode): sequences are
// decoded in order, each copy is checked before it is made, and the first
// check that fails ends the stream with RPP_CORRUPT_INPUT, leaving what the
// earlier sequences wrote.  Stricter than the reference, which accepts a
// stream that produces fewer bytes than the frame states (lz4.cpp:143-152): a
// valid image never holds one.  More lenient than LZ4_decompress_safe in one
// way: the end-of-block rules (last 5 bytes literals, last match 12 bytes
// before the end) are the encoder's duty and are not checked here.
//
// Encoder definition (both the kernels and rpp_lz4_host_encode), for a block
// of n bytes; n < 13 is one literal run:
//   * the block is cut into chunks of kChunk bytes.  A chunk has a table of
//     2^kHashBits entries keyed by hash4 of the 4 bytes at a position; an entry
//     holds the highest position inserted so far.  The table starts with every
//     position of the kChunk bytes before the chunk.
//   * the chunk's positions are taken in steps of kStep.  A step is skipped
//     whole when the last match ends at or behind its end.  Otherwise every
//     position of the step first looks its candidate up, then all of them are
//     inserted (so a candidate always lies in an earlier step).
//   * a position p has a match when its candidate c holds the same 4 bytes,
//     p - c <= 65535, p + 12 <= n and p + 4 <= min(chunk end, n - 5).  Greedy:
//     the first such position at or behind the end of the last match is taken;
//     its length is the common prefix, cut at min(chunk end, n - 5).
//   * the sequences of all chunks, in order, are one LZ4 block: a literal run
//     that spans a chunk boundary belongs to the next match, wherever it is.
//
// The search word (find_sequences with `search`, the *_search entry points):
// depth | RPP_SEARCH_LAZY with a depth of 1, 2, 4 or 8; 0 is the definition
// above and any other word an invalid argument.  Chunks, the table's start
// (the kChunk bytes before the chunk), steps (every lookup before the step's
// inserts, a covered step skipped whole, its positions never inserted), hash4,
// the conditions on a match and the cut of a length stay as above, with
// last_start = n - 12 and lim_end = min(chunk end, n - 5).  Four things change:
//   * bucket: a hash value holds the `depth` highest positions inserted so far.
//   * score: a position p with p <= last_start and p + 4 <= lim_end scores
//     every candidate c of its bucket that holds the same 4 bytes at
//     p - c <= 65535: min(common prefix cut at lim_end, kDeepCap).  best(p) is
//     the candidate with the highest score, of equal scores the highest
//     position (the smallest offset).
//   * choice: without LAZY the first position at or behind the cursor that has
//     a best is taken.  With LAZY a position p is passed over (it becomes a
//     literal) when p + 1 lies in the same step and has a best whose score is
//     strictly greater; the position taken is the first one at or behind the
//     cursor that has a best and is not passed over.  A step's last position
//     is never passed over, nor is a score of kDeepCap.
//   * length: the match taken is (p, best(p)) with the full common prefix, cut
//     at lim_end; the cursor moves to its end and the step goes on.
// Depth 1 without LAZY gives the sequences of search 0.  `level` maps to no
// word: that table needs timings first.
#include <algorithm>
#include <cstring>
#include <vector>

#include "lz4_common.h"
#include "lz4_internal.h"
#include "ricepp_amd.h"

namespace {

using namespace rpp_lz4;

inline uint32_t rd32(const uint8_t* p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

}  // namespace

void rpp_lz4::find_sequences(const uint8_t* in, uint32_t n, std::vector<Seq>& seqs) {
  if (n < kMatchStartGap + 1) return;
  const uint32_t last_start = n - kMatchStartGap, match_end = n - kLastLiterals;
  std::vector<uint32_t> tab(1u << kHashBits);  // position + 1; 0: empty
  for (uint32_t cs = 0; cs < n; cs += kChunk) {
    const uint32_t ce = std::min(cs + kChunk, n), lim_end = std::min(ce, match_end);
    std::fill(tab.begin(), tab.end(), 0u);
    for (uint32_t q = cs >= kChunk ? cs - kChunk : 0; q < cs; ++q)
      if (q + 4 <= n) tab[hash4(rd32(in + q))] = q + 1;
    uint32_t cursor = cs;  // the end of the chunk's last match
    for (uint32_t ss = cs; ss < ce; ss += kStep) {
      const uint32_t se = std::min(ss + kStep, ce);
      if (cursor >= se) continue;
      uint32_t cand[kStep];
      for (uint32_t p = ss; p < se; ++p) cand[p - ss] = p + 4 <= n ? tab[hash4(rd32(in + p))] : 0;
      for (uint32_t p = ss; p < se; ++p)
        if (p + 4 <= n) tab[hash4(rd32(in + p))] = p + 1;
      for (uint32_t p = std::max(cursor, ss); p < se; ++p) {
        if (!cand[p - ss]) continue;
        const uint32_t c = cand[p - ss] - 1;
        if (p > last_start || p + 4 > lim_end || p - c > kMaxOffset || rd32(in + c) != rd32(in + p)) continue;
        const uint32_t lim = lim_end - p;
        uint32_t len = 4;
        while (len < lim && in[c + len] == in[p + len]) ++len;
        seqs.push_back({p, len, p - c});
        cursor = p + len;
        p = cursor - 1;
      }
    }
  }
}

void rpp_lz4::find_sequences(const uint8_t* in, uint32_t n, std::vector<Seq>& seqs, uint32_t search) {
  if (search == 0) return find_sequences(in, n, seqs);
  if (n < kMatchStartGap + 1) return;
  const uint32_t depth = search & ~kSearchLazy;
  const bool lazy = search & kSearchLazy;
  const uint32_t last_start = n - kMatchStartGap, match_end = n - kLastLiterals;
  std::vector<uint32_t> tab(size_t(depth) << kHashBits);  // per hash value: position + 1, highest first; 0: empty
  auto insert = [&](uint32_t q) {
    uint32_t* const b = tab.data() + size_t(hash4(rd32(in + q))) * depth;
    for (uint32_t k = depth - 1; k > 0; --k) b[k] = b[k - 1];
    b[0] = q + 1;
  };
  for (uint32_t cs = 0; cs < n; cs += kChunk) {
    const uint32_t ce = std::min(cs + kChunk, n), lim_end = std::min(ce, match_end);
    std::fill(tab.begin(), tab.end(), 0u);
    for (uint32_t q = cs >= kChunk ? cs - kChunk : 0; q < cs; ++q)
      if (q + 4 <= n) insert(q);
    uint32_t cursor = cs;  // the end of the chunk's last match
    for (uint32_t ss = cs; ss < ce; ss += kStep) {
      const uint32_t se = std::min(ss + kStep, ce);
      if (cursor >= se) continue;
      uint32_t best[kStep], score[kStep];  // best: candidate + 1; 0: none
      for (uint32_t p = ss; p < se; ++p) {
        uint32_t& bc = best[p - ss] = 0;
        uint32_t& bs = score[p - ss] = 0;
        if (p > last_start || p + 4 > lim_end) continue;
        const uint32_t word = rd32(in + p), lim = std::min(lim_end - p, kDeepCap);
        const uint32_t* const b = tab.data() + size_t(hash4(word)) * depth;
        for (uint32_t k = 0; k < depth && b[k]; ++k) {
          const uint32_t c = b[k] - 1;
          if (p - c > kMaxOffset || rd32(in + c) != word) continue;
          uint32_t s = 4;
          while (s < lim && in[c + s] == in[p + s]) ++s;
          if (s > bs) bs = s, bc = c + 1;
        }
      }
      for (uint32_t p = ss; p < se; ++p)
        if (p + 4 <= n) insert(p);
      for (uint32_t p = std::max(cursor, ss); p < se; ++p) {
        const uint32_t i = p - ss;
        if (!best[i]) continue;
        if (lazy && p + 1 < se && best[i + 1] && score[i + 1] > score[i]) continue;
        const uint32_t c = best[i] - 1, lim = lim_end - p;
        uint32_t len = score[i];
        while (len < lim && in[c + len] == in[p + len]) ++len;
        seqs.push_back({p, len, p - c});
        cursor = p + len;
        p = cursor - 1;
      }
    }
  }
}

namespace {

uint8_t* put_length(uint8_t* o, uint32_t v) {  // the extension bytes of a nibble that stands for v >= 15
  for (v -= 15; v >= 255; v -= 255) *o++ = 255;
  *o++ = uint8_t(v);
  return o;
}

}  // namespace

extern "C" uint64_t rpp_lz4_bound(uint64_t n) { return n + n / 255 + 16; }
extern "C" uint32_t rpp_lz4_chunk_bytes(void) { return rpp_lz4::kChunk; }
extern "C" uint32_t rpp_lz4_step_positions(void) { return rpp_lz4::kStep; }

extern "C" size_t rpp_lz4_frame_header(uint32_t uncompressed_bytes, uint8_t* out) {
  for (int i = 0; i < 4; ++i) out[i] = uint8_t(uncompressed_bytes >> (8 * i));
  return 4;
}

extern "C" long rpp_lz4_parse_frame(const uint8_t* data, size_t size, uint32_t* uncompressed_bytes) {
  if (!data || size < 4) return RPP_TRUNCATED_INPUT;
  if (uncompressed_bytes) *uncompressed_bytes = rd32(data);
  return 4;
}

extern "C" int rpp_lz4_host_decode(const uint8_t* in, uint64_t in_bytes, uint8_t* out, uint64_t out_bytes) {
  if ((in_bytes && !in) || (out_bytes && !out)) return RPP_INVALID_ARGUMENT;
  uint64_t ip = 0, op = 0;
  for (;;) {
    if (ip >= in_bytes) return RPP_CORRUPT_INPUT;
    const uint32_t token = in[ip++];
    uint64_t lit = token >> 4;
    if (lit == 15)
      for (;;) {
        if (ip >= in_bytes) return RPP_CORRUPT_INPUT;
        const uint32_t b = in[ip++];
        lit += b;
        if (b != 255) break;
      }
    if (lit > in_bytes - ip || lit > out_bytes - op) return RPP_CORRUPT_INPUT;
    if (lit) std::memcpy(out + op, in + ip, lit);
    ip += lit;
    op += lit;
    if (ip == in_bytes) break;  // the last sequence ends after its literals
    if (in_bytes - ip < 2) return RPP_CORRUPT_INPUT;
    const uint32_t off = uint32_t(in[ip]) | uint32_t(in[ip + 1]) << 8;
    ip += 2;
    if (off == 0 || off > op) return RPP_CORRUPT_INPUT;
    uint64_t len = (token & 15) + kMinMatch;
    if ((token & 15) == 15)
      for (;;) {
        if (ip >= in_bytes) return RPP_CORRUPT_INPUT;
        const uint32_t b = in[ip++];
        len += b;
        if (b != 255) break;
      }
    if (len > out_bytes - op) return RPP_CORRUPT_INPUT;
    for (uint64_t j = 0; j < len; ++j) out[op + j] = out[op - off + j];  // (may overlap: a repeated pattern)
    op += len;
  }
  return op == out_bytes ? RPP_OK : RPP_CORRUPT_INPUT;
}

extern "C" int rpp_lz4_host_encode(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t capacity,
                                   uint64_t* out_bytes, uint32_t* bad_ratio) {
  return rpp_lz4_host_encode_search(in, n, 0, out, capacity, out_bytes, bad_ratio);
}

static_assert(RPP_SEARCH_LAZY == rpp_lz4::kSearchLazy, "the search word");

extern "C" int rpp_lz4_host_encode_search(const uint8_t* in, uint64_t n, uint32_t search, uint8_t* out,
                                          uint64_t capacity, uint64_t* out_bytes, uint32_t* bad_ratio) {
  if ((n && !in) || !out || !out_bytes || !search_valid(search)) return RPP_INVALID_ARGUMENT;
  if (n > kMaxBlock) return RPP_INVALID_ARGUMENT;
  if (capacity < rpp_lz4_bound(n)) return RPP_OUTPUT_TOO_SMALL;
  std::vector<Seq> seqs;
  find_sequences(in, uint32_t(n), seqs, search);
  uint8_t* o = out;
  uint32_t anchor = 0;
  for (const Seq& s : seqs) {
    const uint32_t lit = s.pos - anchor, ml = s.len - kMinMatch;
    *o++ = uint8_t(std::min(lit, 15u) << 4 | std::min(ml, 15u));
    if (lit >= 15) o = put_length(o, lit);
    if (lit) std::memcpy(o, in + anchor, lit);
    o += lit;
    *o++ = uint8_t(s.off);
    *o++ = uint8_t(s.off >> 8);
    if (ml >= 15) o = put_length(o, ml);
    anchor = s.pos + s.len;
  }
  const uint32_t lit = uint32_t(n) - anchor;
  *o++ = uint8_t(std::min(lit, 15u) << 4);
  if (lit >= 15) o = put_length(o, lit);
  if (lit) std::memcpy(o, in + anchor, lit);
  o += lit;
  *out_bytes = uint64_t(o - out);
  if (bad_ratio) *bad_ratio = 4 + *out_bytes >= n ? 1u : 0u;  // bad_compression_ratio_error (lz4.cpp:97-99)
  return RPP_OK;
}
