// zstd_long_host.cpp -- the long-distance matcher of the Zstandard encoder on
// the host: the sequential restatement of the kernels of zstd_long.hip, which
// find the same matches, and rpp_zstd_host_encode_long, which writes the bytes
// of rpp_zstd_encode_batch_long.  Plain C++: the sanitizer test
// (tests/cpp/zstd_long_test.cpp) compiles this file with lz4_host.cpp,
// zstd_encode_host.cpp and zstd_host.cpp.  The constants and the hash are in
// zstd_long_common.h; this is the whole definition.
//
// The `long` word (rpp_zstd_host_encode_long, rpp_zstd_encode_batch_long): 0 is
// the encoder of zstd_encode_host.cpp, byte for byte, for every options and
// search word; 1 adds matches against anything earlier in the same block; any
// other value is an invalid argument.  With 1 a block holds at most
// kLongMaxBlock = 2^27 bytes; a larger one has the status of an over-size block.
// The mirror of the reference's `long` option (src/compression/zstd.cpp:69,
// :404-406: libzstd's long-distance matcher with the window set to the block).
// The result depends on the block's bytes alone.
//   index   one table per block of 2^long_table_log(n) entries.  For every q
//           that is a multiple of kLongGrid with q + kLongWindow <= n, the entry
//           long_slot(long_hash(in[q .. q + kLongWindow))) holds the LOWEST such
//           q (a minimum, so no order between the inserts matters); an entry
//           nothing maps to holds kLongEmpty.
//   find    per chunk of kChunk bytes, with lim_end = min(chunk end, n - 5) as
//           in the short search and a cursor that starts at the chunk's start:
//           a position p with p + kLongWindow <= lim_end has a candidate q when
//           its window's entry holds some q < p and the kLongWindow bytes at q
//           and p are equal.  The match is extended forward over the common
//           prefix, cut at lim_end, and backward while p - 1 >= cursor, q >= 1
//           and in[q - 1] == in[p - 1].  It is kept when it has at least
//           kLongMinMatch bytes.  Greedy: the first position at or behind the
//           cursor with a kept match is taken (a candidate that is not kept
//           changes nothing), and the cursor moves to the match's end.  A long
//           match never crosses a chunk's end; its source may lie anywhere
//           earlier in the block, in the same chunk too, and may overlap it.
//           A chunk has at most kLongPerChunk long matches.
//   merge   the short search (any search word) runs unchanged over the whole
//           chunk.  The chunk's final list, in position order: every long
//           match; every short match that overlaps no long match; and of a
//           short match [a, b) that overlaps one, with F the first and L the
//           last long match that overlaps it: its head [a, F.start) and its
//           tail [L.end, b), each with the short match's offset and only when
//           it has at least kMinMatch bytes.  (What lies between two long
//           matches inside one short match becomes literals.)
// Matches do not overlap and have at least 4 bytes, so kSeqsPerChunk bounds the
// list, and everything behind the list is the encoder's as it stands:
// offset_value, plan_table, the block rule, rpp_zstd_bound and the ratio flag.
// An offset's code reaches 27 where it stayed below 16 without the word.
// Limits: the first occurrence of a window is the source, not the nearest one,
// so offsets are larger than they need be; two different windows that share a
// table entry hide the later one; no match crosses a chunk's end (a far copy is
// one match per chunk).
#include <algorithm>
#include <cstring>
#include <vector>

#include "lz4_internal.h"
#include "ricepp_amd.h"
#include "zstd_enc_common.h"
#include "zstd_long_common.h"
#include "zstd_long_internal.h"

namespace {

using namespace rpp_zstd_long;
using rpp_lz4::kChunk;
using rpp_lz4::Seq;

inline uint32_t window_slot(const uint8_t* p, uint32_t log) {
  uint32_t w[kLongWindow / 4];
  for (uint32_t k = 0; k < kLongWindow / 4; ++k)
    w[k] = uint32_t(p[4 * k]) | uint32_t(p[4 * k + 1]) << 8 | uint32_t(p[4 * k + 2]) << 16 | uint32_t(p[4 * k + 3]) << 24;
  return long_slot(long_hash(w), log);
}

}  // namespace

void rpp_zstd_long::find_long(const uint8_t* in, uint32_t n, std::vector<Seq>& longs) {
  if (n < kLongMinMatch + rpp_lz4::kLastLiterals) return;
  const uint32_t log = long_table_log(n), match_end = n - rpp_lz4::kLastLiterals;
  std::vector<uint32_t> tab(size_t(1) << log, kLongEmpty);
  for (uint32_t q = 0; q + kLongWindow <= n; q += kLongGrid) {
    uint32_t& e = tab[window_slot(in + q, log)];
    e = std::min(e, q);
  }
  for (uint32_t cs = 0; cs < n; cs += kChunk) {
    const uint32_t ce = uint32_t(std::min<uint64_t>(uint64_t(cs) + kChunk, n)), lim_end = std::min(ce, match_end);
    uint32_t cursor = cs;
    for (uint32_t p = cs; p + kLongWindow <= lim_end; ++p) {
      const uint32_t q = tab[window_slot(in + p, log)];
      if (q == kLongEmpty || q >= p || std::memcmp(in + q, in + p, kLongWindow) != 0) continue;
      uint32_t fwd = kLongWindow, back = 0;
      while (p + fwd < lim_end && in[q + fwd] == in[p + fwd]) ++fwd;
      while (p - back > cursor && q - back >= 1 && in[q - back - 1] == in[p - back - 1]) ++back;
      if (fwd + back < kLongMinMatch) continue;
      longs.push_back({p - back, fwd + back, p - q});
      cursor = p + fwd;
      p = cursor - 1;
    }
  }
}

void rpp_zstd_long::merge(const std::vector<Seq>& shorts, const std::vector<Seq>& longs, std::vector<Seq>& out) {
  size_t j = 0;  // the first long match that ends behind the short match's start
  for (const Seq& s : shorts) {
    const uint32_t a = s.pos, b = s.pos + s.len;
    for (; j < longs.size() && longs[j].pos + longs[j].len <= a; ++j) out.push_back(longs[j]);
    if (j == longs.size() || longs[j].pos >= b) {
      out.push_back(s);
      continue;
    }
    if (longs[j].pos >= a + rpp_lz4::kMinMatch) out.push_back({a, longs[j].pos - a, s.off});
    size_t l = j;  // the last long match that starts before the short match's end
    while (l + 1 < longs.size() && longs[l + 1].pos < b) ++l;
    for (; j < l; ++j) out.push_back(longs[j]);
    const uint32_t le = longs[l].pos + longs[l].len;
    if (le + rpp_lz4::kMinMatch <= b) {  // (then the next short match starts behind it: j moves past it there)
      out.push_back(longs[l]);
      ++j;
      out.push_back({le, b - le, s.off});
    }
  }
  for (; j < longs.size(); ++j) out.push_back(longs[j]);
}

void rpp_zstd_long::sequences(const uint8_t* in, uint32_t n, uint32_t search, uint32_t long_mode,
                              std::vector<Seq>& out) {
  if (!long_mode) return rpp_lz4::find_sequences(in, n, out, search);
  std::vector<Seq> shorts, longs;
  rpp_lz4::find_sequences(in, n, shorts, search);
  find_long(in, n, longs);
  merge(shorts, longs, out);
}

extern "C" int rpp_zstd_host_encode_long(const uint8_t* in, uint64_t n, uint32_t options, uint32_t search,
                                         uint32_t long_mode, uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                                         uint32_t* bad_ratio) {
  if (long_mode > 1) return RPP_INVALID_ARGUMENT;
  if (!long_mode) return rpp_zstd_host_encode_search(in, n, options, search, out, capacity, out_bytes, bad_ratio);
  if ((n && !in) || !out || !out_bytes || (options & ~rpp_zstd::kEncOptionsMask) || !rpp_lz4::search_valid(search))
    return RPP_INVALID_ARGUMENT;
  if (n > kLongMaxBlock) return RPP_INVALID_ARGUMENT;
  if (capacity < rpp_zstd::encode_bound(n)) return RPP_OUTPUT_TOO_SMALL;
  std::vector<Seq> seqs;
  sequences(in, uint32_t(n), search, 1, seqs);
  rpp_zstd::write_frame(in, uint32_t(n), options, seqs, out, out_bytes, bad_ratio);
  return RPP_OK;
}

extern "C" int rpp_zstd_host_long_sequences(const uint8_t* in, uint64_t n, uint32_t search, uint32_t long_mode,
                                            uint32_t* triples, uint64_t capacity, uint64_t* count) {
  if ((n && !in) || !count || long_mode > 1 || !rpp_lz4::search_valid(search)) return RPP_INVALID_ARGUMENT;
  if (n > (long_mode ? kLongMaxBlock : rpp_lz4::kMaxBlock)) return RPP_INVALID_ARGUMENT;
  std::vector<Seq> seqs;
  sequences(in, uint32_t(n), search, long_mode, seqs);
  *count = seqs.size();
  if (capacity < seqs.size()) return RPP_OUTPUT_TOO_SMALL;
  for (size_t i = 0; i < seqs.size() && triples; ++i) {
    triples[3 * i] = seqs[i].pos;
    triples[3 * i + 1] = seqs[i].len;
    triples[3 * i + 2] = seqs[i].off;
  }
  return RPP_OK;
}
