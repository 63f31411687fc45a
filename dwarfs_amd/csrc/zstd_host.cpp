// zstd_host.cpp -- the host side of the Zstandard block decoder: the frame
// header as the reader needs it (src/compression/zstd.cpp:443-483: the content
// size decides the buffer, then one ZSTD_decompress call), a walk over the
// block headers, and the sequential restatement of the three kernels of
// zstd_kernels.hip.  Plain C++: the sanitizer test (tests/cpp/zstd_test.cpp)
// compiles this file alone.  Written from RFC 8878; the pieces both sides use
// (header parsers, bit readers, table builders) are in zstd_common.h.
//
// Decode contract (both the kernels and rpp_zstd_host_decode).  The input is
// ONE Zstandard frame, as ZSTD_compress2 writes a DwarFS block, and the caller
// states the size of its content.  RPP_CORRUPT_INPUT when
//   frame     the magic number is missing (a skippable frame included), the
//             reserved header bit is set, the window log is above 31, a
//             Dictionary_ID is present and not 0, a header field is cut; the
//             Frame_Content_Size is present and differs from the stated size;
//             the flagged Content_Checksum's 4 bytes are missing (they are
//             skipped, not verified); any byte follows the frame; the blocks do
//             not produce exactly the stated size.  A frame without
//             Frame_Content_Size is decoded: the stated size stands in.
//   blocks    a header or a block passes the end; the type is Reserved; a Raw
//             or RLE block, or what a Compressed block produces, is larger
//             than Block_Maximum_Size = min(window, 128 KiB), where a
//             single-segment frame's window is its content size; a Compressed
//             block is below 3 bytes or above Block_Maximum_Size.
//   literals  a header or a section passes the block; a size is above 128 KiB;
//             Compressed or Treeless literals regenerate 0 bytes; Treeless
//             comes without an earlier Compressed literals section in the
//             frame; the tree description is cut, leaves no byte for the
//             streams, holds a weight above 11, more than 255 weights, weights
//             that do not complete a code of at most 11 bits, or fewer than 2
//             or an odd number of longest codes; 4 streams in less than 10
//             bytes, with a jump table that leaves the last one empty, an empty
//             stream, or fewer literals than 3 segments; a stream without its
//             end mark, or not used up exactly by its literals.
//   sequences the header is cut; bytes follow a count of 0; the 2-byte form
//             states a count of 0 (only the single byte 0 says "no sequences";
//             libzstd 1.4.8 reads the tables of such a section and then ignores
//             its bitstream, and no encoder writes one); the reserved mode
//             bits are set; an FSE description has an accuracy log above 9/8/9
//             (LL/OF/ML; 6 for Huffman weights), more symbols than 36/32/53,
//             probabilities that do not add up, or is cut; an RLE symbol is
//             above 35/31/52; Repeat comes without an earlier table in the
//             frame; the bitstream has no end mark, runs out, or is not used up
//             exactly; the literals run out; an offset is 0 (repeat offset 1
//             minus 1), reaches before the output's start, or is beyond the
//             window.
// Three of these libzstd 1.4.8 does not enforce although RFC 8878 states
// them: the reserved mode bits (3.1.1.3.2.1), unused sequence bits
// (3.1.1.3.2.1.1) and the offset 0 (3.1.1.5).  The window and
// Block_Maximum_Size checks on Raw and RLE blocks are the RFC's too (3.1.1.2.3).
// Nothing outside [in, in + in_bytes) is read and nothing outside
// [out, out + out_bytes) is written, whatever the bytes are.  What the blocks
// before the failing one produced stays written; the failing block's output is
// unspecified.
#include <cstring>
#include <vector>

#include "ricepp_amd.h"
#include "zstd_common.h"

namespace {

using namespace rpp_zstd;

struct BlockHeader {
  uint32_t kind, size;
  bool last;
};

// the block header at `at`; false if it or the block passes the end, or the type is Reserved
bool block_header(const uint8_t* in, uint64_t n, uint64_t at, BlockHeader& b) {
  if (at + 3 > n) return false;
  const uint32_t h = uint32_t(rd_le(in + at, 3));
  b.last = h & 1;
  b.kind = h >> 1 & 3;
  b.size = h >> 3;
  if (b.kind == 3) return false;
  return at + 3 + (b.kind == kRle ? 1 : b.size) <= n;
}

struct Tables {  // what one block hands to the next
  std::vector<uint16_t> huf = std::vector<uint16_t>(1u << kHufLog);
  uint32_t huf_log = 0;
  bool has_huf = false;
  std::vector<FseEntry> t[3] = {std::vector<FseEntry>(1u << kTableLog[0]), std::vector<FseEntry>(1u << kTableLog[1]),
                                std::vector<FseEntry>(1u << kTableLog[2])};
  uint32_t log[3] = {0, 0, 0};
  bool has[3] = {false, false, false};
  uint32_t rep[3] = {1, 4, 8};
  std::vector<uint8_t> lits = std::vector<uint8_t>(kBlockMax);
  std::vector<Seq> seqs;
};

bool literals(const uint8_t* body, const LiteralsHeader& lh, Tables& T) {
  const uint8_t* p = body + lh.bytes;
  if (lh.kind == kLitRaw) {
    if (lh.regen) std::memcpy(T.lits.data(), p, lh.regen);
    return true;
  }
  if (lh.kind == kLitRle) {
    std::memset(T.lits.data(), p[0], lh.regen);
    return true;
  }
  uint64_t n = lh.comp;
  if (lh.kind == kLitCompressed) {
    uint8_t weights[kWeightSlots];
    FseEntry wt[1u << kHufWeightLog];
    int16_t freq[kFreqSlots];
    uint16_t next[kFreqSlots];
    uint32_t count;
    const int used = huf_read_weights(p, n, weights, count, wt, freq, next);
    if (used < 0 || !huf_build(weights, count, T.huf.data(), T.huf_log)) return false;
    T.has_huf = true;
    p += used;
    n -= uint64_t(used);
  } else if (!T.has_huf) {
    return false;
  }
  if (lh.streams == 1) return n >= 1 && huf_decode_stream(T.huf.data(), T.huf_log, p, n, T.lits.data(), lh.regen);
  uint32_t at[4], bytes[4], cnt[4], out_at = 0;
  if (!huf_four_streams(p, n, lh.regen, at, bytes, cnt)) return false;
  for (uint32_t i = 0; i < 4; ++i) {
    if (!huf_decode_stream(T.huf.data(), T.huf_log, p + at[i], bytes[i], T.lits.data() + out_at, cnt[i])) return false;
    out_at += cnt[i];
  }
  return true;
}

bool sequences(const uint8_t* p, uint64_t n, const SequencesHeader& sh, Tables& T) {
  uint64_t at = sh.bytes;
  int16_t freq[kFreqSlots];
  uint16_t next[kFreqSlots];
  for (uint32_t k = 0; k < 3; ++k) {
    const uint32_t mode = table_mode(sh.modes, k);
    if (mode == kRepeat) {
      if (!T.has[k]) return false;
      continue;
    }
    if (at > n) return false;
    const int used = table_setup(k, mode, p + at, n - at, T.t[k].data(), T.log[k], freq, next);
    if (used < 0) return false;
    T.has[k] = true;
    at += uint64_t(used);
  }
  if (at >= n) return false;
  T.seqs.resize(sh.count);
  return decode_sequences(p + at, n - at, T.t[0].data(), T.log[0], T.t[1].data(), T.log[1], T.t[2].data(), T.log[2],
                          sh.count, T.seqs.data());
}

}  // namespace

extern "C" long rpp_zstd_frame_info(const uint8_t* data, size_t size, uint64_t* content_size, uint64_t* window,
                                    uint32_t* flags) {
  FrameHeader h;
  if (!data || parse_frame_header(data, size, h) < 0) return RPP_CORRUPT_INPUT;
  if (content_size) *content_size = h.content;
  if (window) *window = h.window;
  if (flags) *flags = h.flags;
  return long(h.bytes);
}

extern "C" long rpp_zstd_count_blocks(const uint8_t* data, size_t size) {
  FrameHeader h;
  if (!data || parse_frame_header(data, size, h) < 0) return RPP_CORRUPT_INPUT;
  uint64_t at = h.bytes;
  long count = 0;
  for (;;) {  // every turn passes at least the 3 bytes of a header
    BlockHeader b;
    if (!block_header(data, size, at, b)) return RPP_CORRUPT_INPUT;
    ++count;
    at += 3 + (b.kind == kRle ? 1 : b.size);
    if (b.last) return count;
  }
}

extern "C" int rpp_zstd_host_decode(const uint8_t* in, uint64_t in_bytes, uint8_t* out, uint64_t out_bytes) {
  if ((in_bytes && !in) || (out_bytes && !out)) return RPP_INVALID_ARGUMENT;
  FrameHeader h;
  if (parse_frame_header(in, in_bytes, h) < 0) return RPP_CORRUPT_INPUT;
  if ((h.flags & kFlagContentSize) && h.content != out_bytes) return RPP_CORRUPT_INPUT;
  const uint64_t window = (h.flags & kFlagSingleSegment) ? out_bytes : h.window;
  const uint64_t block_max = window < kBlockMax ? window : kBlockMax;
  Tables T;
  uint64_t at = h.bytes, op = 0;
  for (;;) {
    BlockHeader b;
    if (!block_header(in, in_bytes, at, b)) return RPP_CORRUPT_INPUT;
    at += 3;
    const uint64_t start = op;
    if (b.kind != kCompressed) {
      if (b.size > block_max || b.size > out_bytes - op) return RPP_CORRUPT_INPUT;
      if (b.kind == kRaw && b.size) std::memcpy(out + op, in + at, b.size);
      if (b.kind == kRle && b.size) std::memset(out + op, in[at], b.size);
      op += b.size;
      at += b.kind == kRle ? 1 : b.size;
    } else {
      if (b.size < 3 || b.size > block_max) return RPP_CORRUPT_INPUT;
      const uint8_t* body = in + at;
      LiteralsHeader lh;
      SequencesHeader sh;
      if (parse_literals_header(body, b.size, lh) < 0) return RPP_CORRUPT_INPUT;
      const uint64_t lit_bytes = uint64_t(lh.bytes) + lh.comp;
      if (parse_sequences_header(body + lit_bytes, b.size - lit_bytes, sh) < 0) return RPP_CORRUPT_INPUT;
      if (!literals(body, lh, T)) return RPP_CORRUPT_INPUT;
      if (sh.count && !sequences(body + lit_bytes, b.size - lit_bytes, sh, T)) return RPP_CORRUPT_INPUT;
      uint32_t lit_at = 0;
      for (uint32_t i = 0; i < sh.count; ++i) {
        const Seq q = T.seqs[i];
        if (q.ll > lh.regen - lit_at) return RPP_CORRUPT_INPUT;
        const uint32_t off = resolve_offset(T.rep, q.ll, q.ov);
        if (uint64_t(q.ll) + q.ml > block_max - (op - start) || uint64_t(q.ll) + q.ml > out_bytes - op)
          return RPP_CORRUPT_INPUT;
        if (q.ll) std::memcpy(out + op, T.lits.data() + lit_at, q.ll);
        lit_at += q.ll;
        op += q.ll;
        if (off == 0 || off > op || off > window) return RPP_CORRUPT_INPUT;
        for (uint32_t j = 0; j < q.ml; ++j) out[op + j] = out[op - off + j];  // (may overlap: a repeated pattern)
        op += q.ml;
      }
      const uint32_t rest = lh.regen - lit_at;
      if (rest > block_max - (op - start) || rest > out_bytes - op) return RPP_CORRUPT_INPUT;
      if (rest) std::memcpy(out + op, T.lits.data() + lit_at, rest);
      op += rest;
      at += b.size;
    }
    if (b.last) break;
  }
  if ((h.flags & kFlagChecksum) && in_bytes - at < 4) return RPP_CORRUPT_INPUT;
  if (at + ((h.flags & kFlagChecksum) ? 4 : 0) != in_bytes) return RPP_CORRUPT_INPUT;
  return op == out_bytes ? RPP_OK : RPP_CORRUPT_INPUT;
}
