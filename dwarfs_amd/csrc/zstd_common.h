// zstd_common.h -- what the Zstandard decode kernels (zstd_kernels.hip) and
// their host restatement (zstd_host.cpp) share: the constants of RFC 8878, the
// header parsers, the two bit readers, and the table builders (FSE, Huffman).
// Every function works on a byte range it is given and never reads outside it;
// every loop is bounded by a size read beforehand.  The contracts are stated at
// the top of zstd_host.cpp.
#ifndef RPP_ZSTD_COMMON_H
#define RPP_ZSTD_COMMON_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RPP_ZSTD_HD __host__ __device__ inline
#else
#define RPP_ZSTD_HD inline
#endif

namespace rpp_zstd {

constexpr uint32_t kMagic = 0xFD2FB528u;
constexpr uint32_t kBlockMax = 128u << 10;  // Block_Maximum_Size is min(window, this)
constexpr uint32_t kMaxWindowLog = 31;
constexpr uint32_t kHufLog = 11;            // the longest Huffman code
constexpr uint32_t kHufWeightLog = 6;       // accuracy log of the FSE-compressed weights, at most
constexpr uint32_t kMaxWeights = 255;       // weights a tree description holds (the last one is deduced)
constexpr uint32_t kWeightSlots = 260;      // room for the turn that finds them too many
constexpr uint32_t kTableLog[3] = {9, 8, 9};       // LL, OF, ML: accuracy log, at most
constexpr uint32_t kTableMaxSymbol[3] = {35, 31, 52};
constexpr uint32_t kFreqSlots = 64;         // probabilities of one description (53 at most)

// rpp_zstd_frame_info's flags
constexpr uint32_t kFlagSingleSegment = 1, kFlagChecksum = 2, kFlagContentSize = 4;

enum BlockKind : uint32_t { kRaw = 0, kRle = 1, kCompressed = 2 };
enum LiteralsKind : uint32_t { kLitRaw = 0, kLitRle = 1, kLitCompressed = 2, kLitTreeless = 3 };
enum TableMode : uint32_t { kPredefined = 0, kModeRle = 1, kFse = 2, kRepeat = 3 };

struct FseEntry {
  uint16_t base;
  uint8_t symbol, bits;
};

struct Seq {  // one sequence as the bitstream states it
  uint32_t ll, ml, ov;  // literal length, match length, offset value (above 3: offset + 3)
};

RPP_ZSTD_HD uint32_t highbit(uint32_t v) { return 31u - uint32_t(__builtin_clz(v)); }  // v != 0

RPP_ZSTD_HD uint64_t rd_le(const uint8_t* p, uint32_t bytes) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < bytes; ++i) v |= uint64_t(p[i]) << (8 * i);
  return v;
}

// ---------------------------------------------------------------------------
// headers
// ---------------------------------------------------------------------------
struct FrameHeader {
  uint32_t bytes, flags;
  uint64_t content, window;  // content is 0 without kFlagContentSize; window is content when single-segment
};

// 0, or -1 for a header that cannot be parsed: no magic (a skippable frame included), the reserved bit, a window
// log above 31, a dictionary id other than 0, or a field behind the end
RPP_ZSTD_HD int parse_frame_header(const uint8_t* p, uint64_t n, FrameHeader& h) {
  if (n < 5 || rd_le(p, 4) != kMagic) return -1;
  const uint32_t fhd = p[4], fcs_flag = fhd >> 6, did_flag = fhd & 3;
  const bool single = fhd & 0x20;
  if (fhd & 0x08) return -1;
  uint64_t at = 5;
  h.window = 0;
  if (!single) {
    if (at >= n) return -1;
    const uint32_t log = 10 + (p[at] >> 3);
    if (log > kMaxWindowLog) return -1;
    h.window = (UINT64_C(1) << log) + ((UINT64_C(1) << log) >> 3) * (p[at] & 7);
    ++at;
  }
  const uint32_t did_bytes = did_flag == 3 ? 4 : did_flag;
  if (at + did_bytes > n || rd_le(p + at, did_bytes) != 0) return -1;
  at += did_bytes;
  const uint32_t fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : 1u << fcs_flag;
  if (at + fcs_bytes > n) return -1;
  h.content = fcs_bytes ? rd_le(p + at, fcs_bytes) + (fcs_bytes == 2 ? 256 : 0) : 0;
  at += fcs_bytes;
  if (single) h.window = h.content;
  h.bytes = uint32_t(at);
  h.flags = (single ? kFlagSingleSegment : 0) | (fhd & 0x04 ? kFlagChecksum : 0) | (fcs_bytes ? kFlagContentSize : 0);
  return 0;
}

struct LiteralsHeader {
  uint32_t kind, bytes, regen, comp, streams;  // bytes: of the header; comp: what follows it in the section
};

// the literals-section header of a block body of n bytes; -1 if it or the section it announces passes the end,
// or a size is out of range
RPP_ZSTD_HD int parse_literals_header(const uint8_t* p, uint64_t n, LiteralsHeader& h) {
  if (n < 1) return -1;
  h.kind = p[0] & 3;
  const uint32_t sf = p[0] >> 2 & 3;
  if (h.kind < kLitCompressed) {
    h.bytes = sf == 1 ? 2 : sf == 3 ? 3 : 1;
    if (n < h.bytes) return -1;
    const uint32_t v = uint32_t(rd_le(p, h.bytes));
    h.regen = h.bytes == 1 ? v >> 3 : v >> 4;
    h.streams = 0;
    h.comp = h.kind == kLitRaw ? h.regen : 1;
    if (h.regen > kBlockMax) return -1;
  } else {
    h.bytes = sf < 2 ? 3 : sf + 2;
    if (n < h.bytes) return -1;
    const uint64_t v = rd_le(p, h.bytes) >> 4;
    const uint32_t nb = sf < 2 ? 10 : sf == 2 ? 14 : 18;
    h.regen = uint32_t(v & ((1u << nb) - 1));
    h.comp = uint32_t(v >> nb & ((1u << nb) - 1));
    h.streams = sf == 0 ? 1 : 4;
    if (h.regen > kBlockMax || h.regen == 0) return -1;
  }
  return uint64_t(h.bytes) + h.comp > n ? -1 : 0;
}

struct SequencesHeader {
  uint32_t count, bytes, modes;  // bytes: the count and, where count > 0, the modes byte
};

// the sequences-section header of a section of n bytes; -1 if cut, if bytes follow a count of 0, if the 2-byte
// form states a count of 0, if the reserved mode bits are set, or if no byte is left for the bitstream
RPP_ZSTD_HD int parse_sequences_header(const uint8_t* p, uint64_t n, SequencesHeader& h) {
  if (n < 1) return -1;
  h.modes = 0;
  if (p[0] == 0) {
    h.count = 0;
    h.bytes = 1;
    return n == 1 ? 0 : -1;
  }
  if (p[0] < 128) {
    h.count = p[0];
    h.bytes = 1;
  } else if (p[0] < 255) {
    if (n < 2) return -1;
    h.count = ((uint32_t(p[0]) - 128) << 8) + p[1];
    h.bytes = 2;
    if (h.count == 0) return -1;  // only the single byte 0 says "no sequences"
  } else {
    if (n < 3) return -1;
    h.count = uint32_t(p[1]) + (uint32_t(p[2]) << 8) + 0x7F00;
    h.bytes = 3;
  }
  if (h.bytes >= n) return -1;
  h.modes = p[h.bytes++];
  if (h.modes & 3) return -1;
  return h.bytes >= n ? -1 : 0;
}

RPP_ZSTD_HD uint32_t table_mode(uint32_t modes, uint32_t k) { return modes >> (6 - 2 * k) & 3; }

// ---------------------------------------------------------------------------
// bit readers
// ---------------------------------------------------------------------------
struct ForwardBits {  // from the first byte on, lowest bit first; zeros behind the end
  const uint8_t* p;
  uint64_t n, pos;
  RPP_ZSTD_HD uint32_t read(uint32_t bits) {  // bits <= 16
    uint32_t v = 0;
    const uint64_t byte = pos >> 3;
    for (uint32_t i = 0; i < 3; ++i)
      if (byte + i < n) v |= uint32_t(p[byte + i]) << (8 * i);
    v = v >> (pos & 7) & ((1u << bits) - 1);
    pos += bits;
    return v;
  }
};

// From the last byte on, highest bit first, below the end mark.  `pos` is the number of bits left; it goes
// negative when more is read than the stream holds, and zeros are supplied.  64 bits of the stream are kept.
struct BackwardBits {
  const uint8_t* p;
  int64_t n, pos, base;
  uint64_t held;  // the stream's bits [base, base + 64)

  RPP_ZSTD_HD bool init(const uint8_t* data, uint64_t size) {
    if (size == 0 || data[size - 1] == 0) return false;
    p = data;
    n = int64_t(size);
    pos = 8 * (n - 1) + int64_t(highbit(data[size - 1]));
    base = INT64_MAX / 2;
    held = 0;
    return true;
  }
  RPP_ZSTD_HD void refill() {
    base = ((pos + 7) >> 3) * 8 - 64;
    const int64_t byte = base >> 3;
    if (byte >= 0 && byte + 8 <= n) {
      __builtin_memcpy(&held, p + byte, 8);
    } else {
      held = 0;
      for (int64_t i = 0; i < 8; ++i)
        if (byte + i >= 0 && byte + i < n) held |= uint64_t(p[byte + i]) << (8 * i);
    }
  }
  RPP_ZSTD_HD uint32_t peek(uint32_t bits) {  // bits <= 32
    if (bits == 0) return 0;  // (also keeps the shift below under 64 when pos is a multiple of 8)
    const int64_t lo = pos - int64_t(bits);
    if (lo < base || pos > base + 64) refill();
    return uint32_t(held >> (lo - base)) & uint32_t((UINT64_C(1) << bits) - 1);
  }
  RPP_ZSTD_HD uint32_t read(uint32_t bits) {
    const uint32_t v = peek(bits);
    pos -= int64_t(bits);
    return v;
  }
};

// ---------------------------------------------------------------------------
// FSE
// ---------------------------------------------------------------------------
// Reads a table description (RFC 8878 4.1.1) into freq[kFreqSlots]; the bytes it takes, or -1.
RPP_ZSTD_HD int fse_read_description(const uint8_t* p, uint64_t n, uint32_t max_log, uint32_t max_symbol, int16_t* freq,
                                     uint32_t& nsym, uint32_t& log) {
  if (n == 0) return -1;
  ForwardBits r{p, n, 0};
  log = 5 + r.read(4);
  if (log > max_log) return -1;
  int32_t remaining = 1 << log;
  nsym = 0;
  while (remaining > 0 && nsym <= max_symbol) {  // one symbol per turn
    const uint32_t nbits = highbit(uint32_t(remaining) + 1) + 1;
    uint32_t val = r.read(nbits);
    const uint32_t lower = (1u << (nbits - 1)) - 1, threshold = (1u << nbits) - 1 - (uint32_t(remaining) + 1);
    if ((val & lower) < threshold) {
      r.pos -= 1;
      val &= lower;
    } else if (val > lower) {
      val -= threshold;
    }
    const int32_t prob = int32_t(val) - 1;
    remaining -= prob < 0 ? 1 : prob;
    freq[nsym++] = int16_t(prob);
    if (prob == 0)
      for (;;) {  // two bits per turn; behind the end they are zeros
        const uint32_t rep = r.read(2);
        if (nsym + rep > max_symbol + 1) return -1;
        for (uint32_t k = 0; k < rep; ++k) freq[nsym++] = 0;
        if (rep != 3) break;
      }
  }
  if (remaining != 0 || nsym > max_symbol + 1) return -1;
  const uint64_t used = (r.pos + 7) >> 3;
  return used > n ? -1 : int(used);
}

// The decoding table of a distribution (RFC 8878 4.1.1); next[nsym] is scratch.
RPP_ZSTD_HD bool fse_build(const int16_t* freq, uint32_t nsym, uint32_t log, FseEntry* t, uint16_t* next) {
  const uint32_t size = 1u << log;
  uint32_t high = size;
  for (uint32_t s = 0; s < nsym; ++s) {
    next[s] = 0;
    if (freq[s] == -1) {
      t[--high].symbol = uint8_t(s);
      next[s] = 1;
    }
  }
  const uint32_t step = (size >> 1) + (size >> 3) + 3;
  uint32_t pos = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    if (freq[s] <= 0) continue;
    next[s] = uint16_t(freq[s]);
    for (int32_t i = 0; i < freq[s]; ++i) {
      t[pos].symbol = uint8_t(s);
      do pos = (pos + step) & (size - 1);
      while (pos >= high);  // (the cells below `high` are as many as the probabilities above 0 add up to)
    }
  }
  if (pos != 0) return false;
  for (uint32_t i = 0; i < size; ++i) {
    const uint32_t d = next[t[i].symbol]++;
    t[i].bits = uint8_t(log - highbit(d));
    t[i].base = uint16_t((d << t[i].bits) - size);
  }
  return true;
}

RPP_ZSTD_HD void predefined(uint32_t k, int16_t* freq, uint32_t& nsym, uint32_t& log) {
  const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
                         -1, -1, -1, -1};
  const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                         1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  nsym = k == 0 ? 36 : k == 1 ? 29 : 53;
  log = k == 1 ? 5 : 6;
  for (uint32_t s = 0; s < nsym; ++s) freq[s] = k == 0 ? ll[s] : k == 1 ? of[s] : ml[s];
}

// Table k (0 LL, 1 OF, 2 ML) in `mode` (not kRepeat) from the bytes at p; the bytes it takes, or -1.
RPP_ZSTD_HD int table_setup(uint32_t k, uint32_t mode, const uint8_t* p, uint64_t n, FseEntry* t, uint32_t& log,
                            int16_t* freq, uint16_t* next) {
  uint32_t nsym;
  int used = 0;
  if (mode == kModeRle) {
    if (n < 1 || p[0] > kTableMaxSymbol[k]) return -1;
    t[0] = FseEntry{0, p[0], 0};
    log = 0;
    return 1;
  }
  if (mode == kPredefined) {
    predefined(k, freq, nsym, log);
  } else {
    used = fse_read_description(p, n, kTableLog[k], kTableMaxSymbol[k], freq, nsym, log);
    if (used < 0) return -1;
  }
  return fse_build(freq, nsym, log, t, next) ? used : -1;
}

// Where table k's description starts behind the modes byte of a sequences section (p, n: what follows that
// byte): the descriptions before it are stepped over.  -1 if one of them cannot be read.
RPP_ZSTD_HD int64_t table_position(uint32_t modes, uint32_t k, const uint8_t* p, uint64_t n, int16_t* freq) {
  uint64_t at = 0;
  for (uint32_t j = 0; j < k; ++j) {
    const uint32_t mode = table_mode(modes, j);
    if (mode == kModeRle) {
      at += 1;
    } else if (mode == kFse) {
      uint32_t nsym, log;
      if (at > n) return -1;
      const int used = fse_read_description(p + at, n - at, kTableLog[j], kTableMaxSymbol[j], freq, nsym, log);
      if (used < 0) return -1;
      at += uint64_t(used);
    }
    if (at > n) return -1;
  }
  return int64_t(at);
}

RPP_ZSTD_HD void ll_code(uint32_t c, uint32_t& base, uint32_t& bits) {  // c <= 35
  const uint8_t b[10] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 6};
  const uint8_t v[10] = {16, 18, 20, 22, 24, 28, 32, 40, 48, 64};
  if (c < 16) {
    base = c;
    bits = 0;
  } else if (c < 26) {
    base = v[c - 16];
    bits = b[c - 16];
  } else {
    base = 1u << (c - 19);
    bits = c - 19;
  }
}

RPP_ZSTD_HD void ml_code(uint32_t c, uint32_t& base, uint32_t& bits) {  // c <= 52
  const uint8_t b[11] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5};
  const uint8_t v[11] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99};
  if (c < 32) {
    base = c + 3;
    bits = 0;
  } else if (c < 43) {
    base = v[c - 32];
    bits = b[c - 32];
  } else {
    base = (1u << (c - 36)) + 3;
    bits = c - 36;
  }
}

// The `count` sequences of a bitstream (RFC 8878 3.1.1.3.2.1.1) with the three tables; false if the stream has
// no end mark, runs out, or is not used up exactly.
RPP_ZSTD_HD bool decode_sequences(const uint8_t* p, uint64_t n, const FseEntry* llt, uint32_t ll_log, const FseEntry* oft,
                                  uint32_t of_log, const FseEntry* mlt, uint32_t ml_log, uint32_t count, Seq* out) {
  BackwardBits b;
  if (!b.init(p, n)) return false;
  uint32_t ll_s = b.read(ll_log), of_s = b.read(of_log), ml_s = b.read(ml_log);
  for (uint32_t i = 0; i < count; ++i) {
    const FseEntry le = llt[ll_s], oe = oft[of_s], me = mlt[ml_s];
    uint32_t base, bits;
    Seq q;
    q.ov = (1u << oe.symbol) + b.read(oe.symbol);  // (a code is at most 31)
    ml_code(me.symbol, base, bits);
    q.ml = base + b.read(bits);
    ll_code(le.symbol, base, bits);
    q.ll = base + b.read(bits);
    out[i] = q;
    if (i + 1 < count) {
      ll_s = le.base + b.read(le.bits);
      ml_s = me.base + b.read(me.bits);
      of_s = oe.base + b.read(oe.bits);
    }
    if (b.pos < 0) return false;
  }
  return b.pos == 0;
}

// ---------------------------------------------------------------------------
// Huffman
// ---------------------------------------------------------------------------
// The weights of a tree description (RFC 8878 4.2.1) without the deduced last one, into weights[kWeightSlots];
// the bytes it takes, or -1.  t[1 << kHufWeightLog], freq[kFreqSlots] and next[kFreqSlots] are scratch.
RPP_ZSTD_HD int huf_read_weights(const uint8_t* p, uint64_t n, uint8_t* weights, uint32_t& count, FseEntry* t,
                                 int16_t* freq, uint16_t* next) {
  if (n < 1) return -1;
  const uint32_t head = p[0];
  if (head >= 128) {
    count = head - 127;
    const uint32_t used = 1 + (count + 1) / 2;
    if (used > n) return -1;
    for (uint32_t i = 0; i < count; ++i) weights[i] = i & 1 ? p[1 + i / 2] & 15 : p[1 + i / 2] >> 4;
    return int(used);
  }
  if (head == 0 || 1 + uint64_t(head) > n) return -1;
  uint32_t nsym, log;
  const int used = fse_read_description(p + 1, head, kHufWeightLog, 12, freq, nsym, log);
  if (used < 0 || uint32_t(used) >= head || !fse_build(freq, nsym, log, t, next)) return -1;
  BackwardBits b;
  if (!b.init(p + 1 + used, head - uint32_t(used))) return -1;
  uint32_t s1 = b.read(log), s2 = b.read(log);
  if (b.pos < 0) return -1;
  count = 0;
  // two states take turns; the stream ends where the state whose turn it is cannot be refilled
  for (;;) {  // up to three weights per turn
    if (count > kMaxWeights) return -1;
    weights[count++] = t[s1].symbol;
    if (b.pos < int64_t(t[s1].bits)) {
      weights[count++] = t[s2].symbol;
      break;
    }
    s1 = t[s1].base + b.read(t[s1].bits);
    weights[count++] = t[s2].symbol;
    if (b.pos < int64_t(t[s2].bits)) {
      weights[count++] = t[s1].symbol;
      break;
    }
    s2 = t[s2].base + b.read(t[s2].bits);
  }
  return count > kMaxWeights ? -1 : 1 + int(head);
}

// The decoding table (1 << log entries of symbol | bits << 8) of `count` weights plus the deduced one; false
// for weights that are no complete code of at most kHufLog bits with an even number, at least 2, of longest codes.
RPP_ZSTD_HD bool huf_build(const uint8_t* weights, uint32_t count, uint16_t* table, uint32_t& log) {
  uint32_t total = 0, rank[kHufLog + 2] = {};
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t w = weights[i];
    if (w > kHufLog) return false;
    if (w) total += 1u << (w - 1);
    ++rank[w];
  }
  if (total == 0) return false;
  log = highbit(total) + 1;
  if (log > kHufLog) return false;
  const uint32_t rest = (1u << log) - total;
  if (rest & (rest - 1)) return false;
  const uint32_t last = highbit(rest) + 1;
  ++rank[last];
  if (rank[1] < 2 || (rank[1] & 1)) return false;
  uint32_t start[kHufLog + 2], at = 0;
  for (uint32_t w = 1; w <= log; ++w) {
    start[w] = at;
    at += rank[w] << (w - 1);
  }
  for (uint32_t s = 0; s <= count; ++s) {
    const uint32_t w = s < count ? weights[s] : last;
    if (!w) continue;
    const uint32_t len = 1u << (w - 1), e = s | (log + 1 - w) << 8;
    for (uint32_t i = 0; i < len; ++i) table[start[w] + i] = uint16_t(e);
    start[w] += len;
  }
  return true;
}

// `count` literals of one Huffman stream; false if it has no end mark or is not used up exactly.
RPP_ZSTD_HD bool huf_decode_stream(const uint16_t* table, uint32_t log, const uint8_t* p, uint64_t n, uint8_t* out,
                                   uint32_t count) {
  BackwardBits b;
  if (!b.init(p, n)) return false;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t e = table[b.peek(log)];
    out[i] = uint8_t(e);
    b.pos -= int64_t(e >> 8);
  }
  return b.pos == 0;
}

// The four streams behind a jump table (body: n bytes): where stream i starts, its bytes and its literals;
// false for a body below 10 bytes, a jump table that passes it, an empty stream, or fewer literals than three
// segments hold.
RPP_ZSTD_HD bool huf_four_streams(const uint8_t* body, uint64_t n, uint32_t regen, uint32_t at[4], uint32_t bytes[4],
                                  uint32_t lits[4]) {
  if (n < 10) return false;
  const uint32_t seg = (regen + 3) / 4;
  if (3 * seg > regen) return false;
  uint64_t sum = 6;
  for (uint32_t i = 0; i < 3; ++i) {
    at[i] = uint32_t(sum);
    bytes[i] = uint32_t(rd_le(body + 2 * i, 2));
    lits[i] = seg;
    sum += bytes[i];
  }
  if (sum >= n) return false;
  at[3] = uint32_t(sum);
  bytes[3] = uint32_t(n - sum);
  lits[3] = regen - 3 * seg;
  return bytes[0] && bytes[1] && bytes[2];
}

// The match offset of a sequence and the new repeat-offset history (RFC 8878 3.1.1.5); 0 for the offset 0 that
// "repeat offset 1 minus 1" can give.
RPP_ZSTD_HD uint32_t resolve_offset(uint32_t rep[3], uint32_t ll, uint32_t ov) {
  if (ov > 3) {
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = ov - 3;
    return rep[0];
  }
  const uint32_t idx = ov + (ll == 0 ? 1 : 0);
  if (idx == 1) return rep[0];
  const uint32_t off = idx == 4 ? rep[0] - 1 : rep[idx - 1];
  if (off == 0) return 0;
  if (idx != 2) rep[2] = rep[1];
  rep[1] = rep[0];
  rep[0] = off;
  return off;
}

}  // namespace rpp_zstd

#endif  // RPP_ZSTD_COMMON_H
