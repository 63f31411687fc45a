// zstd_enc_common.h -- every rule that the Zstandard encode kernels
// (zstd_encode.hip) and their host restatement (zstd_encode_host.cpp) share, so
// that the two write the same bytes: the frame, block and section headers, the
// Huffman code lengths and the tree description, the FSE encoding tables, the
// codes of a sequence, and, for the options word, the repeat-offset rule and
// the choice of a block's table modes.  The format they add up to is defined at the top of
// zstd_encode_host.cpp.  Plain C++, no HIP; sequential functions that a single
// lane may run on the device.
#ifndef RPP_ZSTD_ENC_COMMON_H
#define RPP_ZSTD_ENC_COMMON_H

#include "lz4_common.h"
#include "zstd_common.h"

namespace rpp_zstd {

constexpr uint32_t kEncChunk = rpp_lz4::kChunk;  // one block per search chunk
constexpr uint32_t kOneStreamMax = 1023;         // literals of a block that go into 1 Huffman stream
constexpr uint32_t kDirectMax = 128;             // weights the direct tree description can list
constexpr uint32_t kTreeSlots = 320;             // bytes a tree description is built in (kept: below 129)
constexpr uint32_t kSeqInitBits = 6 + 5 + 6;     // the three predefined tables' first states
constexpr uint32_t kEncTables = 1, kEncRepeat = 2;  // the options word (RPP_ZSTD_ENC_TABLES, RPP_ZSTD_ENC_REPEAT)
constexpr uint32_t kEncOptionsMask = kEncTables | kEncRepeat;
constexpr uint32_t kOwnLogMax = 6;               // accuracy log of a block's own table, at most: a move of a state
                                                 // is val | nb << 6 in 9 bits, and the tables stay 64 cells
constexpr uint32_t kDescSlots = 72;              // bytes a table description is built in (at most 54 are kept)
static_assert(kEncChunk <= kBlockMax, "a chunk is one block");

RPP_ZSTD_HD uint32_t chunks_of(uint64_t n) { return uint32_t((n + kEncChunk - 1) / kEncChunk); }
RPP_ZSTD_HD uint64_t encode_bound(uint64_t n) { return n + 3 * (n / kEncChunk + 1) + 9; }

// ---------------------------------------------------------------------------
// headers
// ---------------------------------------------------------------------------
// magic, single-segment descriptor, Frame_Content_Size in 1, 2 or 4 bytes (n < 2^32): 6, 7 or 9 bytes
RPP_ZSTD_HD uint32_t frame_header(uint64_t n, uint8_t* out) {
  const uint32_t flag = n < 256 ? 0 : n < 65536 + 256 ? 1 : 2, fcs = flag == 0 ? 1 : 2 * flag;
  const uint32_t v = uint32_t(flag == 1 ? n - 256 : n);
  for (uint32_t i = 0; i < 4; ++i) out[i] = uint8_t(kMagic >> (8 * i));
  out[4] = uint8_t(flag << 6 | 0x20);
  for (uint32_t i = 0; i < fcs; ++i) out[5 + i] = uint8_t(v >> (8 * i));
  return 5 + fcs;
}

RPP_ZSTD_HD void block_header(uint8_t* out, bool last, uint32_t kind, uint32_t size) {
  const uint32_t v = (last ? 1u : 0u) | kind << 1 | size << 3;
  out[0] = uint8_t(v);
  out[1] = uint8_t(v >> 8);
  out[2] = uint8_t(v >> 16);
}

RPP_ZSTD_HD uint32_t plain_literals_header_bytes(uint32_t m) { return m < 32 ? 1 : m < 4096 ? 2 : 3; }

// the header of Raw or RLE literals in its narrowest width
RPP_ZSTD_HD uint32_t plain_literals_header(uint32_t kind, uint32_t m, uint8_t* out) {
  const uint32_t bytes = plain_literals_header_bytes(m);
  const uint32_t v = bytes == 1 ? kind | m << 3 : kind | (bytes == 2 ? 1u : 3u) << 2 | m << 4;
  for (uint32_t i = 0; i < bytes; ++i) out[i] = uint8_t(v >> (8 * i));
  return bytes;
}

// Size format of Huffman literals: 0 for one stream; for four the narrowest of 1, 2, 3 that holds both sizes.
RPP_ZSTD_HD uint32_t literals_size_format(uint32_t streams, uint32_t regen, uint32_t comp) {
  if (streams == 1) return 0;
  const uint32_t top = regen > comp ? regen : comp;
  return top < 1024 ? 1 : top < 16384 ? 2 : 3;
}

RPP_ZSTD_HD uint32_t huf_literals_header_bytes(uint32_t sf) { return sf < 2 ? 3 : sf + 2; }

RPP_ZSTD_HD uint32_t huf_literals_header(uint32_t sf, uint32_t regen, uint32_t comp, uint8_t* out) {
  const uint32_t nb = sf < 2 ? 10 : sf == 2 ? 14 : 18, bytes = huf_literals_header_bytes(sf);
  const uint32_t lo = uint32_t(kLitCompressed) | sf << 2 | regen << 4 | comp << (4 + nb);  // (its low 32 bits)
  for (uint32_t i = 0; i < 4 && i < bytes; ++i) out[i] = uint8_t(lo >> (8 * i));
  if (bytes == 5) out[4] = uint8_t(comp >> 10);
  return bytes;
}

// Number_of_Sequences in 1 or 2 bytes (count < 0x7F00); out may be null
RPP_ZSTD_HD uint32_t sequence_count_bytes(uint32_t count, uint8_t* out) {
  if (count < 128) {
    if (out) out[0] = uint8_t(count);
    return 1;
  }
  if (out) {
    out[0] = uint8_t((count >> 8) + 128);
    out[1] = uint8_t(count);
  }
  return 2;
}

// `nb` <= 16 bits of v at bit `pos` of a zeroed byte range (lowest bit first)
RPP_ZSTD_HD void put_bits(uint8_t* p, uint32_t pos, uint32_t v, uint32_t nb) {
  if (nb == 0) return;
  const uint32_t w = (v & ((1u << nb) - 1)) << (pos & 7);
  p += pos >> 3;
  p[0] |= uint8_t(w);
  if ((pos & 7) + nb > 8) p[1] |= uint8_t(w >> 8);
  if ((pos & 7) + nb > 16) p[2] |= uint8_t(w >> 16);
}

// ---------------------------------------------------------------------------
// Huffman
// ---------------------------------------------------------------------------
// The code lengths of a histogram of `total` literals with at least two distinct bytes; the longest length.
//   1. a byte seen c times gets the smallest length l >= 1 with c * 2^l >= total, at most kHufLog;
//   2. with K = the sum of 2^(kHufLog - l): while K > 2^kHufLog, passes over the lengths kHufLog - 1 down to 1
//      lengthen, in order of byte value, every byte of that length by one while K is still too large;
//   3. while K < 2^kHufLog, passes over the lengths 2 up to kHufLog shorten, in order of byte value, every byte
//      of that length by one whose gain 2^(kHufLog - l) still fits the gap.
// K is a multiple of the longest code's unit, so step 3 ends with a complete code.
RPP_ZSTD_HD uint32_t huf_lengths(const uint32_t* hist, uint32_t total, uint8_t* len) {
  const uint32_t full = 1u << kHufLog;
  uint32_t K = 0;
  for (uint32_t s = 0; s < 256; ++s) {
    uint32_t l = 0;
    if (hist[s]) {
      l = 1;
      while (l < kHufLog && (hist[s] << l) < total) ++l;
      K += 1u << (kHufLog - l);
    }
    len[s] = uint8_t(l);
  }
  while (K > full)
    for (uint32_t l = kHufLog - 1; l >= 1 && K > full; --l)
      for (uint32_t s = 0; s < 256 && K > full; ++s)
        if (len[s] == l) {
          len[s] = uint8_t(l + 1);
          K -= 1u << (kHufLog - 1 - l);
        }
  while (K < full)
    for (uint32_t l = 2; l <= kHufLog && K < full; ++l)
      for (uint32_t s = 0; s < 256 && K < full; ++s)
        if (len[s] == l && (1u << (kHufLog - l)) <= full - K) {
          len[s] = uint8_t(l - 1);
          K += 1u << (kHufLog - l);
        }
  uint32_t longest = 0;
  for (uint32_t s = 0; s < 256; ++s) longest = len[s] > longest ? len[s] : longest;
  return longest;
}

// code | length << 16 of every byte: the canonical code huf_build reads (weight = longest + 1 - length; the
// longest codes first, bytes of one length in order of value)
RPP_ZSTD_HD void huf_codes(const uint8_t* len, uint32_t longest, uint32_t* ctab) {
  uint32_t rank[kHufLog + 2] = {}, next[kHufLog + 2] = {};
  for (uint32_t s = 0; s < 256; ++s)
    if (len[s]) ++rank[longest + 1 - len[s]];
  for (uint32_t w = 1, at = 0; w <= longest; ++w) {
    next[w] = at >> (w - 1);
    at += rank[w] << (w - 1);
  }
  for (uint32_t s = 0; s < 256; ++s) ctab[s] = len[s] ? next[longest + 1 - len[s]]++ | uint32_t(len[s]) << 16 : 0;
}

// ---------------------------------------------------------------------------
// FSE, the encoding side
// ---------------------------------------------------------------------------
// Of a decoding table and its distribution: cum[s] (where symbol s's cells start in `cells`, cum[nsym] = the
// table's size) and the cells of every symbol in table order.  The k-th cell of a symbol with probability f
// decodes from the state range that starts at (f + k) << bits.
RPP_ZSTD_HD void fse_enc_build(const FseEntry* t, const int16_t* freq, uint32_t nsym, uint32_t log, uint16_t* cum,
                               uint16_t* cells) {
  uint32_t at = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    cum[s] = uint16_t(at);
    at += freq[s] == -1 ? 1u : uint32_t(freq[s]);
  }
  cum[nsym] = uint16_t(at);
  for (uint32_t i = 0; i < (1u << log); ++i) {
    const uint32_t s = t[i].symbol, f = freq[s] == -1 ? 1u : uint32_t(freq[s]);
    cells[cum[s] + ((uint32_t(t[i].base) + (1u << log)) >> t[i].bits) - f] = uint16_t(i);
  }
}

// The state that decodes `sym` (probability f, cells from `first`) and then moves to state `next` by reading
// `nb` bits of value `val`.
RPP_ZSTD_HD uint32_t fse_enc_step(uint32_t f, uint32_t first, const uint16_t* cells, uint32_t log, uint32_t next,
                                  uint32_t& val, uint32_t& nb) {
  const uint32_t x = next + (1u << log);
  nb = log - highbit(f);
  if ((x >> nb) < f) --nb;
  val = x & ((1u << nb) - 1);
  return cells[first + (x >> nb) - f];
}

// ---------------------------------------------------------------------------
// the tree description
// ---------------------------------------------------------------------------
struct TreeScratch {
  uint8_t w[256];
  FseEntry t[1u << kHufWeightLog];
  int16_t freq[16];
  uint16_t next[16], cum[16], cells[1u << kHufWeightLog];
};

// The normalised distribution of counts (count[0 .. nsym), `total` together) for a table of 2^log cells: every
// value seen gets max(1, count * size / total) rounded down; what is missing goes to the value seen most often
// (the smallest such value); what is too much is taken one by one from the value with the largest share (the
// smallest such value; it holds at least 2 while no more values are seen than the table has cells).  False for
// fewer than two values seen.
RPP_ZSTD_HD bool fse_normalise(const uint32_t* count, uint32_t nsym, uint32_t total, uint32_t log, int16_t* freq) {
  const int32_t size = 1 << log;
  int32_t sum = 0;
  uint32_t seen = 0, most = 0;
  for (uint32_t v = 0; v < nsym; ++v) {
    freq[v] = 0;
    if (!count[v]) continue;
    const uint32_t share = count[v] * uint32_t(size) / total;
    freq[v] = int16_t(share ? share : 1);
    sum += freq[v];
    if (!seen || count[v] > count[most]) most = v;
    ++seen;
  }
  if (seen < 2) return false;
  if (sum < size) freq[most] = int16_t(freq[most] + size - sum);
  for (; sum > size; --sum) {
    uint32_t top = 0;
    for (uint32_t v = 1; v < nsym; ++v)
      if (freq[v] > freq[top]) top = v;
    --freq[top];
  }
  return true;
}

// the weights' counts (count[0 .. nsym), `total` weights) for a table of 2^kHufWeightLog cells
RPP_ZSTD_HD bool weight_distribution(const uint32_t* count, uint32_t nsym, uint32_t total, int16_t* freq) {
  return fse_normalise(count, nsym, total, kHufWeightLog, freq);
}

// The description of a distribution without "less than 1" probabilities (RFC 8878 4.1.1) at p (zeroed); its bytes.
RPP_ZSTD_HD uint32_t fse_write_description(const int16_t* freq, uint32_t nsym, uint32_t log, uint8_t* p) {
  uint32_t pos = 0;
  put_bits(p, pos, log - 5, 4);
  pos += 4;
  int32_t remaining = 1 << log;
  for (uint32_t s = 0; s < nsym && remaining > 0;) {
    const uint32_t nbits = highbit(uint32_t(remaining) + 1) + 1, lower = (1u << (nbits - 1)) - 1;
    const uint32_t threshold = (1u << nbits) - 1 - (uint32_t(remaining) + 1), v = uint32_t(freq[s]) + 1;
    if (v < threshold) {
      put_bits(p, pos, v, nbits - 1);
      pos += nbits - 1;
    } else {
      put_bits(p, pos, v > lower ? v + threshold : v, nbits);
      pos += nbits;
    }
    remaining -= freq[s];
    ++s;
    if (freq[s - 1] == 0)
      for (;;) {  // how many more have probability 0, two bits per turn
        uint32_t rep = 0;
        while (rep < 3 && s < nsym && freq[s] == 0) ++rep, ++s;
        put_bits(p, pos, rep, 2);
        pos += 2;
        if (rep != 3) break;
      }
  }
  return (pos + 7) >> 3;
}

// The tree description of the code lengths at desc[kTreeSlots]; its bytes, or 0 where neither form can state
// the tree.  The weights of the bytes below the highest one seen are listed.  FSE-compressed (two states that
// take turns, each ending in the first cell of its last weight, so that the decoder's last state needs bits the
// stream no longer has) when at least 2 weights with 2 values are listed, the bytes behind the header byte
// stay below 128, and it is smaller than the direct form or that cannot list the weights; else direct.
RPP_ZSTD_HD uint32_t huf_write_tree(const uint8_t* len, uint32_t longest, uint8_t* desc, TreeScratch& sc) {
  uint32_t n = 255;
  while (!len[n]) --n;  // the highest byte seen: its weight is deduced
  uint32_t count[kHufLog + 1] = {};
  for (uint32_t s = 0; s < n; ++s) {
    sc.w[s] = len[s] ? uint8_t(longest + 1 - len[s]) : 0;
    ++count[sc.w[s]];
  }
  const uint32_t direct = n <= kDirectMax ? 1 + (n + 1) / 2 : 0;
  for (uint32_t i = 0; i < kTreeSlots; ++i) desc[i] = 0;
  uint32_t nsym = kHufLog + 1;
  while (nsym > 1 && !count[nsym - 1]) --nsym;
  if (n >= 2 && weight_distribution(count, nsym, n, sc.freq) &&
      fse_build(sc.freq, nsym, kHufWeightLog, sc.t, sc.next)) {
    fse_enc_build(sc.t, sc.freq, nsym, kHufWeightLog, sc.cum, sc.cells);
    uint8_t* const p = desc + 1;
    uint32_t pos = 8 * fse_write_description(sc.freq, nsym, kHufWeightLog, p);
    uint32_t st[2] = {sc.cells[sc.cum[sc.w[n - 1]]], sc.cells[sc.cum[sc.w[n - 2]]]};  // of weight n - 1, n - 2
    for (uint32_t j = n - 2; j-- > 0;) {  // weight j moves to the state of weight j + 2
      uint32_t val, nb;
      const uint32_t k = (n - 1 - j) & 1;
      st[k] = fse_enc_step(uint32_t(sc.freq[sc.w[j]]), sc.cum[sc.w[j]], sc.cells, kHufWeightLog, st[k], val, nb);
      put_bits(p, pos, val, nb);
      pos += nb;
    }
    // st[(n - 1) & 1] is weight 0's state, the other weight 1's, which is read second
    put_bits(p, pos, st[n & 1], kHufWeightLog);
    put_bits(p, pos + kHufWeightLog, st[(n - 1) & 1], kHufWeightLog);
    pos += 2 * kHufWeightLog;
    put_bits(p, pos, 1, 1);
    const uint32_t bytes = (pos >> 3) + 1;
    if (bytes < 128 && (!direct || 1 + bytes < direct)) {
      desc[0] = uint8_t(bytes);
      return 1 + bytes;
    }
    for (uint32_t i = 0; i < kTreeSlots; ++i) desc[i] = 0;
  }
  if (!direct) return 0;
  desc[0] = uint8_t(127 + n);
  for (uint32_t i = 0; i < n; ++i) desc[1 + i / 2] |= uint8_t(i & 1 ? sc.w[i] : sc.w[i] << 4);
  return direct;
}

// ---------------------------------------------------------------------------
// literals: the choice of the form
// ---------------------------------------------------------------------------
struct LiteralsPlan {
  uint32_t kind, streams, sf, comp, bytes;  // comp: description, jump table and streams; bytes: the section's
};

RPP_ZSTD_HD uint32_t stream_literals(uint32_t m, uint32_t streams, uint32_t i) {
  if (streams == 1) return m;
  const uint32_t seg = (m + 3) / 4;
  return i < 3 ? seg : m - 3 * seg;
}

// The form of m literals that are not all one byte: Huffman with the tree description of `tree` bytes (0: none)
// and streams of bits[i] bits (before the end mark) when the section is strictly smaller than the Raw form.
RPP_ZSTD_HD LiteralsPlan plan_literals(uint32_t m, uint32_t tree, const uint32_t* bits) {
  LiteralsPlan p;
  p.kind = kLitRaw;
  p.streams = 0;
  p.sf = 0;
  p.comp = m;
  p.bytes = plain_literals_header_bytes(m) + m;
  if (!tree) return p;
  const uint32_t streams = m <= kOneStreamMax ? 1 : 4;
  uint32_t comp = tree + (streams == 4 ? 6 : 0);
  for (uint32_t i = 0; i < streams; ++i) comp += (bits[i] >> 3) + 1;
  const uint32_t sf = literals_size_format(streams, m, comp), bytes = huf_literals_header_bytes(sf) + comp;
  if (bytes >= p.bytes) return p;
  p.kind = kLitCompressed;
  p.streams = streams;
  p.sf = sf;
  p.comp = comp;
  p.bytes = bytes;
  return p;
}

// ---------------------------------------------------------------------------
// sequences
// ---------------------------------------------------------------------------
struct SeqCodes {
  uint32_t llc, mlc, ofc;     // the three codes
  uint32_t llx, mlx, ofx;     // the extra bits' values
  uint32_t llb, mlb, ofb;     // ... and their widths
};

// a sequence of ll literals, a match of ml >= 3 bytes and the offset value ov = offset + 3
RPP_ZSTD_HD SeqCodes sequence_codes(uint32_t ll, uint32_t ml, uint32_t ov) {
  SeqCodes c;
  uint32_t base;
  if (ll < 64) {
    for (c.llc = ll < 16 ? ll : 16;; ++c.llc) {
      ll_code(c.llc, base, c.llb);
      if (ll < base + (1u << c.llb)) break;
    }
  } else {
    c.llb = highbit(ll);
    c.llc = c.llb + 19;
    base = 1u << c.llb;
  }
  c.llx = ll - base;
  if (ml < 131) {
    for (c.mlc = ml < 35 ? ml - 3 : 32;; ++c.mlc) {
      ml_code(c.mlc, base, c.mlb);
      if (ml < base + (1u << c.mlb)) break;
    }
  } else {
    c.mlb = highbit(ml - 3);
    c.mlc = c.mlb + 36;
    base = (1u << c.mlb) + 3;
  }
  c.mlx = ml - base;
  c.ofc = c.ofb = highbit(ov);
  c.ofx = ov - (1u << c.ofc);
  return c;
}

// the three predefined tables as the encoder uses them; k: 0 LL, 1 OF, 2 ML
struct SeqTables {
  uint16_t info[3][kFreqSlots];  // per code: probability | first cell << 8
  uint16_t cells[3][64];
};

// table k of `tabs`; t[64], freq[kFreqSlots], next[kFreqSlots] and cum[kFreqSlots] are scratch
RPP_ZSTD_HD void seq_table_build(uint32_t k, SeqTables& tabs, FseEntry* t, int16_t* freq, uint16_t* next, uint16_t* cum) {
  uint32_t nsym, log;
  predefined(k, freq, nsym, log);
  fse_build(freq, nsym, log, t, next);
  fse_enc_build(t, freq, nsym, log, cum, tabs.cells[k]);
  for (uint32_t s = 0; s < nsym; ++s) tabs.info[k][s] = uint16_t((freq[s] == -1 ? 1 : freq[s]) | cum[s] << 8);
}

RPP_ZSTD_HD uint32_t seq_table_log(uint32_t k) { return k == 1 ? 5 : 6; }

// the first cell of `code`: the state a chain ends in
RPP_ZSTD_HD uint32_t seq_last_state(const SeqTables& tabs, uint32_t k, uint32_t code) {
  return tabs.cells[k][tabs.info[k][code] >> 8];
}

RPP_ZSTD_HD uint32_t seq_step(const SeqTables& tabs, uint32_t k, uint32_t code, uint32_t next, uint32_t& val,
                              uint32_t& nb) {
  const uint32_t e = tabs.info[k][code];
  return fse_enc_step(e & 255, e >> 8, tabs.cells[k], seq_table_log(k), next, val, nb);
}

// ---------------------------------------------------------------------------
// sequences with options: repeat offsets (kEncRepeat)
// ---------------------------------------------------------------------------
// The offset value of sequence i of its chunk (counted from 0) with the offset `off` and ll literals; off1 and
// off2 are the offsets of the sequences i - 1 and i - 2 of the same chunk (not read where i is too small).
//   R1  i >= 1, ll > 0, off == off1                 -> 1 (Repeated_Offset1)
//   R2  i >= 2, off == off2, off != off1            -> 2 with literals, 1 without (both: Repeated_Offset2)
//   else                                            -> off + 3
// A chunk's first sequence is always written in full, the value 3 and Repeated_Offset3 never.  Two invariants of
// the decoder's history (RFC 8878 3.1.1.5) make the rules safe without looking further back than two sequences,
// and so without any state that crosses a chunk:
//   I1  after any sequence, Repeated_Offset1 is that sequence's offset: a full offset and R2 put it there, R1
//       leaves the history as it is, and the history's first entry was off1 == off;
//   I2  after a sequence j >= 1 of a chunk with off_j != off_{j-1}, Repeated_Offset2 is off_{j-1}: by I1 it was
//       Repeated_Offset1 before j, and both a full offset and R2 move Repeated_Offset1 to the second place.
// R1 reads I1 after sequence i - 1.  R2 reads I2 after j = i - 1 >= 1: off_{i-1} != off_{i-2} follows from
// off_i == off_{i-2} and off_i != off_{i-1}.
RPP_ZSTD_HD uint32_t offset_value(uint32_t off, uint32_t off1, uint32_t off2, uint32_t ll, uint32_t i) {
  if (i >= 1 && off == off1) return ll ? 1 : off + 3;
  if (i >= 2 && off == off2) return ll ? 2 : 1;
  return off + 3;
}

// ---------------------------------------------------------------------------
// sequences with options: the table modes of a block (kEncTables)
// ---------------------------------------------------------------------------
// The accuracy log of a block's own table: 5, or kOwnLogMax = 6 for more than 64 sequences or more than 16 codes
// seen.  (The format allows 9, 8 and 9; the cap keeps a state's move in the 9 bits of its record.)
RPP_ZSTD_HD uint32_t own_table_log(uint32_t count, uint32_t seen) { return count > 64 || seen > 16 ? kOwnLogMax : 5; }

// What a code of probability f in a table of 2^log cells costs in state bits, in 1/256 bit:
// log - log2(f), the logarithm's fraction taken as linear between two powers of two.
RPP_ZSTD_HD uint32_t fse_symbol_cost(uint32_t f, uint32_t log) {
  const uint32_t hb = highbit(f);
  return ((log - hb) << 8) - (((f << 8) >> hb) - 256);
}

struct TablePlan {
  uint32_t mode, log, desc_bytes;  // desc_bytes: what follows the modes byte for this table (RLE: the code)
};

RPP_ZSTD_HD TablePlan predefined_plan(uint32_t k) { return TablePlan{kPredefined, seq_table_log(k), 0}; }

// The mode of table k (0 LL, 1 OF, 2 ML) of a block of `count` >= 1 sequences whose codes are counted in
// hist[kFreqSlots]:
//   RLE             one code seen: the description is that code, the table has the log 0 and no state bits;
//   FSE_Compressed  when 8 * the description's bytes + E(own) < E(predefined), where E(d) = 256 * log(d) (the first
//                   state) + the sum over the codes of count * fse_symbol_cost under d, the own distribution being
//                   fse_normalise's at own_table_log; `tabs` then gets table k's encoding side;
//   Predefined      otherwise; `tabs` is left alone (the caller put the predefined table there).
// Never Repeat_Mode.  desc[kDescSlots] gets the description; t[64], freq, next, cum [kFreqSlots] are scratch.
RPP_ZSTD_HD TablePlan plan_table(uint32_t k, const uint32_t* hist, uint32_t count, SeqTables& tabs, uint8_t* desc,
                                 FseEntry* t, int16_t* freq, uint16_t* next, uint16_t* cum) {
  uint32_t nsym = 0, seen = 0, pn, plog;
  for (uint32_t s = 0; s < kFreqSlots; ++s)
    if (hist[s]) {
      nsym = s + 1;
      ++seen;
    }
  for (uint32_t i = 0; i < kDescSlots; ++i) desc[i] = 0;
  if (seen == 1) {
    desc[0] = uint8_t(nsym - 1);
    return TablePlan{kModeRle, 0, 1};
  }
  predefined(k, freq, pn, plog);
  uint32_t pre = plog << 8;
  bool stated = true;  // (the search's codes all have a predefined probability: offset codes stay below 16)
  for (uint32_t s = 0; s < nsym; ++s)
    if (hist[s]) {
      if (s >= pn || freq[s] == 0) stated = false;
      else pre += hist[s] * fse_symbol_cost(freq[s] == -1 ? 1u : uint32_t(freq[s]), plog);
    }
  const uint32_t log = own_table_log(count, seen);
  fse_normalise(hist, nsym, count, log, freq);
  const uint32_t bytes = fse_write_description(freq, nsym, log, desc);
  uint32_t own = (8 * bytes + log) << 8;
  for (uint32_t s = 0; s < nsym; ++s)
    if (hist[s]) own += hist[s] * fse_symbol_cost(uint32_t(freq[s]), log);
  if (stated && own >= pre) return predefined_plan(k);
  fse_build(freq, nsym, log, t, next);
  fse_enc_build(t, freq, nsym, log, cum, tabs.cells[k]);
  for (uint32_t s = 0; s < nsym; ++s) tabs.info[k][s] = uint16_t(uint32_t(freq[s]) | cum[s] << 8);
  return TablePlan{kFse, log, bytes};
}

// seq_last_state and seq_step for a table of the accuracy log `log` (0: RLE, one state and no bits)
RPP_ZSTD_HD uint32_t seq_last_state_own(const SeqTables& tabs, uint32_t k, uint32_t log, uint32_t code) {
  return log ? tabs.cells[k][tabs.info[k][code] >> 8] : 0;
}

RPP_ZSTD_HD uint32_t seq_step_own(const SeqTables& tabs, uint32_t k, uint32_t log, uint32_t code, uint32_t next,
                                  uint32_t& val, uint32_t& nb) {
  if (!log) {
    val = nb = 0;
    return 0;
  }
  const uint32_t e = tabs.info[k][code];
  return fse_enc_step(e & 255, e >> 8, tabs.cells[k], log, next, val, nb);
}

}  // namespace rpp_zstd

#endif  // RPP_ZSTD_ENC_COMMON_H
