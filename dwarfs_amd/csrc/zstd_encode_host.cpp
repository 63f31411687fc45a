// zstd_encode_host.cpp -- the host side of the Zstandard block encoder: the
// size bound and the sequential restatement of the kernels of zstd_encode.hip,
// which writes the same bytes.  Plain C++: the sanitizer test
// (tests/cpp/zstd_encode_test.cpp) compiles this file with lz4_host.cpp (the
// match search) and zstd_host.cpp (the decoder).  Every rule that both sides
// need is a function of zstd_enc_common.h; this is the whole definition.
//
// Encoder definition (both the kernels and rpp_zstd_host_encode: options 0), for a block of
// n <= RPP_LZ4_MAX_BLOCK bytes.  The result is ONE RFC 8878 frame; these are not
// libzstd's bytes, and any Zstandard decoder reads them.
//   frame      the magic number; a single-segment descriptor; the
//              Frame_Content_Size in the narrowest of 1, 2 and 4 bytes that
//              holds n (the 2-byte form stores n - 256); no checksum, no
//              dictionary.  n == 0: the header and one empty Raw block flagged
//              last.
//   blocks     one per search chunk of kChunk bytes (lz4_common.h), the last
//              one flagged.  Compressed when literals section + sequences
//              section is strictly smaller than the chunk, else Raw.  No RLE
//              blocks.
//   sequences  the LZ4 encoder's match search, unchanged (defined at the top of
//              lz4_host.cpp: same table, same greedy choice, same end-of-block
//              margins; a match never crosses a chunk's end, its source may lie
//              in the chunk before).  Each chunk is closed in itself: the first
//              sequence's literals start at the chunk's start, and the bytes
//              behind the last match are the block's trailing literals.  The
//              offset value is offset + 3; repeat-offset codes are never used.
//              The count takes 1 byte below 128, else 2 (a chunk holds at most
//              kSeqsPerChunk).  A chunk without sequences writes the count
//              byte 0 and nothing else.  Otherwise the modes byte is 0 (three
//              Predefined tables) and the bitstream follows, written from the
//              last sequence to the first.  Each of the three state chains ends
//              in the first cell (in table order) of the last sequence's code;
//              sequence i's state is the one cell of its code from which the
//              state of sequence i + 1 is reached.  From the stream's first bit:
//              for i = count - 1 down to 0, the bits that move the OF, ML and
//              LL state from sequence i to i + 1 (none for the last sequence),
//              then the extra bits of LL, ML and OF; then the first ML, OF and
//              LL state; then the final 1 bit.
//   literals   the chunk's bytes outside its matches, in order; m of them.
//              m == 0: a Raw header of 0.  All equal: RLE.  Otherwise Huffman
//              when header + tree description + streams is strictly smaller
//              than the Raw form, else Raw; Raw and RLE headers take the
//              narrowest of their three widths.  Up to kOneStreamMax literals go
//              into 1 stream (size format 0); more into 4 streams behind the
//              6-byte jump table, in the narrowest of size formats 1, 2 and 3
//              that holds both sizes.  (More than 1023 literals never fit format
//              1: the encoder writes formats 0, 2 and 3.)  The first three
//              streams hold (m + 3) / 4 literals each.  A stream is written from
//              its last literal to its first and closed with a 1 bit.
//   lengths    huf_lengths: from the chunk's byte histogram, at most kHufLog
//              bits, ties by byte value.  Codes are canonical (huf_codes).
//   tree       huf_write_tree: the weights of the bytes below the highest one
//              seen, FSE-compressed (accuracy log kHufWeightLog, the
//              distribution of weight_distribution, two states that take turns,
//              each chain ending in the first cell of its last weight) when that
//              can be stated (at least 2 weights with 2 distinct values, a
//              header byte below 128) and is smaller than the direct form or
//              the direct form cannot list the weights (more than 128); else the
//              direct 4-bit form; else (more than 128 weights, all equal) the
//              literals are Raw.  No Treeless literals, no Repeat tables.
// The options word (rpp_zstd_host_encode_opt, rpp_zstd_encode_batch_opt) changes
// the sequences section only; 0 is everything above, and rpp_zstd_host_encode
// is that call.  Any bit but the two below is an invalid argument.
//   repeat     RPP_ZSTD_ENC_REPEAT.  With off_i, ll_i the offset and literal
//              length of sequence i of a chunk (from 0), offset_value gives
//                R1  i >= 1, ll_i > 0, off_i == off_{i-1}: offset value 1;
//                R2  i >= 2, off_i == off_{i-2}, off_i != off_{i-1}: offset
//                    value 2 when ll_i > 0, value 1 when ll_i == 0 (without
//                    literals the value 1 means Repeated_Offset2);
//                else offset + 3.
//              A chunk's first sequence never uses a repeat code, so no state
//              crosses a chunk; the value 3 and Repeated_Offset3 are never
//              written.  The two invariants that make the rules safe are
//              stated at offset_value.  Codes 0 and 1 (one extra bit, 0).
//   tables     RPP_ZSTD_ENC_TABLES.  For each of the LL, OF and ML tables of a
//              block with at least one sequence, plan_table chooses
//                RLE             every sequence has the same code: the
//                                description is that code, no state bits;
//                FSE_Compressed  when 8 * description bytes + E(own) <
//                                E(predefined), E(d) = 256 * log(d) + the sum
//                                over the codes of count * fse_symbol_cost (a
//                                code's cost in 1/256 bit, integer, log2 taken
//                                as linear between powers of two);
//                Predefined      otherwise.  Never Repeat_Mode.
//              The own table's accuracy log (own_table_log) is 5, or 6 for more
//              than 64 sequences or more than 16 codes seen: capped at
//              kOwnLogMax = 6 below the format's 9, 8 and 9, so that a state's
//              move (value and width, 6 bits and 6 at most) keeps the 9 bits it
//              has in the kernels' workspace record.  Its distribution is
//              fse_normalise's: every code seen gets max(1, count * size /
//              total); what is missing goes to the code seen most often, what
//              is too much is taken one by one from the code with the largest
//              share; ties by code value; no "less than 1" probabilities.
//              The section is then: count, modes byte, the descriptions in LL,
//              OF, ML order (fse_write_description; RLE: the code), bitstream;
//              the chains as above in the block's tables, the first states
//              written in their tables' logs (RLE: 0 bits).
// The search word (rpp_zstd_host_encode_search, rpp_zstd_encode_batch_search)
// changes the sequences alone: the LZ4 encoder's deeper search, defined at the
// top of lz4_host.cpp.  0 is the search above; the options word applies to
// whatever sequences the search hands over.
// The block rule (Compressed only when strictly smaller than the chunk) and so
// rpp_zstd_bound are the same for every options word and every search word.
// The ratio flag is size >= n (zstd_block_compressor::compress's
// bad_compression_ratio_error, src/compression/zstd.cpp:435).
#include <algorithm>
#include <cstring>
#include <vector>

#include "lz4_internal.h"
#include "ricepp_amd.h"
#include "zstd_enc_common.h"
#include "zstd_long_internal.h"

namespace {

using namespace rpp_zstd;

struct Tables {
  SeqTables seq;
  Tables() {
    FseEntry t[64];
    int16_t freq[kFreqSlots];
    uint16_t next[kFreqSlots], cum[kFreqSlots];
    for (uint32_t k = 0; k < 3; ++k) seq_table_build(k, seq, t, freq, next, cum);
  }
};

// one Huffman stream of the literals [lits, lits + m) at p (zeroed); its bytes
uint32_t write_stream(const uint8_t* lits, uint32_t m, const uint32_t* ctab, uint8_t* p) {
  uint32_t pos = 0;
  for (uint32_t i = m; i-- > 0;) {
    const uint32_t e = ctab[lits[i]];
    put_bits(p, pos, e & 0xffff, e >> 16);
    pos += e >> 16;
  }
  put_bits(p, pos, 1, 1);
  return (pos >> 3) + 1;
}

// The literals section of the m literals at o (zeroed, at least the section's size); its bytes.
uint32_t write_literals(const uint8_t* lits, uint32_t m, const uint32_t* hist, uint8_t* o, bool write,
                        LiteralsPlan* planned) {
  LiteralsPlan plan{kLitRaw, 0, 0, m, plain_literals_header_bytes(m) + m};
  uint8_t len[256], desc[kTreeSlots];
  uint32_t ctab[256], tree = 0;
  if (m && hist[lits[0]] == m) {
    plan.kind = kLitRle;
    plan.bytes = plain_literals_header_bytes(m) + 1;
  } else if (m) {
    TreeScratch sc;
    const uint32_t longest = huf_lengths(hist, m, len);
    tree = huf_write_tree(len, longest, desc, sc);
    huf_codes(len, longest, ctab);
    const uint32_t streams = m <= kOneStreamMax ? 1 : 4;
    uint32_t bits[4] = {}, at = 0;
    for (uint32_t i = 0; i < streams; ++i) {
      const uint32_t k = stream_literals(m, streams, i);
      for (uint32_t j = 0; j < k; ++j) bits[i] += ctab[lits[at + j]] >> 16;
      at += k;
    }
    plan = plan_literals(m, tree, bits);
  }
  if (planned) *planned = plan;
  if (!write) return plan.bytes;
  if (plan.kind != kLitCompressed) {
    const uint32_t h = plain_literals_header(plan.kind, m, o);
    if (plan.kind == kLitRle) o[h] = lits[0];
    else if (m) std::memcpy(o + h, lits, m);
    return plan.bytes;
  }
  uint8_t* p = o + huf_literals_header(plan.sf, m, plan.comp, o);
  std::memcpy(p, desc, tree);
  p += tree;
  if (plan.streams == 1) {
    write_stream(lits, m, ctab, p);
  } else {
    uint8_t* const jump = p;
    p += 6;
    for (uint32_t i = 0, at = 0; i < 4; ++i) {
      const uint32_t k = stream_literals(m, 4, i), bytes = write_stream(lits + at, k, ctab, p);
      if (i < 3) {
        jump[2 * i] = uint8_t(bytes);
        jump[2 * i + 1] = uint8_t(bytes >> 8);
      }
      p += bytes;
      at += k;
    }
  }
  return plan.bytes;
}

struct Trans {  // what moves the three states from a sequence to the next one
  uint8_t val[3], nb[3];
};

// The sequences section of a chunk that starts at `cs` at o (zeroed, when `write`); its bytes.  `tabs` holds the
// three predefined tables and is left so; with kEncTables the block's own tables are built in a copy.
uint32_t write_sequences(const rpp_lz4::Seq* seqs, uint32_t count, uint32_t cs, uint32_t options, const SeqTables& tabs,
                         std::vector<SeqCodes>& codes, std::vector<Trans>& trans, uint8_t* o, bool write) {
  if (count == 0) {
    if (write) o[0] = 0;
    return 1;
  }
  codes.resize(count);
  trans.resize(count);
  uint32_t prev = cs, bits = 0, hist[3][kFreqSlots] = {};
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t ll = seqs[i].pos - prev;
    const uint32_t ov = options & kEncRepeat
                            ? offset_value(seqs[i].off, i >= 1 ? seqs[i - 1].off : 0, i >= 2 ? seqs[i - 2].off : 0, ll, i)
                            : seqs[i].off + 3;
    codes[i] = sequence_codes(ll, seqs[i].len, ov);
    bits += codes[i].llb + codes[i].mlb + codes[i].ofb;
    ++hist[0][codes[i].llc];
    ++hist[1][codes[i].ofc];
    ++hist[2][codes[i].mlc];
    prev = seqs[i].pos + seqs[i].len;
  }
  TablePlan plan[3] = {predefined_plan(0), predefined_plan(1), predefined_plan(2)};
  uint8_t desc[3][kDescSlots];
  SeqTables own;
  if (options & kEncTables) {
    own = tabs;
    FseEntry t[64];
    int16_t freq[kFreqSlots];
    uint16_t next[kFreqSlots], cum[kFreqSlots];
    for (uint32_t k = 0; k < 3; ++k) plan[k] = plan_table(k, hist[k], count, own, desc[k], t, freq, next, cum);
  }
  const SeqTables& use = options & kEncTables ? own : tabs;
  uint32_t st[3], described = 0;
  for (uint32_t k = 0; k < 3; ++k) {
    auto code = [&](uint32_t i) { return k == 0 ? codes[i].llc : k == 1 ? codes[i].ofc : codes[i].mlc; };
    st[k] = seq_last_state_own(use, k, plan[k].log, code(count - 1));
    trans[count - 1].nb[k] = 0;
    for (uint32_t i = count - 1; i-- > 0;) {
      uint32_t val, nb;
      st[k] = seq_step_own(use, k, plan[k].log, code(i), st[k], val, nb);
      trans[i].val[k] = uint8_t(val);
      trans[i].nb[k] = uint8_t(nb);
      bits += nb;
    }
    bits += plan[k].log;  // the first state
    described += plan[k].desc_bytes;
  }
  const uint32_t head = sequence_count_bytes(count, nullptr) + 1, total = head + described + (bits >> 3) + 1;
  if (!write) return total;
  sequence_count_bytes(count, o);
  o[head - 1] = uint8_t(plan[0].mode << 6 | plan[1].mode << 4 | plan[2].mode << 2);  // options 0: 0, all Predefined
  uint8_t* p = o + head;
  for (uint32_t k = 0; k < 3; ++k) {  // the descriptions in LL, OF, ML order
    if (plan[k].desc_bytes) std::memcpy(p, desc[k], plan[k].desc_bytes);
    p += plan[k].desc_bytes;
  }
  uint32_t pos = 0;
  auto put = [&](uint32_t v, uint32_t nb) {  // (put_bits takes 16 bits; an offset's extra bits reach 27 with long = 1)
    if (nb > 16) {
      put_bits(p, pos, v & 0xffffu, 16);
      put_bits(p, pos + 16, v >> 16, nb - 16);
    } else {
      put_bits(p, pos, v, nb);
    }
    pos += nb;
  };
  for (uint32_t i = count; i-- > 0;) {
    const SeqCodes& c = codes[i];
    const Trans& t = trans[i];
    put(t.val[1], t.nb[1]);
    put(t.val[2], t.nb[2]);
    put(t.val[0], t.nb[0]);
    put(c.llx, c.llb);
    put(c.mlx, c.mlb);
    put(c.ofx, c.ofb);
  }
  put(st[2], plan[2].log);
  put(st[1], plan[1].log);
  put(st[0], plan[0].log);
  put(1, 1);
  return total;
}

}  // namespace

extern "C" uint64_t rpp_zstd_bound(uint64_t n) { return encode_bound(n); }

static_assert(RPP_ZSTD_ENC_TABLES == kEncTables && RPP_ZSTD_ENC_REPEAT == kEncRepeat, "the options word");

extern "C" int rpp_zstd_host_encode(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t capacity,
                                    uint64_t* out_bytes, uint32_t* bad_ratio) {
  return rpp_zstd_host_encode_opt(in, n, 0, out, capacity, out_bytes, bad_ratio);
}

extern "C" int rpp_zstd_host_encode_opt(const uint8_t* in, uint64_t n, uint32_t options, uint8_t* out,
                                        uint64_t capacity, uint64_t* out_bytes, uint32_t* bad_ratio) {
  return rpp_zstd_host_encode_search(in, n, options, 0, out, capacity, out_bytes, bad_ratio);
}

extern "C" int rpp_zstd_host_encode_search(const uint8_t* in, uint64_t n, uint32_t options, uint32_t search,
                                           uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                                           uint32_t* bad_ratio) {
  if ((n && !in) || !out || !out_bytes || (options & ~kEncOptionsMask) || !rpp_lz4::search_valid(search))
    return RPP_INVALID_ARGUMENT;
  if (n > rpp_lz4::kMaxBlock) return RPP_INVALID_ARGUMENT;
  if (capacity < encode_bound(n)) return RPP_OUTPUT_TOO_SMALL;
  std::vector<rpp_lz4::Seq> seqs;
  rpp_lz4::find_sequences(in, uint32_t(n), seqs, search);
  rpp_zstd::write_frame(in, uint32_t(n), options, seqs, out, out_bytes, bad_ratio);
  return RPP_OK;
}

// The frame of a block of n bytes from its sequences (in order, none across a chunk's end), at out
// (encode_bound(n) bytes): everything of the definition above behind the search.  Also the back end of
// rpp_zstd_host_encode_long (zstd_long_host.cpp), whose sequences come from two searches.
void rpp_zstd::write_frame(const uint8_t* in, uint32_t n, uint32_t options, const std::vector<rpp_lz4::Seq>& seqs,
                           uint8_t* out, uint64_t* out_bytes, uint32_t* bad_ratio) {
  static const Tables tables;
  uint8_t* o = out + frame_header(n, out);
  if (n == 0) {
    block_header(o, true, kRaw, 0);
    o += 3;
  }
  std::vector<uint8_t> lits(kEncChunk), body(kEncChunk);
  std::vector<SeqCodes> codes;
  std::vector<Trans> trans;
  size_t si = 0;
  for (uint32_t cs = 0; cs < n; cs += kEncChunk) {
    const uint32_t ce = uint32_t(std::min<uint64_t>(uint64_t(cs) + kEncChunk, n)), cn = ce - cs;
    const size_t s0 = si;
    uint32_t hist[256] = {}, m = 0, prev = cs;
    auto take = [&](uint32_t from, uint32_t to) {
      for (uint32_t q = from; q < to; ++q) ++hist[lits[m++] = in[q]];
    };
    for (; si < seqs.size() && seqs[si].pos < ce; ++si) {
      take(prev, seqs[si].pos);
      prev = seqs[si].pos + seqs[si].len;
    }
    take(prev, ce);
    const uint32_t count = uint32_t(si - s0);
    const rpp_lz4::Seq* const cseqs = seqs.data() + s0;  // (not dereferenced when count == 0)
    const uint32_t lit_bytes = write_literals(lits.data(), m, hist, nullptr, false, nullptr);
    const uint32_t seq_bytes = write_sequences(cseqs, count, cs, options, tables.seq, codes, trans, nullptr, false);
    const bool last = ce == n;
    if (uint64_t(lit_bytes) + seq_bytes < cn) {
      std::fill(body.begin(), body.begin() + lit_bytes + seq_bytes, uint8_t(0));
      write_literals(lits.data(), m, hist, body.data(), true, nullptr);
      write_sequences(cseqs, count, cs, options, tables.seq, codes, trans, body.data() + lit_bytes, true);
      block_header(o, last, kCompressed, lit_bytes + seq_bytes);
      std::memcpy(o + 3, body.data(), lit_bytes + seq_bytes);
      o += 3 + lit_bytes + seq_bytes;
    } else {
      block_header(o, last, kRaw, cn);
      std::memcpy(o + 3, in + cs, cn);
      o += 3 + cn;
    }
  }
  *out_bytes = uint64_t(o - out);
  if (bad_ratio) *bad_ratio = *out_bytes >= n ? 1u : 0u;  // bad_compression_ratio_error (zstd.cpp:435)
}
