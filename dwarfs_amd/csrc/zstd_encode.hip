// zstd_encode.hip -- the Zstandard block encoder on the GPU (gfx950).  The
// format, and every rule that decides a byte, is stated at the top of
// zstd_encode_host.cpp, the sequential restatement that writes the same bytes;
// the rules themselves are the functions of zstd_enc_common.h, which both use.
//
// Five launches: the LZ4 encoder's prep and search (lz4_internal.h: the same
// kernels, one wave per 32 KiB chunk, a sequence list per chunk), then
//   entropy  one wave per chunk: gathers the literals (an LDS histogram on the
//            way), chooses their form, builds code lengths and tree description
//            (lane 0, the shared sequential functions), runs the three FSE state
//            chains, and, when the block comes out smaller than the chunk,
//            writes literals and sequences sections into the chunk's slot of
//            the workspace;
//   place    one wave per frame: the frame header, an exclusive scan of the
//            block sizes, the frame's size and its ratio flag;
//   emit     one wave per chunk: block header and the block's bytes (the slot,
//            or the chunk itself for a Raw block) at their place.
// Bit streams are assembled in a 4 KiB LDS window: every lane computes the width
// of its codes, a wave prefix sum gives their bit positions, and the codes are
// OR-ed into the window's words (LDS atomics: the result does not depend on
// their order); full words leave with 4-byte stores.  Huffman emission takes 256
// literals per turn, the sequence stream 64 sequences (six fields each).  The
// FSE chains are sequential by nature (each state depends on the next
// sequence's): the three run side by side in lanes 0 to 2 over a register tile
// of 64 codes, and only their results (9 bits per chain and sequence) go to
// memory; everything else about a sequence is recomputed in parallel.
// No global atomics.  Variable shifts are 32-bit ("64-bit
// shifts and the last VGPR").
//
// The entropy kernel is a template on "options != 0" (rpp_zstd_encode_batch_opt).
// The `false` instantiation is the code path above and writes its bytes.  The
// `true` one adds, where the options word asks for it: the offsets of the two
// sequences before (a lane shuffle, and across a tile of 64 the carry of the
// tile's last two offsets) for the repeat-offset rule; LDS histograms of the
// three code alphabets; the table modes, chosen and built by lanes 0 to 2, one
// table each, with the shared sequential function plan_table; the descriptions
// behind the modes byte; and chains and first states in each table's own log.
// A state's move stays val | nb << 6 in 9 bits of the `tr` record because the
// own tables' accuracy log is capped at 6 (kOwnLogMax: val and nb are at most
// 6 bits and 6), so the workspace is the same for every options word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RPP_LZ4_KERNEL_SIDE
#include "lz4_internal.h"
#include "ricepp_amd.h"
#include "zstd_enc_common.h"
#include "zstd_enc_internal.h"
#include "zstd_long_common.h"
#include "zstd_long_internal.h"

namespace {

using namespace rpp_zstd;
using rpp_lz4::block_of_chunk;
using rpp_lz4::EncodeWs;
using rpp_lz4::kSeqsPerChunk;

constexpr uint32_t kWave = 64;
constexpr uint32_t kWinWords = 1024;  // the LDS window
constexpr uint32_t kTileBits = 4096;  // what one turn adds, at most: 256 codes of 11 bits, 64 sequences of 62
constexpr uint32_t kLitsPerLane = 4;  // (with own tables 63: three moves of kOwnLogMax bits, 15 extra bits thrice)
static_assert(kWave * kLitsPerLane * kHufLog <= kTileBits && kWave * (3 * kOwnLogMax + 45) <= kTileBits,
              "a turn fits the window");
// With the `long` word an offset's extra bits reach 27 where they stayed at 15: a turn of 64 sequences adds more.
constexpr uint32_t kTileBitsLong = kWave * (3 * kOwnLogMax + 30 + 27);
static_assert(kTileBitsLong + 32 <= 32 * kWinWords / 2, "a turn of wide offsets fits the window");

// The fields of a workspace record.  kLong: the widened record (zstd_long_common.h), whose offset continues in
// the upper half of .y; without it the short search's record as it always was.
template <bool kLong>
__device__ inline uint32_t seq_len(uint2 s) {
  if constexpr (kLong) return rpp_zstd_long::rec_len(s.y);
  else return s.y;
}

template <bool kLong>
__device__ inline uint32_t seq_off(uint2 s) {
  if constexpr (kLong) return rpp_zstd_long::rec_off(s.x, s.y);
  else return s.x >> 16;
}

struct ZstdWs {
  uint8_t* lits;   // per chunk: [kEncChunk] its literals
  uint8_t* body;   //   [kEncChunk] literals and sequences section of a Compressed block
  uint32_t* tr;    //   [kSeqsPerChunk] per sequence: codes, then the bits that move the three states on
  uint32_t* kind;  //   block type
  uint32_t* size;  //   Block_Size
  uint32_t* at;    //   where the block header goes in the frame
};

__device__ inline uint32_t lane_id() { return threadIdx.x & (kWave - 1); }

__device__ inline uint32_t wave_incl_sum(uint32_t v, uint32_t lane) {
  for (uint32_t d = 1; d < kWave; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ inline uint32_t wave_sum(uint32_t v, uint32_t lane) { return __shfl(wave_incl_sum(v, lane), kWave - 1); }

// n bytes from s to d, the two ranges apart; 4 bytes per lane while 256 are left
__device__ inline void wave_copy(uint8_t* d, const uint8_t* s, uint32_t n, uint32_t lane) {
  uint32_t k = 0;
  for (; k + 256 <= n; k += 256) {
    uint32_t v;
    __builtin_memcpy(&v, s + k + 4 * lane, 4);
    __builtin_memcpy(d + k + 4 * lane, &v, 4);
  }
  for (uint32_t j = k + lane; j < n; j += kWave) d[j] = s[j];
}

// what this wave stored to global memory is read back by other lanes behind this
__device__ inline void wave_publish() {
  __threadfence();
  __syncthreads();
}

// ---------------------------------------------------------------------------
// the bit window
// ---------------------------------------------------------------------------
struct Win {
  uint32_t* w;       // LDS [kWinWords]: the stream's words from `flushed` on
  uint8_t* dst;      // where the stream's first byte goes
  uint32_t flushed;  // words stored
};

__device__ inline void win_open(Win& win, uint32_t* lds, uint8_t* dst, uint32_t lane) {
  win.w = lds;
  win.dst = dst;
  win.flushed = 0;
  __syncthreads();
  for (uint32_t i = lane; i < kWinWords; i += kWave) lds[i] = 0;
  __syncthreads();
}

// nb <= 32 bits of v (nothing above them) at bit `pos` of the stream
__device__ inline void win_put(const Win& win, uint32_t pos, uint32_t v, uint32_t nb) {
  if (nb == 0) return;
  const uint32_t rel = pos - 32 * win.flushed, word = rel >> 5, sh = rel & 31;
  atomicOr(&win.w[word], v << sh);
  if (sh + nb > 32) atomicOr(&win.w[word + 1], v >> (32 - sh));
}

// room for a turn of kTurnBits bits from `pos` on (uniform): stores the full words when the window runs short
template <uint32_t kTurnBits = kTileBits>
__device__ inline void win_room(Win& win, uint32_t pos, uint32_t lane) {
  if (pos - 32 * win.flushed + kTurnBits + 32 <= 32 * kWinWords) return;
  __syncthreads();
  const uint32_t full = (pos >> 5) - win.flushed;
  for (uint32_t k = lane; k < full; k += kWave) {
    const uint32_t v = win.w[k];
    __builtin_memcpy(win.dst + 4 * (win.flushed + k), &v, 4);
  }
  const uint32_t part = win.w[full];
  __syncthreads();
  for (uint32_t k = lane; k <= full; k += kWave) win.w[k] = k == 0 ? part : 0;
  __syncthreads();
  win.flushed += full;
}

// the final 1 bit behind `pos` bits, and the bytes still in the window; the stream's bytes
__device__ inline uint32_t win_close(Win& win, uint32_t pos, uint32_t lane) {
  __syncthreads();
  if (lane == 0) win_put(win, pos, 1, 1);
  __syncthreads();
  const uint32_t bytes = (pos >> 3) + 1, rest = bytes - 4 * win.flushed;
  for (uint32_t k = lane; k < rest; k += kWave) win.dst[4 * win.flushed + k] = uint8_t(win.w[k >> 2] >> (8 * (k & 3)));
  return bytes;
}

// one Huffman stream of the literals [lits, lits + m) at dst, from the last literal to the first
__device__ inline void emit_stream(uint32_t* lds, uint8_t* dst, const uint8_t* lits, uint32_t m, const uint32_t* ctab,
                                   uint32_t lane) {
  Win win;
  win_open(win, lds, dst, lane);
  uint32_t pos = 0;
  for (uint32_t t = 0; t < m; t += kWave * kLitsPerLane) {
    win_room(win, pos, lane);
    uint32_t e[kLitsPerLane], width = 0;
    for (uint32_t q = 0; q < kLitsPerLane; ++q) {
      const uint32_t r = t + kLitsPerLane * lane + q;  // counted from the end
      e[q] = r < m ? ctab[lits[m - 1 - r]] : 0;
      width += e[q] >> 16;
    }
    const uint32_t incl = wave_incl_sum(width, lane);
    uint32_t at = pos + incl - width;
    for (uint32_t q = 0; q < kLitsPerLane; ++q) {
      win_put(win, at, e[q] & 0xffffu, e[q] >> 16);
      at += e[q] >> 16;
    }
    pos += __shfl(incl, kWave - 1);
  }
  win_close(win, pos, lane);
}

// `lit` bytes of the input into the literals, counted in the histogram, by the whole wave
__device__ inline void wave_gather(uint8_t* d, const uint8_t* s, uint32_t lit, uint32_t* hist, uint32_t lane) {
  for (uint32_t j = lane; j < lit; j += kWave) {
    const uint32_t v = s[j];
    d[j] = uint8_t(v);
    atomicAdd(&hist[v], 1u);
  }
}

struct SeqView {  // sequence i of a chunk that starts at cs
  uint32_t ll, ml, ov;
};

template <bool kLong>
__device__ inline SeqView seq_view(const uint2* seqs, uint32_t i, uint32_t cs) {
  const uint2 s = seqs[i];
  uint32_t prev = cs;
  if (i) {
    const uint2 p = seqs[i - 1];
    prev = cs + (p.x & 0xffffu) + seq_len<kLong>(p);
  }
  return SeqView{cs + (s.x & 0xffffu) - prev, seq_len<kLong>(s), seq_off<kLong>(s) + 3};
}

// ... with the offset value of the repeat-offset rule
template <bool kLong>
__device__ inline SeqView seq_view_repeat(const uint2* seqs, uint32_t i, uint32_t cs) {
  SeqView v = seq_view<kLong>(seqs, i, cs);
  const uint32_t off1 = i >= 1 ? seq_off<kLong>(seqs[i - 1]) : 0, off2 = i >= 2 ? seq_off<kLong>(seqs[i - 2]) : 0;
  v.ov = offset_value(v.ov - 3, off1, off2, v.ll, i);
  return v;
}

// ---------------------------------------------------------------------------
// entropy: one wave per chunk
// ---------------------------------------------------------------------------
template <bool kOpt, bool kLong>  // kOpt: options != 0; kLong: the sequences are widened records (long = 1)
__global__ __launch_bounds__(kWave) void rpp_zstd_enc_entropy_kernel(const uint8_t* __restrict__ d_in,
                                                                const uint64_t* __restrict__ in_offsets,
                                                                const uint64_t* __restrict__ n_bytes,
                                                                uint32_t nblocks, EncodeWs ws, ZstdWs zws,
                                                                uint32_t options) {
  __shared__ uint32_t win_words[kWinWords], hist[256], ctab[256], shared[2];
  __shared__ uint8_t lens[256], desc[kTreeSlots];
  __shared__ TreeScratch sc;
  __shared__ SeqTables tabs;
  __shared__ FseEntry build_t[3][64];
  __shared__ int16_t build_freq[3][kFreqSlots];
  __shared__ uint16_t build_next[3][kFreqSlots], build_cum[3][kFreqSlots];
  __shared__ uint32_t code_hist[3][kFreqSlots], table_plan[3][3];  // (kOpt only) per table: mode, log, description bytes
  __shared__ uint8_t table_desc[3][kDescSlots];                    // (kOpt only)
  const uint32_t g = blockIdx.x, lane = lane_id();
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const uint32_t b = block_of_chunk(ws.chunk_base, nblocks, g);
  const uint8_t* const in = d_in + in_offsets[b];
  const uint32_t n = uint32_t(n_bytes[b]);
  const uint32_t cs = (g - ws.chunk_base[b]) * kEncChunk, ce = min(cs + kEncChunk, n), cn = ce - cs;
  const uint32_t cnt = ws.cnt[g];
  const uint2* const seqs = ws.seqs + uint64_t(g) * kSeqsPerChunk;
  uint8_t* const lits = zws.lits + uint64_t(g) * kEncChunk;
  uint8_t* const body = zws.body + uint64_t(g) * kEncChunk;
  uint32_t* const tr = zws.tr + uint64_t(g) * kSeqsPerChunk;

  for (uint32_t s = lane; s < 256; s += kWave) hist[s] = 0;
  if constexpr (kOpt)
    for (uint32_t k = 0; k < 3; ++k) code_hist[k][lane] = 0;
  if (lane < 3) seq_table_build(lane, tabs, build_t[lane], build_freq[lane], build_next[lane], build_cum[lane]);
  __syncthreads();

  // the literals: a run of up to 64 bytes by its lane, a longer one by the wave; the codes of every sequence
  uint32_t m = 0, prev_end = cs, extra_bits = 0;
  [[maybe_unused]] uint32_t off_carry1 = 0, off_carry2 = 0;  // the offsets of the last two sequences of the tile before
  for (uint32_t t = 0; t < cnt; t += kWave) {
    const uint32_t i = t + lane, here = min(cnt - t, kWave);
    const bool has = i < cnt;
    const uint2 s = has ? seqs[i] : make_uint2(0, 0);
    const uint32_t pos = cs + (s.x & 0xffffu), len = seq_len<kLong>(s);
    const uint32_t end = has ? pos + len : 0;
    uint32_t prev = __shfl_up(end, 1);
    if (lane == 0) prev = prev_end;
    const uint32_t lit = has ? pos - prev : 0;
    const uint32_t incl = wave_incl_sum(lit, lane), mine = m + incl - lit;
    uint32_t ov = seq_off<kLong>(s) + 3;
    if constexpr (kOpt) {
      const uint32_t off = seq_off<kLong>(s);
      uint32_t off1 = __shfl_up(off, 1), off2 = __shfl_up(off, 2);
      if (lane == 0) off1 = off_carry1;
      if (lane < 2) off2 = lane == 0 ? off_carry2 : off_carry1;
      if (has && (options & kEncRepeat)) ov = offset_value(off, off1, off2, lit, i);
      off_carry1 = uint32_t(__shfl(off, int(kWave - 1)));  // (read only behind a full tile)
      off_carry2 = uint32_t(__shfl(off, int(kWave - 2)));
    }
    if (has) {
      const SeqCodes c = sequence_codes(lit, len, ov);
      extra_bits += c.llb + c.mlb + c.ofb;
      tr[i] = c.llc | c.ofc << 6 | c.mlc << 12;
      if constexpr (kOpt)
        if (options & kEncTables) {
          atomicAdd(&code_hist[0][c.llc], 1u);
          atomicAdd(&code_hist[1][c.ofc], 1u);
          atomicAdd(&code_hist[2][c.mlc], 1u);
        }
      if (lit <= kWave)
        for (uint32_t j = 0; j < lit; ++j) {
          const uint32_t v = in[prev + j];
          lits[mine + j] = uint8_t(v);
          atomicAdd(&hist[v], 1u);
        }
    }
    uint64_t big = __ballot(has && lit > kWave);
    while (big) {
      const int j = __builtin_ctzll(big);
      big &= big - 1;
      wave_gather(lits + uint32_t(__shfl(mine, j)), in + uint32_t(__shfl(prev, j)), uint32_t(__shfl(lit, j)), hist, lane);
    }
    m += uint32_t(__shfl(incl, kWave - 1));
    prev_end = uint32_t(__shfl(end, int(here - 1)));
  }
  wave_gather(lits + m, in + prev_end, ce - prev_end, hist, lane);
  m += ce - prev_end;
  extra_bits = wave_sum(extra_bits, lane);
  wave_publish();

  // the literals' form
  LiteralsPlan plan{kLitRaw, 0, 0, m, plain_literals_header_bytes(m) + m};
  uint32_t tree = 0, bits[4] = {0, 0, 0, 0};
  if (m) {
    bool one = false;
    for (uint32_t s = lane; s < 256; s += kWave) one = one || hist[s] == m;
    if (__any(one)) {
      plan.kind = kLitRle;
      plan.bytes = plain_literals_header_bytes(m) + 1;
    } else {
      if (lane == 0) {
        const uint32_t longest = huf_lengths(hist, m, lens);
        shared[0] = huf_write_tree(lens, longest, desc, sc);
        huf_codes(lens, longest, ctab);
      }
      __syncthreads();
      tree = shared[0];
      const uint32_t streams = m <= kOneStreamMax ? 1 : 4;
      for (uint32_t i = 0, at = 0; i < streams; ++i) {
        const uint32_t k = stream_literals(m, streams, i);
        uint32_t sum = 0;
        for (uint32_t j = lane; j < k; j += kWave) sum += ctab[lits[at + j]] >> 16;
        bits[i] = wave_sum(sum, lane);
        at += k;
      }
      plan = plan_literals(m, tree, bits);
    }
  }

  // the three state chains, side by side in lanes 0 to 2 (the other lanes repeat them), from the last sequence
  uint32_t seq_bytes = 1, first_state[3] = {0, 0, 0};
  [[maybe_unused]] uint32_t tmode[3] = {0, 0, 0}, tlog[3] = {6, 5, 6}, tdesc[3] = {0, 0, 0};
  if constexpr (kOpt)
    if (cnt) {  // the table modes: lanes 0 to 2 choose and build one table each (tabs holds the predefined ones)
      if (lane < 3) {
        TablePlan p = predefined_plan(lane);
        if (options & kEncTables)
          p = plan_table(lane, code_hist[lane], cnt, tabs, table_desc[lane], build_t[lane], build_freq[lane],
                         build_next[lane], build_cum[lane]);
        table_plan[lane][0] = p.mode;
        table_plan[lane][1] = p.log;
        table_plan[lane][2] = p.desc_bytes;
      }
      __syncthreads();
      for (uint32_t q = 0; q < 3; ++q) {
        tmode[q] = table_plan[q][0];
        tlog[q] = table_plan[q][1];
        tdesc[q] = table_plan[q][2];
      }
    }
  if (cnt) {
    const uint32_t k = lane % 3;
    [[maybe_unused]] const uint32_t my_log = k == 0 ? tlog[0] : k == 1 ? tlog[1] : tlog[2];
    uint32_t st = 0, state_bits = 0;
    for (uint32_t tile = (cnt - 1) / kWave * kWave;; tile -= kWave) {
      const uint32_t i = tile + lane, here = min(cnt - tile, kWave);
      const uint32_t codes = i < cnt ? tr[i] : 0;  // (stored by this lane)
      uint32_t out = 0;
      for (uint32_t j = here; j-- > 0;) {
        const uint32_t code = uint32_t(__shfl(codes, int(j))) >> (6 * k) & 63;
        uint32_t mine = 0;
        if (tile + j == cnt - 1) {
          if constexpr (kOpt) st = seq_last_state_own(tabs, k, my_log, code);
          else st = seq_last_state(tabs, k, code);
        } else {
          uint32_t val, nb;
          if constexpr (kOpt) st = seq_step_own(tabs, k, my_log, code, st, val, nb);
          else st = seq_step(tabs, k, code, st, val, nb);
          mine = val | nb << 6;
          state_bits += nb;
        }
        const uint32_t packed = uint32_t(__shfl(mine, 0)) | uint32_t(__shfl(mine, 1)) << 9 | uint32_t(__shfl(mine, 2)) << 18;
        if (lane == j) out = packed;
      }
      if (i < cnt) tr[i] = out;
      if (tile == 0) break;
    }
    uint32_t total_bits = (kOpt ? tlog[0] + tlog[1] + tlog[2] : kSeqInitBits) + extra_bits;
    for (uint32_t q = 0; q < 3; ++q) {
      first_state[q] = uint32_t(__shfl(st, int(q)));
      total_bits += uint32_t(__shfl(state_bits, int(q)));
    }
    seq_bytes = sequence_count_bytes(cnt, nullptr) + 1 + (total_bits >> 3) + 1;
    if constexpr (kOpt) seq_bytes += tdesc[0] + tdesc[1] + tdesc[2];
    wave_publish();
  }

  const bool compressed = plan.bytes + seq_bytes < cn;
  if (lane == 0) {
    zws.kind[g] = compressed ? kCompressed : kRaw;
    zws.size[g] = compressed ? plan.bytes + seq_bytes : cn;
  }
  if (!compressed) return;

  // the literals section
  if (plan.kind != kLitCompressed) {
    const uint32_t h = plain_literals_header_bytes(m);
    if (lane == 0) {
      plain_literals_header(plan.kind, m, body);
      if (plan.kind == kLitRle) body[h] = lits[0];
    }
    if (plan.kind == kLitRaw) wave_copy(body + h, lits, m, lane);
  } else {
    const uint32_t h = huf_literals_header_bytes(plan.sf);
    if (lane == 0) huf_literals_header(plan.sf, m, plan.comp, body);
    for (uint32_t j = lane; j < tree; j += kWave) body[h + j] = desc[j];
    uint8_t* p = body + h + tree;
    if (plan.streams == 4) {
      if (lane < 3) {
        const uint32_t bytes = (bits[lane == 0 ? 0 : lane == 1 ? 1 : 2] >> 3) + 1;
        p[2 * lane] = uint8_t(bytes);
        p[2 * lane + 1] = uint8_t(bytes >> 8);
      }
      p += 6;
    }
    for (uint32_t i = 0, at = 0; i < plan.streams; ++i) {
      const uint32_t k = stream_literals(m, plan.streams, i);
      emit_stream(win_words, p, lits + at, k, ctab, lane);
      p += (bits[i] >> 3) + 1;
      at += k;
    }
  }

  // the sequences section
  uint8_t* const q = body + plan.bytes;
  if (cnt == 0) {
    if (lane == 0) q[0] = 0;
    return;
  }
  uint32_t head = sequence_count_bytes(cnt, nullptr) + 1;
  if (lane == 0) {
    sequence_count_bytes(cnt, q);
    q[head - 1] = kOpt ? uint8_t(tmode[0] << 6 | tmode[1] << 4 | tmode[2] << 2) : 0;  // 0: three Predefined tables
  }
  if constexpr (kOpt)
    for (uint32_t k = 0; k < 3; ++k) {  // the descriptions in LL, OF, ML order
      if (lane < tdesc[k]) q[head + lane] = table_desc[k][lane];
      head += tdesc[k];
    }
  Win win;
  win_open(win, win_words, q + head, lane);
  uint32_t pos = 0;
  for (uint32_t t = 0; t < cnt; t += kWave) {
    win_room<kLong ? kTileBitsLong : kTileBits>(win, pos, lane);
    const uint32_t r = t + lane;  // counted from the end
    const bool has = r < cnt;
    SeqCodes c{};
    uint32_t f[3] = {0, 0, 0}, width = 0;
    if (has) {
      SeqView v;
      if constexpr (kOpt)
        v = options & kEncRepeat ? seq_view_repeat<kLong>(seqs, cnt - 1 - r, cs) : seq_view<kLong>(seqs, cnt - 1 - r, cs);
      else v = seq_view<kLong>(seqs, cnt - 1 - r, cs);
      c = sequence_codes(v.ll, v.ml, v.ov);
      const uint32_t moved = tr[cnt - 1 - r];
      for (uint32_t k = 0; k < 3; ++k) f[k] = moved >> (9 * k) & 511;
      width = (f[0] >> 6) + (f[1] >> 6) + (f[2] >> 6) + c.llb + c.mlb + c.ofb;
    }
    const uint32_t incl = wave_incl_sum(width, lane);
    uint32_t at = pos + incl - width;
    if (has) {
      win_put(win, at, f[1] & 63, f[1] >> 6);  // OF, ML, LL states; LL, ML, OF extra bits
      at += f[1] >> 6;
      win_put(win, at, f[2] & 63, f[2] >> 6);
      at += f[2] >> 6;
      win_put(win, at, f[0] & 63, f[0] >> 6);
      at += f[0] >> 6;
      win_put(win, at, c.llx, c.llb);
      at += c.llb;
      win_put(win, at, c.mlx, c.mlb);
      at += c.mlb;
      win_put(win, at, c.ofx, c.ofb);
    }
    pos += uint32_t(__shfl(incl, kWave - 1));
  }
  win_room(win, pos, lane);
  if constexpr (kOpt) {
    if (lane == 0) {
      win_put(win, pos, first_state[2], tlog[2]);
      win_put(win, pos + tlog[2], first_state[1], tlog[1]);
      win_put(win, pos + tlog[2] + tlog[1], first_state[0], tlog[0]);
    }
    win_close(win, pos + tlog[0] + tlog[1] + tlog[2], lane);
  } else {
    if (lane == 0) {
      win_put(win, pos, first_state[2], seq_table_log(2));
      win_put(win, pos + 6, first_state[1], seq_table_log(1));
      win_put(win, pos + 11, first_state[0], seq_table_log(0));
    }
    win_close(win, pos + kSeqInitBits, lane);
  }
}

// ---------------------------------------------------------------------------
// place: one wave per frame
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rpp_zstd_enc_place_kernel(const uint64_t* __restrict__ n_bytes, EncodeWs ws,
                                                              ZstdWs zws, uint8_t* d_out,
                                                              const uint64_t* __restrict__ out_offsets,
                                                              uint64_t* out_bytes, uint32_t* flags,
                                                              const int32_t* __restrict__ status) {
  const uint32_t b = blockIdx.x, lane = lane_id();
  if (!*ws.ok || status[b] != RPP_OK) return;
  const uint64_t n = n_bytes[b];
  uint8_t* const out = d_out + out_offsets[b];
  const uint32_t g0 = ws.chunk_base[b], nc = ws.chunk_base[b + 1] - g0;
  uint8_t header[9];
  const uint32_t hb = frame_header(n, header);
  if (lane < hb) out[lane] = header[lane];
  uint32_t run = hb;
  for (uint32_t t = 0; t < nc; t += kWave) {
    const uint32_t c = t + lane;
    const uint32_t size = c < nc ? 3 + zws.size[g0 + c] : 0;
    const uint32_t incl = wave_incl_sum(size, lane);
    if (c < nc) zws.at[g0 + c] = run + incl - size;
    run += uint32_t(__shfl(incl, kWave - 1));
  }
  if (lane == 0) {
    if (n == 0) {  // an empty frame has no chunk to emit its one block
      block_header(out + run, true, kRaw, 0);
      run += 3;
    }
    out_bytes[b] = run;
    flags[b] = run >= n ? 1u : 0u;
  }
}

// ---------------------------------------------------------------------------
// emit: one wave per chunk
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rpp_zstd_enc_emit_kernel(const uint8_t* __restrict__ d_in,
                                                             const uint64_t* __restrict__ in_offsets,
                                                             uint32_t nblocks, EncodeWs ws, ZstdWs zws,
                                                             uint8_t* __restrict__ d_out,
                                                             const uint64_t* __restrict__ out_offsets) {
  const uint32_t g = blockIdx.x, lane = lane_id();
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const uint32_t b = block_of_chunk(ws.chunk_base, nblocks, g);
  const uint32_t cs = (g - ws.chunk_base[b]) * kEncChunk;
  const uint32_t kind = zws.kind[g], size = zws.size[g];
  uint8_t* const o = d_out + out_offsets[b] + zws.at[g];
  if (lane == 0) block_header(o, g + 1 == ws.chunk_base[b + 1], kind, size);
  wave_copy(o + 3, kind == kCompressed ? zws.body + uint64_t(g) * kEncChunk : d_in + in_offsets[b] + cs, size, lane);
}

uint64_t align16(uint64_t v) { return (v + 15) & ~UINT64_C(15); }

struct Stage {
  EncodeWs ws;
  ZstdWs zws;
  const uint64_t* n_bytes;  // the blocks' sizes as the kernels take them
};

template <bool kLong>
void launch_entropy(hipStream_t s, uint32_t mc, const uint8_t* d_in, const uint64_t* d_in_offsets,
                    const uint64_t* d_in_bytes, uint32_t nblocks, const EncodeWs& ws, const ZstdWs& zws,
                    uint32_t options) {
  if (options)
    hipLaunchKernelGGL((rpp_zstd_enc_entropy_kernel<true, kLong>), dim3(mc), dim3(kWave), 0, s, d_in, d_in_offsets,
                       d_in_bytes, nblocks, ws, zws, options);
  else
    hipLaunchKernelGGL((rpp_zstd_enc_entropy_kernel<false, kLong>), dim3(mc), dim3(kWave), 0, s, d_in, d_in_offsets,
                       d_in_bytes, nblocks, ws, zws, options);
}

// The workspace carved, then prep, search and entropy on the stream.  With long_mode the long-distance matcher's
// launches (zstd_long.hip) stand around the search: the entropy kernel and everything behind it then read the
// merged lists in the short lists' place and the sizes in st.n_bytes, where an over-size block is one that the
// prep kernel has refused.
Stage launch_stage(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes, uint32_t nblocks,
                   uint32_t options, uint32_t search, uint32_t long_mode, uint64_t* d_out_bytes, uint32_t* d_flags,
                   int32_t* d_status, uint64_t total_bytes, void* d_workspace, void* stream) {
  const uint64_t mc = rpp_lz4::max_chunks_of(total_bytes, nblocks);
  EncodeWs ws = rpp_lz4::carve_workspace(d_workspace, total_bytes, nblocks);
  uint8_t* p = static_cast<uint8_t*>(d_workspace) + align16(rpp_lz4_encode_workspace_bytes(total_bytes, nblocks));
  ZstdWs zws{};
  zws.lits = p;
  p += mc * kEncChunk;
  zws.body = p;
  p += mc * kEncChunk;
  zws.tr = reinterpret_cast<uint32_t*>(p);
  p += mc * kSeqsPerChunk * sizeof(uint32_t);
  zws.kind = reinterpret_cast<uint32_t*>(p);
  p += align16(4 * mc);
  zws.size = reinterpret_cast<uint32_t*>(p);
  p += align16(4 * mc);
  zws.at = reinterpret_cast<uint32_t*>(p);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!long_mode) {
    rpp_lz4::launch_search(d_in, d_in_offsets, d_in_bytes, nblocks, ws, d_out_bytes, d_flags, d_status, search, stream);
    launch_entropy<false>(s, uint32_t(mc), d_in, d_in_offsets, d_in_bytes, nblocks, ws, zws, options);
    return Stage{ws, zws, d_in_bytes};
  }
  p += align16(4 * mc);
  const rpp_zstd_long::LongWs lws = rpp_zstd_long::carve(p, total_bytes, nblocks);
  rpp_zstd_long::launch_prepare(d_in_bytes, nblocks, lws, stream);
  rpp_lz4::launch_search(d_in, d_in_offsets, lws.n_eff, nblocks, ws, d_out_bytes, d_flags, d_status, search, stream);
  rpp_zstd_long::launch_match(d_in, d_in_offsets, nblocks, ws, lws, stream);
  ws.cnt = lws.mcnt;
  ws.seqs = lws.mseqs;
  launch_entropy<true>(s, uint32_t(mc), d_in, d_in_offsets, lws.n_eff, nblocks, ws, zws, options);
  return Stage{ws, zws, lws.n_eff};
}

}  // namespace

rpp_zstd::EntropyStage rpp_zstd::launch_search_entropy(const uint8_t* d_in, const uint64_t* d_in_offsets,
                                                       const uint64_t* d_in_bytes, uint32_t nblocks, uint32_t options,
                                                       uint32_t search, uint32_t long_mode, uint64_t* d_out_bytes,
                                                       uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                                                       void* d_workspace, void* stream) {
  const Stage st = launch_stage(d_in, d_in_offsets, d_in_bytes, nblocks, options, search, long_mode, d_out_bytes, d_flags,
                                d_status, total_bytes, d_workspace, stream);
  return EntropyStage{st.ws, st.zws.size};
}

extern "C" uint64_t rpp_zstd_encode_workspace_bytes(uint64_t total_bytes, uint32_t nblocks) {
  const uint64_t mc = rpp_lz4::max_chunks_of(total_bytes, nblocks);
  return align16(rpp_lz4_encode_workspace_bytes(total_bytes, nblocks)) + 2 * mc * kEncChunk +
         mc * kSeqsPerChunk * sizeof(uint32_t) + 3 * align16(4 * mc);
}

extern "C" uint64_t rpp_zstd_encode_workspace_bytes_long(uint64_t total_bytes, uint32_t nblocks, uint32_t long_mode) {
  const uint64_t base = rpp_zstd_encode_workspace_bytes(total_bytes, nblocks);
  return long_mode ? base + rpp_zstd_long::workspace_bytes(total_bytes, nblocks) : base;
}

extern "C" int rpp_zstd_encode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                     uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets,
                                     uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                                     void* d_workspace, uint64_t workspace_bytes, void* stream) {
  return rpp_zstd_encode_batch_opt(d_in, d_in_offsets, d_in_bytes, nblocks, 0, d_out, d_out_offsets, d_out_bytes, d_flags,
                                   d_status, total_bytes, d_workspace, workspace_bytes, stream);
}

static_assert(RPP_ZSTD_ENC_TABLES == kEncTables && RPP_ZSTD_ENC_REPEAT == kEncRepeat, "the options word");

extern "C" int rpp_zstd_encode_batch_opt(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                         uint32_t nblocks, uint32_t options, uint8_t* d_out,
                                         const uint64_t* d_out_offsets, uint64_t* d_out_bytes, uint32_t* d_flags,
                                         int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                                         uint64_t workspace_bytes, void* stream) {
  return rpp_zstd_encode_batch_search(d_in, d_in_offsets, d_in_bytes, nblocks, options, 0, d_out, d_out_offsets,
                                      d_out_bytes, d_flags, d_status, total_bytes, d_workspace, workspace_bytes, stream);
}

extern "C" int rpp_zstd_encode_batch_search(const uint8_t* d_in, const uint64_t* d_in_offsets,
                                            const uint64_t* d_in_bytes, uint32_t nblocks, uint32_t options,
                                            uint32_t search, uint8_t* d_out, const uint64_t* d_out_offsets,
                                            uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status,
                                            uint64_t total_bytes, void* d_workspace, uint64_t workspace_bytes,
                                            void* stream) {
  return rpp_zstd_encode_batch_long(d_in, d_in_offsets, d_in_bytes, nblocks, options, search, 0, d_out, d_out_offsets,
                                    d_out_bytes, d_flags, d_status, total_bytes, d_workspace, workspace_bytes, stream);
}

static_assert(RPP_ZSTD_LONG_MAX_BLOCK == rpp_zstd_long::kLongMaxBlock, "the long word's largest block");

extern "C" int rpp_zstd_encode_batch_long(const uint8_t* d_in, const uint64_t* d_in_offsets,
                                          const uint64_t* d_in_bytes, uint32_t nblocks, uint32_t options,
                                          uint32_t search, uint32_t long_mode, uint8_t* d_out,
                                          const uint64_t* d_out_offsets, uint64_t* d_out_bytes, uint32_t* d_flags,
                                          int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                                          uint64_t workspace_bytes, void* stream) {
  if ((options & ~kEncOptionsMask) || !rpp_lz4::search_valid(search) || long_mode > 1) return RPP_INVALID_ARGUMENT;
  if (nblocks == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_in_bytes || !d_out || !d_out_offsets || !d_out_bytes || !d_flags || !d_status ||
      !d_workspace || ((uintptr_t)d_workspace & 15))
    return RPP_INVALID_ARGUMENT;
  const uint64_t mc = rpp_lz4::max_chunks_of(total_bytes, nblocks);
  if (mc >= 0x7fffffffu) return RPP_INVALID_ARGUMENT;
  if (workspace_bytes < rpp_zstd_encode_workspace_bytes_long(total_bytes, nblocks, long_mode)) return RPP_OUTPUT_TOO_SMALL;
  const Stage st = launch_stage(d_in, d_in_offsets, d_in_bytes, nblocks, options, search, long_mode, d_out_bytes, d_flags,
                                d_status, total_bytes, d_workspace, stream);
  const EncodeWs& ws = st.ws;
  const ZstdWs& zws = st.zws;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_zstd_enc_place_kernel, dim3(nblocks), dim3(kWave), 0, s, st.n_bytes, ws, zws, d_out,
                     d_out_offsets, d_out_bytes, d_flags, d_status);
  hipLaunchKernelGGL(rpp_zstd_enc_emit_kernel, dim3(uint32_t(mc)), dim3(kWave), 0, s, d_in, d_in_offsets, nblocks, ws, zws,
                     d_out, d_out_offsets);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}
