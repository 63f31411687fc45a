// ricepp_tables.h -- what the decode kernels (ricepp_decode_fused.hip,
// ricepp_decode_rows.hip, ricepp_parse.hip) share: the launch parameters, the
// Rice parse's transfer tables and their copy into LDS, the per-wave LDS
// layout, the state maps with their scan steps, and the fs >= 8 front end
// (w32_count).  g_map_table has internal linkage: one copy per translation
// unit that includes this header.
#pragma once

#include "ricepp_wave.h"

namespace {

struct DecParams {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint64_t* in_bytes;
  uint16_t* out;
  const uint64_t* out_off;
  const uint64_t* n_samples;
  int32_t* status;
  uint32_t nblocks;
  uint32_t bs, cs, be, ulsb;
  uint32_t waves;          // waves (streams) per workgroup
  uint32_t only_fallback;  // decode only streams whose status is kSegFallback
  const uint64_t* units;   // non-null: skip streams split into more than one unit (segmented decode)
};

// ---- transfer tables (built at compile time) ----
// Entry (fs, byte): dwords {map 0-3, map 4-7, term 0-3, term 4-7}: byte s of
// `map` is the state after the byte when entering it in state s (0..7), byte
// s of `term` the bits of the byte that end a code (the '1' closing a unary
// run) on that path.  Entering in state s >= 8 (fs >= 8 only) skips the byte:
// state s - 8, no terminator.
constexpr uint32_t kMapFs = 14;  // fs 0..13 (fs + 1 = 1..14 is a Rice header)
constexpr uint32_t kMapEntries = kMapFs * 256;

struct MapTable {
  uint32_t w[kMapEntries * 4];
};

constexpr MapTable make_map_table() {
  MapTable t{};
  for (uint32_t fs = 0; fs < kMapFs; ++fs) {
    for (uint32_t b = 0; b < 256; ++b) {
      uint32_t m[2] = {0, 0}, tm[2] = {0, 0};
      for (uint32_t s = 0; s < 8; ++s) {
        uint32_t c = s, mask = 0, ex = 0;
        for (;;) {
          const uint32_t rest = b >> c;
          if (rest == 0) {  // the unary search runs into the next byte
            ex = 0;
            break;
          }
          const uint32_t tp = c + (uint32_t)__builtin_ctz(rest);
          mask |= 1u << tp;
          c = tp + 1 + fs;  // skip the terminator and fs remainder bits
          if (c >= 8) {
            ex = c - 8;
            break;
          }
        }
        m[s >> 2] |= ex << (8 * (s & 3));
        tm[s >> 2] |= mask << (8 * (s & 3));
      }
      const uint32_t e = (fs * 256 + b) * 4;
      t.w[e] = m[0];
      t.w[e + 1] = m[1];
      t.w[e + 2] = tm[0];
      t.w[e + 3] = tm[1];
    }
  }
  return t;
}

__device__ const MapTable g_map_table = make_map_table();

// The transfer tables into LDS, eight 16-byte loads in flight per lane (a
// one-wave workgroup -- small batches -- copies the 56 KiB in 7 round trips
// instead of 56).  The caller synchronises.
__device__ __forceinline__ void copy_tables(uint4* dsm) {
  const uint4* gt = reinterpret_cast<const uint4*>(g_map_table.w);
  const uint32_t bd = blockDim.x;
  uint32_t i = threadIdx.x;
  for (; i + 7 * bd < kMapEntries; i += 8 * bd) {
    uint4 v[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) v[k] = gt[i + k * bd];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) dsm[i + k * bd] = v[k];
  }
  for (; i < kMapEntries; i += bd) dsm[i] = gt[i];
}

constexpr uint32_t kSegBits = 24;                // bits per lane segment (3 table bytes)
constexpr uint32_t kWinBits = kWave * kSegBits;  // bits per window
constexpr uint32_t kRingWords = 1024;            // per-stream LDS ring of the compressed stream (4 KiB)
constexpr uint32_t kRingMask = kRingWords - 1;
constexpr uint32_t kChunkWords = 4 * kWave;      // refill unit: 16 B per lane
constexpr uint32_t kAhead = 288;                 // words kept resident ahead of the read position
constexpr uint32_t kDecMaxWaves = 16;            // waves per workgroup (one table copy each)
constexpr uint32_t kRingPad = 64;               // ring words 0..63 mirrored after the ring end
constexpr uint32_t kListDump = 512;            // list slot written by masked-off lanes
constexpr uint32_t kListWords = kListDump + 24;  // terminator positions of one sub-block (bs <= 512), dump pairs (MT <= 12)
constexpr uint32_t kListLead = 4;  // words before a decode list: pair -1 = (0, 0), a_(-1) of the fast loop's deltas
constexpr uint32_t kWaveLdsWords = kRingWords + kRingPad + kListLead + kListWords;
constexpr uint32_t kTabBytes = kMapEntries * 16;

__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return readlane(v, kWave - 1); }

// ---- state maps ----
// An 8-entry map (states 0..7) is 8 bytes; byte s = image of s.  g after f
// (apply f first): byte s of the result = g[f[s]] = v_perm_b32(g.hi, g.lo, f).
constexpr uint32_t kId0 = 0x03020100u, kId1 = 0x07060504u, kId2 = 0x0B0A0908u, kId3 = 0x0F0E0D0Cu;
constexpr uint32_t kSelByte0 = 0x0C0C0C00u;  // v_perm selector: byte 0 = index, bytes 1-3 = 0

struct Map8 {
  uint32_t lo, hi;
};
__device__ __forceinline__ Map8 comp8(Map8 g, Map8 f) {
  return Map8{__builtin_amdgcn_perm(g.hi, g.lo, f.lo), __builtin_amdgcn_perm(g.hi, g.lo, f.hi)};
}
template <int Ctrl, int RowMask = 0xF>
__device__ __forceinline__ Map8 scan_step8(Map8 m) {
  const Map8 d{dpp_keep<Ctrl, RowMask>(kId0, m.lo), dpp_keep<Ctrl, RowMask>(kId1, m.hi)};
  return comp8(m, d);
}

// One scan step as two DPP moves into persistent registers: lanes without a
// source (row_shr: the first lanes of each row; row_bcast: the rows the row
// mask leaves out; wave_shr: lane 0) are not written by a DPP move without
// bound_ctrl, so they keep the identity map the register was initialised
// with -- no mask, no vcc.  s_nop 1: a DPP read of a VGPR written by the
// previous VALU instruction needs two wait states.
#define RPP_SCAN8_STEP(NAME, CTRL, RM)                                                           \
  __device__ __forceinline__ Map8 NAME(Map8 m, Map8& keep) {                                              \
    asm("s_nop 1\n\t"                                                                                    \
        "v_mov_b32_dpp %0, %2 " CTRL " row_mask:" RM " bank_mask:0xf\n\t"                                \
        "v_mov_b32_dpp %1, %3 " CTRL " row_mask:" RM " bank_mask:0xf"                                      \
        : "+v"(keep.lo), "+v"(keep.hi)                                                                    \
        : "v"(m.lo), "v"(m.hi));                                                                          \
    return comp8(m, keep);                                                                                \
  }
RPP_SCAN8_STEP(scan8_shr1, "row_shr:1", "0xf")
RPP_SCAN8_STEP(scan8_shr2, "row_shr:2", "0xf")
RPP_SCAN8_STEP(scan8_shr4, "row_shr:4", "0xf")
RPP_SCAN8_STEP(scan8_shr8, "row_shr:8", "0xf")
RPP_SCAN8_STEP(scan8_bc15, "row_bcast:15", "0xa")
RPP_SCAN8_STEP(scan8_bc31, "row_bcast:31", "0xc")
// the persistent destination registers of the six steps and of the final
// shift, initialised to the identity map (opaque to the compiler)
struct ScanRegs {
  Map8 r1, r2, r4, r8, b15, b31, w1;
  // entry-state rounds (w32_count, fs >= 8 loop): lane 0 holds the window's
  // entry state (skip the 4-bit header) in replicated form and is never
  // written
  uint32_t ja, jb;
  __device__ ScanRegs() {
    Map8* all[7] = {&r1, &r2, &r4, &r8, &b15, &b31, &w1};
    for (Map8* x : all) {
      x->lo = kId0;
      x->hi = kId1;
      asm volatile("" : "+v"(x->lo), "+v"(x->hi));
    }
    ja = jb = 0x04040404u;
    asm volatile("" : "+v"(ja), "+v"(jb));
  }
};
// the value of lane l-1 into `keep` (lane 0 keeps its value)
__device__ __forceinline__ uint32_t jshift(uint32_t x, uint32_t& keep) {
  asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(keep) : "v"(x));
  return keep;
}

// fs >= 8: states 0..13 (13 remainder bits still to skip at most).  A state
// is kept replicated in all four bytes of a dword (a v_perm selector that
// yields the looked-up byte in all four bytes).  One byte of the segment:
// states 0..7 go through the byte's 8-entry map (table entry .x/.y); a state
// s >= 8 skips the byte (s - 8).  v_perm gives 0x00 for selectors 8..12 (the
// map bytes are < 0x80) and 0xFF for 13, so s' = max_i16(perm, s - 8) per
// half-word: below 8 the subtraction is negative in both halves.
constexpr int kJacobi16 = 4;  // fixed rounds before the settle check (fs >= 8)
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
  return as_u32(__builtin_bit_cast(us2, __builtin_elementwise_max(__builtin_bit_cast(ss2, a), __builtin_bit_cast(ss2, b))));
}
__device__ __forceinline__ uint32_t byte_step(uint32_t S, uint4 e) {
  return pk_max_i16(__builtin_amdgcn_perm(e.y, e.x, S), S - 0x08080808u);
}
// the byte's terminator bits when entered in state S (none when skipped)
__device__ __forceinline__ uint32_t byte_term(uint32_t S, uint4 e) {
  uint32_t skip;  // all ones for s >= 8 (bit 3; s <= 13)
  asm("v_bfe_i32 %0, %1, 3, 1" : "=v"(skip) : "v"(S));
  return __builtin_amdgcn_perm(e.w, e.z, S) & ~skip;
}
#undef RPP_SCAN8_STEP
// exclusive form: the map of lanes 0..l-1 (identity on lane 0)
__device__ __forceinline__ Map8 shift8_wave(Map8 m, Map8& keep) {
  asm("s_nop 1\n\t"
      "v_mov_b32_dpp %0, %2 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_mov_b32_dpp %1, %3 wave_shr:1 row_mask:0xf bank_mask:0xf"
      : "+v"(keep.lo), "+v"(keep.hi)
      : "v"(m.lo), "v"(m.hi));
  return keep;
}

// 16-entry maps (states 0..15) for fs >= 8.
struct Map16 {
  uint32_t w[4];
};
// bytes of g selected by the 4 byte indices (0..15) in idx
__device__ __forceinline__ uint32_t sel16(const Map16& g, uint32_t idx) {
  const uint32_t i7 = idx & 0x07070707u;
  const uint32_t lo = __builtin_amdgcn_perm(g.w[1], g.w[0], i7);
  const uint32_t hi = __builtin_amdgcn_perm(g.w[3], g.w[2], i7);
  const uint32_t m = idx & 0x08080808u;
  const uint32_t mask = (m << 5) - (m >> 3);  // 0xFF in bytes with index >= 8
  return (hi & mask) | (lo & ~mask);
}
__device__ __forceinline__ Map16 comp16(const Map16& g, const Map16& f) {
  return Map16{{sel16(g, f.w[0]), sel16(g, f.w[1]), sel16(g, f.w[2]), sel16(g, f.w[3])}};
}
template <int Ctrl, int RowMask = 0xF>
__device__ __forceinline__ Map16 scan_step16(const Map16& m) {
  const Map16 d{{dpp_keep<Ctrl, RowMask>(kId0, m.w[0]), dpp_keep<Ctrl, RowMask>(kId1, m.w[1]),
                 dpp_keep<Ctrl, RowMask>(kId2, m.w[2]), dpp_keep<Ctrl, RowMask>(kId3, m.w[3])}};
  return comp16(m, d);
}

// Front end of the fs 8..13 parse (32-bit lane segments): states 0..13 and no
// map scan -- the entry states by jacobi rounds of byte steps (states in
// replicated form, byte_step); the per-byte states of the final round give
// the terminator mask tm of the lane's segment; then the counts (inclusive
// prefix incl, the lanes reaching n codes in finm) and the rider's prefix as
// in the fused fast loop.
// (exit_state: each lane's state after its segment, in replicated form, for a
// parse that continues in the next window)
__device__ __forceinline__ void w32_count(uint4 e0, uint4 e1, uint4 e2, uint4 e3, uint32_t n, uint32_t rider,
                                          ScanRegs& sreg, uint32_t& tm, uint32_t& cnt, uint32_t& incl,
                                          uint64_t& finm, uint32_t& rider_incl, uint32_t* exit_state = nullptr) {
  // lanes up to the first one that ends the sub-block (all when none does)
  auto upto_end = [](uint64_t fm) { return (2ull << (uint32_t)__builtin_ctzll(fm | (1ull << 63))) - 1ull; };
  uint32_t S1, S2, S3;
  auto eval = [&](uint32_t S0) {
    S1 = byte_step(S0, e0);
    S2 = byte_step(S1, e1);
    S3 = byte_step(S2, e2);
    return byte_step(S3, e3);
  };
  auto term_mask = [&](uint32_t S0) {
    const uint32_t a0 = byte_term(S0, e0), a1 = byte_term(S1, e1), a2 = byte_term(S2, e2), a3 = byte_term(S3, e3);
    return __builtin_amdgcn_perm(a3, a2, 0x04000C0Cu) | __builtin_amdgcn_perm(a1, a0, 0x0C0C0400u);
  };
  uint32_t ea = jshift(eval(0u), sreg.ja), eb = 0;
#pragma unroll
  for (int r = 0; r < kJacobi16; ++r) {
    if (r & 1) ea = jshift(eval(eb), sreg.ja);
    else eb = jshift(eval(ea), sreg.jb);
  }
  // the last eval ran on the older of ea / eb; where the round changed
  // nothing its byte states are exact
  uint32_t Sold = (kJacobi16 & 1) ? ea : eb;
  uint32_t Snew = (kJacobi16 & 1) ? eb : ea;
  uint64_t unsettled = __ballot(Sold != Snew);
  tm = term_mask(Sold);
  cnt = __builtin_popcount(tm);
  const uint32_t incl2 = wave_incl_sum(cnt | (rider << 16));
  incl = incl2 & 0xFFFFu;
  rider_incl = incl2 >> 16;
  finm = __ballot(incl >= n);
  // more rounds until every lane up to the sub-block's end is settled (lane
  // l is exact after l rounds: at most 64)
  for (uint32_t guard = 0; (unsettled & upto_end(finm)) && guard < 2 * kWave; ++guard) {
    Sold = Snew;
    Snew = jshift(eval(Sold), sreg.ja);
    unsettled = __ballot(Sold != Snew);
    tm = term_mask(Sold);
    cnt = __builtin_popcount(tm);
    incl = wave_incl_sum(cnt);
    finm = __ballot(incl >= n);
  }
  if (exit_state) *exit_state = eval(Sold);
}

}  // namespace
