// ricepp_decode_fused.hip -- rpp_decode_kernel, the fused ricepp decode (parse
// and values in one kernel, any block size), and its launcher.
//
// One stream per wavefront; a workgroup holds up to kDecMaxWaves waves plus
// one shared copy of the transfer tables (ricepp_tables.h).  Per-stream state
// is wave-uniform (scalar registers, uniform branches).
//
// A Rice sub-block (ricepp/include/ricepp/detail/decode.h:62-71) has no
// index: code i+1 starts where code i ends, so the parse is a finite-state
// machine whose state at any bit boundary is "remainder bits still to skip
// before the next unary search" (sigma, 0..fs).  Per 8-bit unit and fs the
// machine's transfer function (sigma -> sigma', and which bits of the byte
// end a code) is a table lookup (g_map_table, 16 B per (fs, byte)).  A
// sub-block is parsed in windows of 64 lane segments of 24 bits starting at
// its 4-bit header:
//   1. each lane composes the maps of its 3 bytes into one segment map;
//   2. a 6-level DPP scan composes the segment maps along the wave (function
//      composition of 8-entry byte maps is two v_perm_b32), so every lane
//      knows its exact entry state -- no speculation, no re-runs;
//   3. the entry state selects each byte's terminator bits -> a 24-bit
//      terminator mask; popcounts -> DPP prefix sums -> code indices and the
//      lane holding the sub-block's last code (its end is the next header);
//   4. each lane turns its terminators into zig-zag deltas (q = gap from the
//      previous code's end, remainder from its registers) into an LDS tile;
//      a chunk's tile is prefix-summed, pixel-encoded and stored.
// fs >= 8 uses 16-entry maps (sigma up to 13), composed by two v_perm_b32
// per dword plus a byte select.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ricepp_amd.h"
#include "ricepp_internal.h"
#include "ricepp_stats.h"
#include "ricepp_tables.h"

// -DRPP_W16=0 builds the kernel without the 16-bit-segment instance of the
// fast loop (below), for an A/B from one tree.
#ifndef RPP_W16
#define RPP_W16 1
#endif

#ifdef RPP_STATS
__device__ unsigned long long g_dec_stats[16];
#endif

namespace {

// wave priority over the fast loop's parse chain (profiles/r02_prio_ab.jsonl)
constexpr int kParsePrio = 1;

// The narrow instance of the fs 5..7, bs 128 fast loop: 64 lane segments of
// 16 bits.  A sub-block whose 128th terminator lies in these 1024 bits is
// parsed with two table lookups per lane instead of three; one that is longer
// is handed to the 24-bit instance.
constexpr uint32_t kSeg16Bits = 16;
constexpr uint32_t kWin16Bits = kWave * kSeg16Bits;
// Sub-blocks in a row that the 24-bit instance must see fit in kWin16Bits
// before the stream goes back to the narrow instance.  A change of instance
// costs an unpipelined parse (about three sub-block times) each way, a
// fitting sub-block in the 24-bit instance about an eighth of one more than
// in the narrow one.  In Poisson(1000) data 0.26 % of the sub-blocks are long
// and 90 % of them have no other within 16 sub-blocks,
// so any small value serves there; 8 also keeps data whose sub-blocks lie
// around the window's length (a long one in every few) from changing
// instance at each of them: with a share p of long ones a return takes a run
// of 8 fitting ones, (1 - p)^8 of the positions.
constexpr uint32_t kW16Return = 8;

// the table entry at byte offset off16 (16 * entry) from tb
__device__ __forceinline__ uint4 tb_entry(const uint4* tb, uint32_t off16) {
  return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(tb) + off16);
}

// SH: unused_lsb_count != 0 (the pixel write shifts)
template <uint32_t CS, bool SH>
__global__ __launch_bounds__(kWave* kDecMaxWaves) void rpp_decode_kernel(DecParams p) {
  extern __shared__ __attribute__((aligned(16))) uint4 dsm[];
  // ---- this wave's stream, and whether the workgroup has anything to do (the
  //      fallback launch skips most streams: leave before the table copy) ----
  const uint32_t b = blockIdx.x * p.waves + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  bool mine = b < p.nblocks;
  if (mine && p.only_fallback) mine = p.status[b] == rpp_internal::kSegFallback;
  if (mine && p.units && p.units[b] > 1) mine = false;
  if (!__syncthreads_or(mine)) return;
  // ---- the transfer tables, one copy per workgroup ----
  copy_tables(dsm);
  __syncthreads();
  const uint4* tab = dsm;
  const uint32_t lane = lane_id();
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  // (one opaque scalar word offset, so that ring addresses fold into one
  // scalar base)
  uint32_t ring_w = kTabBytes / 4 + wv * kWaveLdsWords;
  asm("" : "+s"(ring_w));
  uint32_t* ring = reinterpret_cast<uint32_t*>(dsm) + ring_w;
  uint32_t* list = ring + kRingWords + kRingPad + kListLead;  // terminator positions of the current sub-block
  if (lane < kListLead) list[(int)lane - (int)kListLead] = 0u;  // (never written again)
  const uint32_t bs = p.bs, be = p.be, ulsb = p.ulsb;
  const uint32_t selbe = be ? 0x02030001u : 0x03020100u;
  const uint32_t selpack = be ? 0x04050001u : 0x05040100u;  // v_perm(hi, lo): pack two samples (+ swap)
  const uint32_t lane24 = kSegBits * lane;
  const uint32_t lane16 = kSeg16Bits * lane;
  if (!mine) return;  // no barrier below this point
#ifdef RPP_STATS
  uint32_t stat_acc[16] = {0};
  unsigned long long tprev_;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev_)::"memory");
#endif

  // ---- per-stream setup (wave-uniform) ----
  // Bit positions are 32-bit and relative to `in`, which starts at the
  // 4-aligned word holding the stream's first byte; a stream longer than
  // 2^30 bits (blocks of more than ~2^26 samples: mkdwarfs -S 28..30) is
  // rebased as the parse goes (rebase() below), so any stream the C ABI
  // accepts decodes here.
  int32_t status = RPP_OK;
  uint32_t N = 0, nbytes = 0, mis = 0;
  uint64_t nb_all = 0, lim_all = 0;  // the stream's bytes (+ mis) and readable bits from the original base
  const uint8_t* in = p.in;
  uint16_t* out = p.out;
  {
    const uint64_t n64 = p.n_samples[b];
    const uint64_t ioff = p.in_off[b];
    const uint64_t nb64 = p.in_bytes[b];
    if (n64 % CS != 0 || n64 >= RPP_MAX_STREAM_SAMPLES || nb64 >= (UINT64_C(1) << 32) - 8) {
      status = RPP_INVALID_ARGUMENT;
    } else {
      mis = (uint32_t)(ioff & 3u);
      N = (uint32_t)n64;
      nb_all = nb64 + mis;
      // last readable bit + 1: the reader pulls whole 8-byte packets of the
      // stream (bitstream_reader.h:149-183), so it only throws past this point.
      lim_all = 8u * mis + 64u * ((nb64 + 7u) >> 3);
      in = p.in + (ioff - mis);
      out = p.out + p.out_off[b];
    }
  }
  const bool aligned16 = ((uintptr_t)in & 15u) == 0;
  nbytes = (uint32_t)nb_all;
  uint32_t lim = (uint32_t)min(lim_all, (uint64_t)0xFFFFFFFFu);
  uint64_t base_w = 0;  // words `in` has moved by
  const uint32_t chunk_len = CS * bs;
  const uint32_t nchunks = status == RPP_OK ? (N + chunk_len - 1) / chunk_len : 0u;

  // ---- LDS ring of the stream's words: words [fill_w - kRingWords, fill_w)
  //      are resident.  Steady state: at the end of an iteration, a chunk of
  //      256 words lying wholly inside the input is requested by
  //      global_load_lds (no registers, nothing for the compiler to wait on);
  //      it is retired (vmcnt(0), by then long complete) a few iterations
  //      later, and only then counted resident.  ensure() is the synchronous
  //      path (start-up, the zero-padded tail, long sub-blocks). ----
  uint32_t fill_w = 0;
  bool pend = false;  // a requested chunk is in flight
  // vector-memory instructions known to be issued after the pending request
  // (the fast loop's output stores; elsewhere reset to 0 = unknown), so that
  // retiring it need not wait for the stores
  uint32_t vm_after = 0;
  auto retire = [&]() {
    if (pend) {
      vm_wait_all_but(vm_after);
      fill_w += kChunkWords;
      pend = false;
    }
  };
  auto refill_sync = [&]() {  // appends 256 words (zero past the input) synchronously
    const uint32_t w = fill_w + 4 * lane;
    uint4 v;
    if (aligned16 && 4 * w + 16 <= nbytes) {
      v = *reinterpret_cast<const uint4*>(in + 4 * w);
    } else {
      v = make_uint4(stream_word(in, nbytes, w), stream_word(in, nbytes, w + 1), stream_word(in, nbytes, w + 2),
                     stream_word(in, nbytes, w + 3));
    }
    *reinterpret_cast<uint4*>(&ring[w & kRingMask]) = v;
    if ((w & kRingMask) < kRingPad) *reinterpret_cast<uint4*>(&ring[kRingWords + (w & kRingMask)]) = v;
    fill_w += kChunkWords;
  };
  auto request = [&]() {  // asynchronous 256-word chunk (only wholly inside the input)
    if (4u * (fill_w + kChunkWords) > nbytes) return;
    // m0 such that lane l lands at ring slot + 16 l (4 l)
    const uint32_t slot = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)&ring[fill_w & kRingMask]);
    const uint8_t* src = in + 4u * fill_w;
    if (aligned16) {
      glds16(src + 16u * lane, slot);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) glds4(src + 256u * q + 4u * lane, slot + 256u * q);
    }
    if ((fill_w & kRingMask) == 0)  // the mirror of words 0..63
      glds4(src + 4u * lane, __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)&ring[kRingWords]));
    pend = true;
    vm_after = 0;
  };
  refill_sync();
  refill_sync();
  lds_fence();
  // keeps words [w, w + kAhead) of the stream resident
  auto ensure = [&](uint32_t w) {
    if (fill_w < w + kAhead) {
      retire();
      while (fill_w < w + kAhead) refill_sync();
      lds_fence();
    }
  };
  // words w, w + 1, w + 2 are contiguous in LDS thanks to the mirror
  auto wptr = [&](uint32_t w) -> const uint32_t* { return ring + (w & kRingMask); };
  auto peek32 = [&](uint32_t pos) -> uint32_t {
    const uint32_t* q = wptr(pos >> 5);
    return __builtin_amdgcn_alignbit(q[1], q[0], pos & 31u);
  };

  // codec.h:69-74,81-86: the 16-bit initial value of each component
  uint32_t last0 = 0, last1 = 0;
  uint32_t P = 8 * mis + 16 * CS;
  // moves `in` forward by a multiple of the ring's size below P (ring slots
  // and the pending chunk keep their places), once P passes 2^30; between
  // two rebases the parse advances less than 2^31 bits (the fast loop stops
  // at 2^31, see ring_bounds), so positions never wrap
  auto rebase = [&]() {
    if (P < (1u << 30)) return;
    const uint32_t sh = ((P >> 5) - kRingWords) & ~(kRingWords - 1u);
    in += 4ull * sh;
    base_w += sh;
    P -= 32u * sh;
    fill_w -= sh;
    nbytes = (uint32_t)(nb_all - 4ull * base_w);
    lim = (uint32_t)min(lim_all - 32ull * base_w, (uint64_t)0xFFFFFFFFu);
  };
  if (status == RPP_OK) {
    if (P > lim) status = RPP_TRUNCATED_INPUT;
    last0 = __builtin_amdgcn_readfirstlane(peek32(8 * mis) & 0xFFFFu);
    if (CS > 1) last1 = __builtin_amdgcn_readfirstlane(peek32(8 * mis + 16) & 0xFFFFu);
  }
  // this lane's 64 bits from bit sb of the stream (its 24-bit segment of a
  // window and what follows it)
  auto load_x = [&](uint32_t sb, uint32_t& xl, uint32_t& xh) {
    const uint32_t* q = wptr(sb >> 5);
    const uint32_t o = sb & 31u;
    const uint32_t a0 = q[0], a1 = q[1], a2 = q[2];
    xl = __builtin_amdgcn_alignbit(a1, a0, o);
    xh = __builtin_amdgcn_alignbit(a2, a1, o);
  };
  // keep the look-ahead: retire the pending chunk once it is needed soon;
  // request the next once the look-ahead drops below 766 words (it
  // overwrites words [fill_w - 1024, fill_w - 768), all below q >> 5, the
  // next bit to be read)
  auto ring_keep = [&](uint32_t q) {
    if (pend && fill_w < (q >> 5) + kAhead + 128) retire();
    if (!pend && fill_w <= (q >> 5) + 766) request();
  };
  const uint32_t nsb = nchunks * CS;
  // sub-blocks the fast loop may take: those of full 128-sample chunks
  // (CS 1: the 2-sample stores must be dword aligned)
  // bs 128: two codes per lane, 2-sample stores (CS 1: dword aligned);
  // bs 16, 32, 64: one code per lane
  const bool fast_bs = bs == 2 * kWave ? (CS == 2 || (((uintptr_t)out) & 3u) == 0)
                                       : (bs == 16 || bs == 32 || bs == 64);
  const uint32_t nsb_fast = fast_bs ? (N / chunk_len) * CS : 0u;
  // one-code-per-lane stores: this lane's byte offset in a sub-block, far
  // out of range (dropped) for lanes past it
  const uint32_t lane_off1 = lane < bs ? 2u * CS * lane : 0x7FFFFFF0u;
  // the stream's output as a raw buffer (N * 2 < 2^28 bytes; stores past it are dropped)
  const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(out, (short)0, (int)(2 * N), 0x00020000);
  ScanRegs sreg;
  // fs 5..7, bs 128: sub-blocks in a row seen to fit the narrow window
  // (wave-uniform; the narrow instance runs while it is at kW16Return)
  uint32_t fit_run = kW16Return;

  for (uint32_t s = 0; s < nsb && status == RPP_OK; ++s) {
    rebase();
    // ---- fast loop (the common case): Rice sub-blocks of 128 codes with fs
    //      5..7 that lie in one window, ring resident.  Straight-line code: at
    //      most 4 terminators per 24-bit segment (codes are >= 6 bits), every
    //      lane owns exactly 2 codes.  Software-pipelined: while sub-block s is
    //      turned into samples, sub-block s+1 is parsed (ring read, table
    //      lookups, scans) in the same basic block, so the LDS latencies and
    //      DPP chains of the two overlap.  Anything else leaves the loop and
    //      takes the general path below for that sub-block. ----
    // MT: terminators a lane segment can hold (codes of >= fs + 1 bits),
    // [LO, HI]: the fs range of this instance (fs 8..13: 32-bit segments)
    // TWO: bs 128, two codes per lane; else bs <= 64, one code per lane
    // W16: the narrow instance (16-bit segments, two table bytes per lane,
    // at most 3 terminators: codes of fs 5..7 are >= 6 bits, so a segment
    // holds terminators at most at t, t + 6, t + 12)
    auto fast = [&]<uint32_t MT, uint32_t LO, uint32_t HI, bool TWO, bool W16 = false>() {
      // fs >= 8: 32-bit lane segments (2048-bit windows), entry states by
      // jacobi rounds over 14 states; else 24-bit segments and 8-state maps
      constexpr bool W32 = LO >= 8;
      static_assert(!W16 || (LO >= 5 && HI <= 7 && MT == 3 && TWO), "16-bit segments: fs 5..7, bs 128");
      constexpr uint32_t SB = W32 ? 32u : W16 ? kSeg16Bits : kSegBits;
      // the 24-bit instance that counts fitting sub-blocks for the return to
      // the narrow one
      constexpr bool kCountFit = RPP_W16 != 0 && !W16 && LO == 5 && HI == 7 && TWO;
      const uint32_t n = TWO ? 2 * kWave : bs;
      const uint4* const list4 = reinterpret_cast<const uint4*>(list);
      uint2* const list2 = reinterpret_cast<uint2*>(list);
      // this lane's 32 bits from bit q + SB lane (24-bit segments: the
      // segment and 8 more, where a terminator in it has its <= 7 remainder
      // bits; 16-bit segments: the segment and 16 more; 32-bit segments: the
      // next 32 bits in xh)
      // (window start word and bit offset are scalar; 24-bit segments: the
      // lane's words lie within 50 words of the window start (16-bit: within
      // 33), inside the ring's mirror; 32-bit segments: the first word index
      // is wrapped per lane, the next two are in the mirror)
      auto seg_bits = [&](uint32_t q, uint32_t& xh) {
        if constexpr (W32) {
          const uint32_t* w = ring + (((q >> 5) + lane) & kRingMask);
          const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
          xh = __builtin_amdgcn_alignbit(w2, w1, q & 31u);
          return __builtin_amdgcn_alignbit(w1, w0, q & 31u);
        } else {
          // (vector addressing from q + lane24 alone: no scalar splitting of
          // q; word wi + 1 <= kRingWords lies in the ring's mirror)
          const uint32_t x = q + (W16 ? lane16 : lane24);
          const uint32_t* w = ring + ((x >> 5) & kRingMask);
          xh = 0u;
          return __builtin_amdgcn_alignbit(w[1], w[0], x);  // (shift x mod 32)
        }
      };
      // the header's fs (scalar; not clamped: a header outside [LO+1, HI+1]
      // -- which the loop then leaves -- makes lookups read other LDS words or
      // out of range, which reads 0; their results are discarded)
      auto fs_of = [](uint32_t h) { return (h & 15u) - 1u; };
      auto header_ok = [](uint32_t h) { return (uint32_t)((h & 15u) - (LO + 1) <= HI - LO); };
      // Parse of the sub-block at bit q: entry states by the map scan,
      // terminators, (a_i, remainder) of code i into list pair i with a_i =
      // terminator position - (q + 4) - i k (the unary part of code i is then
      // a_i - a_(i-1), a_(-1) = 0).  Returns whether the sub-block ends in the
      // window, and its end (the header of the next) in Pe.
      // The count scan also carries a rider: the previous sub-block's delta
      // sums in the high halves (mod 2^16; counts <= 512 stay in the low
      // halves), so that sub-block's value prefix costs no scan of its own.
      // The next window's bits are read from the ring as soon as Pe is known
      // (into xln / xhn), before this sub-block's list writes, so that the
      // read's LDS latency overlaps them instead of opening the next parse.
      auto parse = [&](uint32_t q, uint32_t xl, uint32_t xh, uint32_t fs, uint4 e0, uint4 e1, uint4 e2, uint4 e3,
                       uint32_t& Pe, uint32_t& xln, uint32_t& xhn, uint32_t rider, uint32_t& rider_incl,
                       auto&& mid) -> uint32_t {
        __builtin_amdgcn_s_setprio(kParsePrio);
        const uint32_t k = fs + 1;
        // (off the chain) the end is q + 4 + n k + a_(n-1)
        const uint32_t pe_base = q + 4u + n * k;
        uint32_t tm, cnt, incl;
        uint32_t tot2;  // lane 63's inclusive sums: the window's code count (low), the rider's total (high)
        if constexpr (!W32) {
          const Map8 M01 = comp8(Map8{e1.x, e1.y}, Map8{e0.x, e0.y});  // (also gives byte 2's entry state)
          const Map8 M = W16 ? M01 : comp8(Map8{e2.x, e2.y}, M01);
          // state 4 at the window start: skip the header.  A selector
          // carries the state in byte 0 (the other bytes are 0xFF or copies
          // of byte 0), so each byte's next state comes out of its v_perm as
          // the next selector, with no masking.
          auto scan_sel = [&]() {
            Map8 S = scan8_shr1(M, sreg.r1);
            S = scan8_shr2(S, sreg.r2);
            S = scan8_shr4(S, sreg.r4);
            S = scan8_shr8(S, sreg.r8);
            S = scan8_bc15(S, sreg.b15);
            S = scan8_bc31(S, sreg.b31);
            const Map8 X = shift8_wave(S, sreg.w1);
            return __builtin_amdgcn_perm(X.hi, X.lo, 0xFFFFFF04u);
          };
          // terminator mask of the segment entered in state sel: byte 0 of
          // a0, a1, a2 -> bytes 0, 1, 2 (16-bit segments: of a0, a1)
          auto term_mask = [&](uint32_t sel) {
            const uint32_t a0 = __builtin_amdgcn_perm(e0.w, e0.z, sel);
            const uint32_t a1 = __builtin_amdgcn_perm(e1.w, e1.z, __builtin_amdgcn_perm(e0.y, e0.x, sel));
            if constexpr (W16) return __builtin_amdgcn_perm(a1, a0, 0x0C0C0400u);
            const uint32_t a2 = __builtin_amdgcn_perm(e2.w, e2.z, __builtin_amdgcn_perm(M01.hi, M01.lo, sel));
            return __builtin_amdgcn_perm(a2, __builtin_amdgcn_perm(a1, a0, 0x0C0C0400u), 0x0C040100u);
          };
          tm = term_mask(scan_sel());
          cnt = __builtin_popcount(tm);
          const uint32_t incl2 = wave_incl_sum(cnt | (rider << 16));
          incl = incl2 & 0xFFFFu;
          // (the rider in the high halves is exact whatever the counts: they
          // sum to at most 512 and never carry into it)
          rider_incl = incl2 >> 16;
          tot2 = readlane(incl2, kWave - 1);
        } else {
          uint64_t finm;
          w32_count(e0, e1, e2, e3, n, rider, sreg, tm, cnt, incl, finm, rider_incl);
          tot2 = readlane(incl, kWave - 1) | (readlane(rider_incl, kWave - 1) << 16);
        }
        const uint32_t excl = incl - cnt;
        RPP_TSTAMP(7);
        // terminator positions t0 < t1 < ... in the segment (garbage past
        // cnt)
        uint32_t t[MT];
#pragma unroll
        for (uint32_t j = 0; j < MT; ++j) {
          t[j] = ffbl(tm);
          tm &= tm - 1;
        }
        RPP_TSTAMP(8);
        // pair excl + j for j = MT-1 .. 0, one instruction each (kept apart:
        // a merged ds_write2 would put two j in one instruction): a slot past
        // this lane's codes belongs to a later lane, which writes it in a
        // later instruction (its j is smaller); lanes without terminators or
        // past the sub-block write the unused pairs from 256
        const uint32_t base = cnt != 0 && excl < n ? excl : 256u;
        uint32_t abase = (uint32_t)((int)(SB * lane - 4u) + __mul24((int)base, -(int)k));
        asm volatile("" : "+v"(abase));  // computed once, not per pair
        // the remainder of a terminator at t is bits t+1 .. t+fs of xl: up
        // to bit 23 + 7 = 30 with 24-bit segments, 15 + 7 = 22 with 16-bit
        // ones (the segment's last terminator reaches into the next lane's
        // bits, which xl's 32 hold)
        const uint32_t xr = xl >> 1;
#pragma unroll
        for (int j = MT - 1; j >= 0; --j) {
          // (32-bit segments: the remainder may reach into the next word)
          const uint32_t rem = W32 ? __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(xh, xl, t[j]), 1, fs)
                                   : __builtin_amdgcn_ubfe(xr, t[j], fs);
          list2[base + j] = make_uint2(abase + t[j] - j * k, rem);
          lds_fence();
        }
        // the next sub-block starts after code n-1's remainder: its entry,
        // read back from the list (one broadcast LDS read after the writes,
        // instead of picking the terminator out of the lane that holds it);
        // unused when the sub-block does not end in the window
        // (picking it by readlane out of the lane that holds it measured
        // slower: profiles/r04_decode_ab.jsonl)
        Pe = pe_base + __builtin_amdgcn_readfirstlane(list[2 * (n - 1)]);
        __builtin_amdgcn_s_setprio(0);
        xln = seg_bits(Pe, xhn);
        // (the previous sub-block's stores, off the chain)
        mid(rider_incl, tot2 >> 16);
        RPP_TSTAMP(13);
        return (uint32_t)((tot2 & 0xFFFFu) >= n);
      };
      // codes 2c, 2c+1 of a sub-block on lane c -> zig-zag deltas
      // (decode.h:66-69): d1 and the lane's sum d0 + d1
      // (aprev: a of the code before this lane's first, read from the list;
      // a_(-1) = 0 lies in the list's lead words)
      auto deltas = [&](uint4 tt, uint32_t aprev, uint32_t fs, uint32_t& d1, uint32_t& dsum) {
        if constexpr (TWO) {
          const uint32_t df0 = lshl_or(tt.x - aprev, fs, tt.y), df1 = lshl_or(tt.z - tt.x, fs, tt.w);
          const uint32_t d0 = (df0 >> 1) ^ neg_lsb(df0);
          d1 = (df1 >> 1) ^ neg_lsb(df1);
          dsum = d0 + d1;
        } else {
          // code c on lane c (pair c in tt.x, tt.y); lanes past the
          // sub-block contribute nothing to the prefix
          const uint32_t df = lshl_or(tt.x - aprev, fs, tt.y);
          d1 = (df >> 1) ^ neg_lsb(df);
          dsum = lane < n ? d1 : 0u;
        }
      };
      // inclusive prefix inc of the delta sums -> values -> stored samples of
      // sub-block sx
      // (inc_last: inc of lane 63, the sub-block's delta total)
      auto store = [&](uint32_t d1, uint32_t inc, uint32_t inc_last, uint32_t sx) {
        const uint32_t comp = sx % CS;
        const uint32_t lastc = comp ? last1 : last0;
        const uint32_t v1 = lastc + inc;  // value of sample 2c + 1 (TWO) or c (mod 2^16)
        if constexpr (!TWO) {
          const uint32_t o = SH ? px_write2<true>(v1, selbe, ulsb) : __builtin_amdgcn_perm(v1, v1, selbe);
          __builtin_amdgcn_raw_buffer_store_b16((uint16_t)o, orsrc, lane_off1,
                                                (int)(2 * ((sx / CS) * chunk_len + comp)), 0);
          const uint32_t lnew = lastc + inc_last;
          if (comp) last1 = lnew;
          else last0 = lnew;
          return;
        }
        // samples 2c (low), 2c+1 (high) in stored order: pack and byte-swap
        // in one v_perm when there is no shift
        const uint32_t o = SH ? px_write2<true>(__builtin_amdgcn_perm(v1, v1 - d1, 0x05040100u), selbe, ulsb)
                              : __builtin_amdgcn_perm(v1, v1 - d1, selpack);
        // buffer stores: scalar base + 32-bit lane offset
        if constexpr (CS == 1) {
          __builtin_amdgcn_raw_buffer_store_b32(o, orsrc, 4 * lane, (int)(sx * (2 * n)), 0);
        } else {
          const int sbase = (int)(2 * ((sx / CS) * chunk_len + comp));
          __builtin_amdgcn_raw_buffer_store_b16((uint16_t)o, orsrc, 4 * CS * lane, sbase, 0);
          __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(o >> 16), orsrc, 4 * CS * lane + 2 * CS, sbase, 0);
        }
        // (kept mod 2^32 here, only the low 16 bits count; masked when the
        // loop is left)
        const uint32_t lnew = lastc + inc_last;
        if (comp) last1 = lnew;
        else last0 = lnew;
      };
      // (entry offsets by SDWA byte selects: two VOP2 operations per byte
      // instead of a bit-field extract and a shift-add, both VOP3)
      auto lookups = [&](uint32_t xl, uint32_t fs, uint4& e0, uint4& e1, uint4& e2, uint4& e3) {
        const uint4* tb = tab + 256u * fs;
        e0 = tb_entry(tb, sdwa_byte16<0>(xl));
        e1 = tb_entry(tb, sdwa_byte16<1>(xl));
        if constexpr (!W16) e2 = tb_entry(tb, sdwa_byte16<2>(xl));
        if constexpr (W16) e2 = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (W32) e3 = tb_entry(tb, sdwa_byte16<3>(xl));
        if constexpr (!W32) e3 = make_uint4(0u, 0u, 0u, 0u);
      };

      // Ring bounds, recomputed only when the ring changes: the next window
      // start may be at most pn_limit (resident look-ahead, the header
      // inside the input), and ring_keep has something to do once the
      // window start reaches word trig_w (lim >= P + 4 here).
      // (wave-uniform; readfirstlane keeps them in SGPRs for the loop's
      // scalar tests)
      uint32_t pn_limit, trig_bits;
      auto ring_bounds = [&]() {
        pn_limit = __builtin_amdgcn_readfirstlane(min(min(lim - 4u, 32u * (fill_w - kAhead) + 31u), 1u << 31));
        trig_bits =
            __builtin_amdgcn_readfirstlane(32u * (pend ? fill_w - (kAhead + 127u) : (fill_w > 766u ? fill_w - 766u : 0u)));
      };
      // vector-memory stores per loop iteration (the previous sub-block's
      // samples), counted into vm_after only when the ring is kept
      constexpr uint32_t kStoresPerSub = TWO && CS == 2 ? 2u : 1u;
      uint32_t s_keep = s;
      ring_bounds();
      // prologue: parse sub-block s
      uint32_t Pn;
      uint32_t xh;
      uint32_t xl = seg_bits(P, xh);
      const uint32_t h = __builtin_amdgcn_readfirstlane(xl);
      uint32_t fs = fs_of(h);
      uint4 e0, e1, e2, e3;
      lookups(xl, fs, e0, e1, e2, e3);
      uint32_t unused_rider;
      uint32_t xlB, xhB;  // the window of the sub-block at Pn
      uint32_t ok =
          parse(P, xl, xh, fs, e0, e1, e2, e3, Pn, xlB, xhB, 0u, unused_rider, [](uint32_t, uint32_t) {}) & header_ok(h);
      // a sub-block that does not end in the narrow window: the 24-bit
      // instance takes over (also below, at the loop's own parse)
      if constexpr (W16) {
        if (!ok) fit_run = 0;
      }
      // the look-ahead bound when the window at Pn was read (ring_keep may
      // raise pn_limit afterwards; the window read earlier stays good only
      // below the bound of its time)
      uint32_t pn_read_limit = pn_limit;
      while (ok) {
        // sub-block s at P (ends at Pn) is parsed, its pairs are in the list
        uint4 tt;
        uint32_t aprev;
        if constexpr (TWO) {
          tt = list4[lane];
          aprev = list[4 * lane - 2];
        } else {
          const uint2 t2 = list2[lane];
          tt = make_uint4(t2.x, t2.y, 0u, 0u);
          aprev = list[2 * lane - 2];
        }
        const uint32_t hB = __builtin_amdgcn_readfirstlane(xlB);
        RPP_TSTAMP(1);
        RPP_STAT(0, 1);
        if constexpr (W16) RPP_STAT(3, 1);
        uint32_t d1A, sumA, incA;
        // Does the loop go on to the sub-block at Pn?  (Computed here, tested
        // with the parse's own result after it, so that sub-block s's values
        // still ride on that parse's scan; testing it first, as scalar
        // branches, measured 5 % slower: profiles/r04_decode_ab.jsonl.)
        uint32_t nxt = (uint32_t)(s + 1 < nsb_fast) & (uint32_t)(Pn <= pn_read_limit) & header_ok(hB);
        // sub-block s is Pn - P bits: after kW16Return in a row that the
        // narrow window holds, leave (like at a header of another class) for
        // the narrow instance.  (A sub-block of up to kWin16Bits + fs bits
        // would fit; the bound without fs is one scalar compare.)
        if constexpr (kCountFit) {
          fit_run = Pn - P <= kWin16Bits ? fit_run + 1 : 0u;
          nxt &= (uint32_t)(fit_run < kW16Return);
        }
        pn_read_limit = pn_limit;
        const uint32_t fsB = fs_of(hB);
        lookups(xlB, fsB, e0, e1, e2, e3);
        deltas(tt, aprev, fs, d1A, sumA);
        RPP_TSTAMP(2);
        uint32_t PnB, xlC, xhC;
        ok = parse(Pn, xlB, xhB, fsB, e0, e1, e2, e3, PnB, xlC, xhC, sumA, incA,
                   [&](uint32_t inc, uint32_t inc_last) { store(d1A, inc, inc_last, s); });
        ++s;
        P = Pn;
        if constexpr (W16) {
          if (!ok) fit_run = 0;
        }
        if (!(ok & nxt)) {
          if (P > lim) status = RPP_TRUNCATED_INPUT;
          break;
        }
        Pn = PnB;
        fs = fsB;
        xlB = xlC;
        xhB = xhC;
        if (Pn >= trig_bits) {
          vm_after += (s - s_keep) * kStoresPerSub;  // (the stores since the last keep)
          s_keep = s;
          ring_keep(Pn);
          ring_bounds();
        }
        RPP_TSTAMP(15);
      }
    };
    // dispatch on the sub-block's fs class; a loop that stops at a
    // sub-block of the other class hands over to the other loop directly
    while (s < nsb_fast && status == RPP_OK && fill_w >= (P >> 5) + kAhead && P + 4 <= lim) {
      rebase();
      const uint32_t* w = ring + ((P >> 5) & kRingMask);
      const uint32_t h = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(w[1], w[0], P & 31u)) & 15u;
      const uint32_t s0 = s;
      // (fs 1: the fs 1-4 instance, 12 terminators per segment; a stream
      // that mixes fs 1 and 2..4 sub-blocks stays in it)
      if (bs == 2 * kWave) {
#if RPP_W16
        if (h - 6u <= 2u && fit_run >= kW16Return) {
          fast.template operator()<3, 5, 7, true, true>();
          // (no progress: the first sub-block is too long for the narrow
          // window, and fit_run is 0 now)
          if (s == s0 && fit_run < kW16Return) continue;
        } else
#endif
        if (h - 6u <= 2u) fast.template operator()<4, 5, 7, true>();
        else if (h - 3u <= 2u) fast.template operator()<8, 2, 4, true>();
        else if (h - 9u <= 5u) fast.template operator()<4, 8, 13, true>();
        else if (h == 2u) fast.template operator()<12, 1, 4, true>();
      } else {
        if (h - 6u <= 2u) fast.template operator()<4, 5, 7, false>();
        else if (h - 3u <= 2u) fast.template operator()<8, 2, 4, false>();
        else if (h - 9u <= 5u) fast.template operator()<4, 8, 13, false>();
        else if (h == 2u) fast.template operator()<12, 1, 4, false>();
      }
      last0 &= 0xFFFFu;
      last1 &= 0xFFFFu;
      if (s == s0) break;  // no progress: the general path takes this sub-block
    }
    if (s >= nsb || status != RPP_OK) break;
    // ---- general path: one sub-block of any kind ----
    vm_after = 0;
    const uint32_t comp = s % CS;
    const uint32_t cbase = (s / CS) * chunk_len;
    const uint32_t n = min(N - cbase, chunk_len) / CS;  // samples per component sub-block
    RPP_TSTAMP(4);
    ensure(P >> 5);
    // decode.h:60: 4-bit fs+1 header
    if (P + 4 > lim) {
      status = RPP_TRUNCATED_INPUT;
      break;
    }
    uint32_t xl, xh;
    load_x(P + kSegBits * lane, xl, xh);
    const uint32_t fsp1 = __builtin_amdgcn_readfirstlane(xl) & 15u;
    const uint32_t P4 = P + 4;
    uint16_t* dst = out + cbase + comp;  // sample i of this sub-block at dst[CS * i]
    const bool dw = CS == 1 && (((uintptr_t)dst) & 3u) == 0;
    // stores the packed stored-order samples i0 (low), i0 + 1 (high) of the
    // sub-block (i0 even)
    auto put2 = [&](uint32_t i0, uint32_t o, bool ok0, bool ok1) {
      if (dw && ok1) {
        *reinterpret_cast<uint32_t*>(dst + i0) = o;
      } else {
        if (ok0) dst[CS * i0] = (uint16_t)o;
        if (ok1) dst[CS * (i0 + 1)] = (uint16_t)(o >> 16);
      }
    };
    RPP_STAT(6, 1);
    RPP_TSTAMP(5);
    if (fsp1 == 0) {
      // decode.h:79-80: every sample = write(last)
      const uint32_t v = px_write(comp ? last1 : last0, be, ulsb) * 0x10001u;
      for (uint32_t i0 = 2 * lane; i0 < n; i0 += 2 * kWave) put2(i0, v, true, i0 + 1 < n);
      P = P4;
    } else if (fsp1 == 15) {
      // decode.h:72-77: raw stored values; last = read(last sample)
      if ((uint64_t)P4 + 16ull * n > lim) {
        status = RPP_TRUNCATED_INPUT;
        break;
      }
      for (uint32_t i0 = 2 * lane; i0 < n; i0 += 2 * kWave) {
        put2(i0, peek32(P4 + 16 * i0), true, i0 + 1 < n);
      }
      const uint32_t lv = __builtin_amdgcn_readfirstlane(px_read(peek32(P4 + 16 * (n - 1)) & 0xFFFFu, be, ulsb));
      if (comp) last1 = lv;
      else last0 = lv;
      P = P4 + 16 * n;
    } else {
      // decode.h:62-71: n Rice codes with fs = fsp1 - 1
      const uint32_t fs = fsp1 - 1;
      const uint32_t k = fsp1;
      const uint32_t fmask = (1u << fs) - 1u;
      const uint4* tb = tab + 256u * fs;
      // ---- codes [xdone, m) -> zig-zag deltas (decode.h:66-69) -> values,
      //      2 per lane (m even or m == n) ----
      uint32_t acc = comp ? last1 : last0, start = P4, xdone = 0;  // start: first bit of code xdone's unary run
      // a code left over by an odd count when the parse moves to the next window: its remainder, read while
      // the ring still holds it (the run that follows may be longer than the ring keeps)
      uint32_t held_i = 0xFFFFFFFFu, held_r = 0;
      auto extract = [&](uint32_t m) {
        for (; xdone < m; xdone += 2 * kWave) {
          const uint32_t i0 = xdone + 2 * lane;
          const bool ok0 = i0 < m, ok1 = i0 + 1 < m;
          const uint2 tt = *reinterpret_cast<const uint2*>(&list[min(i0, kListDump - 2)]);
          const uint32_t t0 = tt.x, t1 = ok1 ? tt.y : t0;
          const uint32_t st0 = dpp_keep<kDppWaveShr1>(start, t1 + k);  // end of code i0 - 1
          const uint32_t r0 = i0 == held_i ? held_r : peek32(t0 + 1) & fmask, r1 = peek32(t1 + 1) & fmask;
          const uint32_t df0 = ((t0 - st0) << fs) | r0, df1 = ((t1 - t0 - k) << fs) | r1;
          const uint32_t d0 = ok0 ? (df0 >> 1) ^ (0u - (df0 & 1u)) : 0u;
          const uint32_t d1 = ok1 ? (df1 >> 1) ^ (0u - (df1 & 1u)) : 0u;
          const uint32_t inc = wave_incl_sum(d0 + d1);
          const uint32_t v1 = acc + inc;  // value of sample i0 + 1 (mod 2^16)
          put2(i0, px_write2<true>(((v1 - d1) & 0xFFFFu) | (v1 << 16), selbe, ulsb), ok0, ok1);
          acc += wave_last(inc);
          start = wave_last(t1) + k;
        }
        xdone = m;
        start = __builtin_amdgcn_readfirstlane(list[m - 1]) + k;
      };
      // ---- parse: the terminator position of code i -> list[i] ----
      // q0: first bit of the window; s0: state at q0 (4 = skip the header);
      // done: codes before the window
      uint32_t q0 = P, s0 = 4, done = 0;
      for (;;) {
        RPP_STAT(0, 1);
        const uint32_t sb = q0 + kSegBits * lane;
        // 1. byte transfer functions
        const uint4 e0 = tb[xl & 0xFFu], e1 = tb[__builtin_amdgcn_ubfe(xl, 8, 8)],
                    e2 = tb[__builtin_amdgcn_ubfe(xl, 16, 8)];
        RPP_TSTAMP(10);
        uint32_t tm, xexit;
        if (fs < 8) {
          // 2. segment map, scan along the wave, entry state
          Map8 M = comp8(Map8{e2.x, e2.y}, comp8(Map8{e1.x, e1.y}, Map8{e0.x, e0.y}));
          M = scan_step8<kDppRowShr1>(M);
          M = scan_step8<kDppRowShr2>(M);
          M = scan_step8<kDppRowShr4>(M);
          M = scan_step8<kDppRowShr8>(M);
          M = scan_step8<kDppRowBcast15, 0xA>(M);
          M = scan_step8<kDppRowBcast31, 0xC>(M);
          const Map8 X{dpp_keep<kDppWaveShr1>(kId0, M.lo), dpp_keep<kDppWaveShr1>(kId1, M.hi)};
          // 3. terminators of this lane's segment
          uint32_t sel = __builtin_amdgcn_perm(X.hi, X.lo, s0 | kSelByte0) | kSelByte0;
          const uint32_t t0 = __builtin_amdgcn_perm(e0.w, e0.z, sel);
          sel = __builtin_amdgcn_perm(e0.y, e0.x, sel) | kSelByte0;
          const uint32_t t1 = __builtin_amdgcn_perm(e1.w, e1.z, sel);
          sel = __builtin_amdgcn_perm(e1.y, e1.x, sel) | kSelByte0;
          const uint32_t t2 = __builtin_amdgcn_perm(e2.w, e2.z, sel);
          xexit = __builtin_amdgcn_perm(e2.y, e2.x, sel);
          tm = t0 | (t1 << 8) | (t2 << 16);
        } else {
          const Map16 b0{{e0.x, e0.y, kId0, kId1}}, b1{{e1.x, e1.y, kId0, kId1}}, b2{{e2.x, e2.y, kId0, kId1}};
          Map16 M = comp16(b2, comp16(b1, b0));
          M = scan_step16<kDppRowShr1>(M);
          M = scan_step16<kDppRowShr2>(M);
          M = scan_step16<kDppRowShr4>(M);
          M = scan_step16<kDppRowShr8>(M);
          M = scan_step16<kDppRowBcast15, 0xA>(M);
          M = scan_step16<kDppRowBcast31, 0xC>(M);
          const Map16 X{{dpp_keep<kDppWaveShr1>(kId0, M.w[0]), dpp_keep<kDppWaveShr1>(kId1, M.w[1]),
                         dpp_keep<kDppWaveShr1>(kId2, M.w[2]), dpp_keep<kDppWaveShr1>(kId3, M.w[3])}};
          uint32_t st = sel16(X, s0) & 0xFFu;
          uint32_t t[3];
          const uint4 ee[3] = {e0, e1, e2};
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const uint32_t sel = st | kSelByte0;
            const bool skip = st >= 8;
            t[j] = skip ? 0u : __builtin_amdgcn_perm(ee[j].w, ee[j].z, sel);
            st = skip ? st - 8 : __builtin_amdgcn_perm(ee[j].y, ee[j].x, sel);
          }
          tm = t[0] | (t[1] << 8) | (t[2] << 16);
          xexit = st;
        }
        RPP_TSTAMP(11);
        // 4. code indices: terminators -> list[done + excl + j]
        const uint32_t cnt = __builtin_popcount(tm);
        const uint32_t incl = wave_incl_sum(cnt);
        const uint32_t excl = incl - cnt;
        const uint32_t need = n - done;
        const uint32_t mine = need > excl ? min(cnt, need - excl) : 0u;
        uint32_t* lp = list + done + excl;
        for (uint32_t j = 0; __any(j < mine); ++j) {
          const uint32_t t = ffbl(tm);
          tm &= tm - 1;
          *(j < mine ? lp + j : list + kListDump) = sb + t;
        }
        RPP_TSTAMP(12);
        if (__ballot(incl >= need)) break;
        // continuation window: the sub-block is longer than kWinBits;
        // turn the codes found so far into samples first (the ring only
        // keeps the recent windows resident)
        done += wave_last(incl);
        if ((done & ~1u) > xdone) {
          lds_fence();
          extract(done & ~1u);
        }
        if ((done & 1u) && held_i != done - 1) {
          lds_fence();
          held_i = done - 1;
          held_r = __builtin_amdgcn_readfirstlane(peek32(list[held_i] + 1)) & fmask;
        }
        s0 = wave_last(xexit);
        q0 += kWinBits;
        if (q0 >= lim) {  // the open unary search would read past the input
          status = RPP_TRUNCATED_INPUT;
          break;
        }
        ensure(q0 >> 5);
        load_x(q0 + kSegBits * lane, xl, xh);
      }
      if (status != RPP_OK) break;
      lds_fence();
      extract(n);
      if (comp) last1 = acc & 0xFFFFu;
      else last0 = acc & 0xFFFFu;
      // the next sub-block starts after code n-1's remainder
      P = __builtin_amdgcn_readfirstlane(list[n - 1]) + k;
      if (P > lim) {
        status = RPP_TRUNCATED_INPUT;
        break;
      }
    }
    RPP_TSTAMP(14);
    ring_keep(P);
  }
  retire();
  if (lane == 0) p.status[b] = status;
#ifdef RPP_STATS
  if (lane == 0)
    for (int i = 0; i < 16; ++i) atomicAdd(&g_dec_stats[i], (unsigned long long)stat_acc[i]);
#endif
}

}  // namespace

#ifdef RPP_STATS
// Diagnostic build only: copies (and optionally clears) the fused decode's loop counters.
extern "C" int rpp_dec_stats_fetch(uint64_t* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dec_stats), sizeof(uint64_t) * 16) != hipSuccess) return RPP_HIP_ERROR;
  if (reset) {
    uint64_t z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_dec_stats), z, sizeof z) != hipSuccess) return RPP_HIP_ERROR;
  }
  return RPP_OK;
}
#endif

namespace rpp_internal {

int launch_decode_fused(const rpp_config* cfg, const uint8_t* d_in, const uint64_t* d_in_offsets,
                        const uint64_t* d_in_bytes, uint32_t nblocks, uint16_t* d_out, const uint64_t* d_out_offsets,
                        const uint64_t* d_n_samples, int32_t* d_status, hipStream_t stream, bool only_fallback,
                        const uint64_t* d_units, uint32_t waves, bool rows) {
  int st = rpp_check_config(cfg);
  if (st != RPP_OK) return st;
  if (nblocks == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_in_bytes || !d_out || !d_out_offsets || !d_n_samples || !d_status)
    return RPP_INVALID_ARGUMENT;
  // one stream per wave; up to kDecMaxWaves waves share one copy of the
  // transfer tables, fewer when the batch cannot fill the 256 CUs anyway
  uint32_t W = std::min<uint32_t>(kDecMaxWaves, std::max<uint32_t>(1, (nblocks + 255) / 256));
  if (waves) W = std::min<uint32_t>(kDecMaxWaves, waves);
  const size_t lds = kTabBytes + (size_t)W * kWaveLdsWords * 4;
  static void (*const kernels[4])(DecParams) = {rpp_decode_kernel<1, false>, rpp_decode_kernel<1, true>,
                                                 rpp_decode_kernel<2, false>, rpp_decode_kernel<2, true>};
  static const hipError_t attr_err =
      set_max_dynamic_lds(kernels, kTabBytes + (size_t)kDecMaxWaves * kWaveLdsWords * 4);
  if (attr_err != hipSuccess) return RPP_HIP_ERROR;
  DecParams p{d_in, d_in_offsets, d_in_bytes, d_out, d_out_offsets, d_n_samples, d_status, nblocks,
              cfg->block_size, cfg->component_stream_count, cfg->big_endian ? 1u : 0u,
              cfg->unused_lsb_count, W, only_fallback ? 1u : 0u, d_units};
  const auto k = kernels[2 * (cfg->component_stream_count - 1) + (cfg->unused_lsb_count ? 1 : 0)];
  if (rows && !only_fallback && !d_units && !waves &&
      (cfg->block_size == 16 || cfg->block_size == 32)) {
    // bs 16 / 32: four streams per wave, then the fused kernel for the
    // streams it left (status kSegFallback)
    st = launch_decode_rows(cfg, d_in, d_in_offsets, d_in_bytes, nblocks, d_out, d_out_offsets, d_n_samples, d_status,
                            stream);
    if (st != RPP_OK) return st;
    p.only_fallback = 1;
  }
  hipLaunchKernelGGL(k, dim3((nblocks + W - 1) / W), dim3(kWave * W), lds, stream, p);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}

}  // namespace rpp_internal
