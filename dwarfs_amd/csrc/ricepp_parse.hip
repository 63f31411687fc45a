// ricepp_parse.hip -- the parse pass of the segmented ricepp decode
// (rpp_decode_batch_ws, stage 1 of 2): rpp_parse_kernel, rpp_seg_guess_kernel
// and their launchers.
//
// The serial part of decoding a stream is finding where each sub-block
// starts: sub-block k+1 begins where the n-th code of sub-block k ends
// (codec.h:103-140, decode.h:42-83).  rpp_parse_kernel does only that, with
// the exact table-driven parse of rpp_decode_kernel (window map scan, count
// scan, the lane holding code n-1) and none of its value extraction, and
// records the start bit of every sub-block's header (plus the end of the last
// one) in sb_pos.  The values are then produced by rpp_extract_kernel
// (ricepp_decode2.hip) with all sub-blocks of all streams in parallel.
//
// Bit positions are relative to the 4-byte-aligned word containing the
// stream's first byte (streams may start at any byte offset): the stream's bit
// 0 is at 8 * (in_off & 3).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "ricepp_amd.h"
#include "ricepp_internal.h"
#include "ricepp_tables.h"

namespace {

struct ParseParams {
  const uint8_t* in;
  const uint64_t* in_off;
  const uint64_t* in_bytes;
  const uint64_t* n_samples;
  const uint64_t* sb_base;  // [nblocks] first sb_pos entry of stream b
  uint32_t* sb_pos;         // [sum(nsb_b + 1)] header start bits, then the end
  int32_t* status;
  uint32_t nblocks;
  uint32_t bs;
  uint32_t waves;  // waves (streams or units) per workgroup
  rpp_internal::SegView sv;  // SEG: the units of the segmented decode
  uint32_t wave_words;       // LDS words per wave (kWaveLdsWords, or more for a long-sub-block guess)
};
// Per-wave LDS of the units' parse: bs >= 256 sub-blocks are 2-8 Kib long, so
// a guess that chains kSpecSteps of them needs ~60-90 Kib of the stream
// staged: such launches run 8 waves per workgroup with twice the words each.
constexpr uint32_t kLongSbBs = 256;
__host__ __device__ constexpr uint32_t parse_wave_words(uint32_t bs) {
  return bs >= kLongSbBs ? 2 * kWaveLdsWords : kWaveLdsWords;
}

// segmented-decode parse diagnostics (rpp_parse_diag_read): cycles in the
// guess, cycles in the chain, sub-blocks parsed, units
// (8..11: the guess's lane-serial steps and wave-parallel tail: cycles,
// cycles, tail sub-blocks, tail windows)
__device__ unsigned long long g_parse_diag[16];
__device__ __forceinline__ uint64_t memtime() {
  uint64_t t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// The end (next header) of the sub-block with its header at bit r of the
// staged words st (relative positions), parsed by the whole wave in 2048-bit
// windows of 32-bit lane segments with exact entry states (w32_count, byte
// maps for any fs): the first window enters after the 4-bit header, a later
// one in the state the previous window's last lane left (sub-blocks longer
// than a window: fs 11-13 with outliers, bs 256 / 512).  Returns `lim` when
// the sub-block runs past lim - 64 (the staged words' end).
__device__ __forceinline__ uint32_t seg_sb_end_wave(const uint32_t* st, const uint4* tab, uint32_t r, uint32_t bs,
                                                    uint32_t lane, const ScanRegs& sreg0, uint32_t lim) {
  const uint32_t* w = st + (r >> 5) + lane;
  uint32_t x = __builtin_amdgcn_alignbit(w[1], w[0], r & 31u);
  const uint32_t v = __builtin_amdgcn_readfirstlane(x) & 15u;
  if (v == 0) return r + 4u;
  if (v == 15) return r + 4u + 16u * bs;
  const uint4* tb = tab + 256u * (v - 1u);
  ScanRegs sreg = sreg0;  // (lane 0's entry state: the header's 4 bits, then the carried state)
  uint32_t base = r, need = bs;
  for (;;) {
    const uint4 e0 = tb[x & 0xFFu], e1 = tb[__builtin_amdgcn_ubfe(x, 8, 8)], e2 = tb[__builtin_amdgcn_ubfe(x, 16, 8)],
                e3 = tb[x >> 24];
    uint32_t tm, cnt, incl, unused, ex;
    uint64_t finm;
    w32_count(e0, e1, e2, e3, need, 0u, sreg, tm, cnt, incl, finm, unused, &ex);
    if (finm != 0) {
      const uint32_t lz = (uint32_t)__builtin_ctzll(finm);
      uint32_t t = readlane(tm, (int)lz);
      const uint32_t rr = need - 1u - (readlane(incl, (int)lz) - readlane(cnt, (int)lz));
      for (uint32_t i = 0; i < rr; ++i) t &= t - 1u;  // (scalar: the rr-th terminator of lane lz)
      return base + 32u * lz + (uint32_t)__builtin_ctz(t) + v;
    }
    need -= readlane(incl, kWave - 1);
    base += 32u * kWave;
    if (base + 32u * kWave + 64u > lim) return lim;
    sreg.ja = sreg.jb = readlane(ex, kWave - 1);
    w = st + (base >> 5) + lane;
    x = __builtin_amdgcn_alignbit(w[1], w[0], base & 31u);
  }
}

// Segmented decode, the first header of a unit (ricepp_internal.h): the
// first candidate bit c in [c_first, 4 + 16 bs) of the staged words `st`
// whose chain of kSpecSteps sub-blocks (each parsed exactly as
// decode.h:42-83 would from there) keeps its header values within a range
// (highest - lowest <= `range`: 3, or 5 in a second search when the first
// finds nothing), with zero headers only in an all-zero chain.
// ricepp output does: the Rice parameter follows the local noise level
// (Poisson data stays on one or two values, 6-bit noise with outliers on fs
// 11..13).  Random bits do not, except through the zero high bits of small
// remainders, which read as chains of small headers -- hence the zero rule (a
// CPU replay of the guess on the generator data: 6 of 60 units unstitchable
// without it, 0 with it).  A chain through other bits survives a step with
// probability ~0.35, so some guesses are wrong: the unit's own parse checks
// the same rule over the first kSpecVerify sub-blocks of its chain and asks
// for the next candidate when it fails.  Candidates a few bits before the
// true header often land on the true chain after one sub-block; the stitch
// accepts those.  Candidates are parsed lane by lane out of LDS, up to four
// chains per lane and three codes per read, 256 candidates at a time; after
// every sub-block the survivors are compacted into `list` (512 words of LDS).
// Long sub-blocks (bs 256 / 512: 2-8 Kib each) do not fit kSpecSteps of them
// in the staged words: a chain that reaches their end after kGuessMinSteps
// sub-blocks is finished (a survivor that is checked no further here).
// A wrong guess costs time, never a wrong result.
constexpr uint32_t kSlotsPerGuess = 4;  // candidates per lane of a chunk (one wave: 256-candidate chunks)
constexpr uint32_t kGuessWaveMax = 12;  // survivors below which seg_guess parses wave-parallel
constexpr uint32_t kGuessMinSteps = 4;  // sub-blocks a chain must pass before the staged words may end it
constexpr uint32_t kGuessFin = 1u << 31;  // (list word 2: the chain is finished)
// (chunk0, chunk_step: this wave's share of the chunks when
// several waves search one unit -- rpp_seg_guess_kernel -- with `best`, the
// lowest survivor any of them found so far, in LDS: a wave stops at chunks
// beyond it)
// (kSlots: candidates per lane of a chunk; the multi-wave search takes
// smaller chunks, so that its waves cover the candidates in more, shorter
// lane-serial passes)
template <uint32_t kSlots = kSlotsPerGuess>
__device__ __forceinline__ uint32_t seg_guess(const uint32_t* st, uint32_t* list, uint32_t end_rel, uint32_t bs,
                                              uint32_t lane, uint32_t c_first, uint32_t range, const uint4* tab,
                                              uint32_t chunk0 = 0, uint32_t chunk_step = 1, uint32_t* best = nullptr,
                                              uint32_t steps = rpp_internal::kSpecSteps) {
  using rpp_internal::kSegNone;
  const uint32_t maxsb = 4u + 16u * bs;
  auto peek = [&](uint32_t r) {
    const uint32_t* w = st + (r >> 5);
    return __builtin_amdgcn_alignbit(w[1], w[0], r & 31u);
  };
  uint32_t n_chunks = 0, n_steps = 0, n_slotsteps = 0;
  auto found = [&](uint32_t m) {
    if (best && lane == 0) atomicMin(best, m);
    return m;
  };
  for (uint32_t c0 = c_first + kSlots * kWave * chunk0; c0 < maxsb; c0 += kSlots * kWave * chunk_step) {
    if (best && c0 >= __builtin_amdgcn_readfirstlane(__hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)))
      break;
    ++n_chunks;
    const uint64_t t_serial = memtime();
    bool tailed = false;
    uint32_t cur[kSlots], org[kSlots], rng[kSlots];  // rng: lowest header | highest << 4
    bool alive[kSlots], fin[kSlots];
    uint32_t nslots = kSlots;
#pragma unroll
    for (uint32_t i = 0; i < kSlots; ++i) {
      org[i] = c0 + lane + kWave * i;
      alive[i] = org[i] < maxsb && org[i] + 4 <= end_rel;
      fin[i] = false;
      cur[i] = alive[i] ? org[i] : 0u;
      rng[i] = 0x0Fu;
    }
    for (uint32_t step = 0; step < steps; ++step) {
      ++n_steps;
      n_slotsteps += nslots;
      const bool may_finish = step >= kGuessMinSteps;
      uint32_t fsv[kSlots];
      bool rice[kSlots];
#pragma unroll
      for (uint32_t i = 0; i < kSlots; ++i) {
        rice[i] = false;
        fsv[i] = 0;
        if (i < nslots && !fin[i]) {
          const uint32_t v = peek(cur[i]) & 15u;
          const uint32_t lo = min(rng[i] & 15u, v), hi = max(rng[i] >> 4, v);
          rng[i] = lo | (hi << 4);
          const uint32_t nc = cur[i] + (v == 15 ? 4u + 16u * bs : 4u);
          // (zero sub-blocks only in an all-zero run: chains of small
          // headers through the zero high bits of small remainders are the
          // common false survivors)
          const bool inside = nc + 4 <= end_rel;
          alive[i] = alive[i] && hi - lo <= range && (lo != 0 || hi == 0) && (inside || may_finish);
          fin[i] = alive[i] && !inside;
          rice[i] = alive[i] && !fin[i] && v - 1u < 14u;
          fsv[i] = v - 1;
          cur[i] = alive[i] && !fin[i] ? nc : 0u;
        }
      }
      // the codes of the Rice sub-blocks, branch-free, up to three per LDS
      // read (a 64-bit window; codes 2 and 3 when the previous one ends in
      // the first 32 bits).  A window without a terminator (a unary run past
      // 32 bits, rare) advances 32 bits and consumes no code.
      uint32_t ncode[kSlots];
#pragma unroll
      for (uint32_t i = 0; i < kSlots; ++i) ncode[i] = 0;
      auto codes = [&](uint32_t i) {
        const uint32_t* w = st + (cur[i] >> 5);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        const uint32_t sh = cur[i] & 31u;
        const uint32_t x = __builtin_amdgcn_alignbit(w1, w0, sh), xn = __builtin_amdgcn_alignbit(w2, w1, sh);
        const uint32_t k1 = fsv[i] + 1, left = bs - ncode[i];
        const uint32_t e1 = ffbl(x) + k1;
        const uint32_t y = __builtin_amdgcn_alignbit(xn, x, e1 & 31u);
        const bool c2 = e1 < 32 && y != 0 && left >= 2;
        const uint32_t e2 = e1 + ffbl(y) + k1;
        const uint32_t z = __builtin_amdgcn_alignbit(xn, x, e2 & 31u);
        const bool c3 = c2 && e2 < 32 && z != 0 && left >= 3;
        const uint32_t e3 = e2 + ffbl(z) + k1;
        const bool zero = x == 0;
        const uint32_t adv = zero ? 32u : c3 ? e3 : c2 ? e2 : e1;
        const uint32_t n = zero ? 0u : 1u + (c2 ? 1u : 0u) + (c3 ? 1u : 0u);
        const bool r = rice[i];
        const uint32_t nxt = cur[i] + adv;
        const bool bad = r && nxt + 4 > end_rel;
        cur[i] = r ? (bad ? 0u : nxt) : cur[i];
        ncode[i] += r ? n : 0u;
        alive[i] = alive[i] && (!bad || may_finish);
        fin[i] = fin[i] || (bad && may_finish);
        rice[i] = r && !bad && ncode[i] < bs;
      };
      static_assert(kSlots == 2 || kSlots == 4, "seg_guess: 2 or 4 candidates per lane");
      for (;;) {
        bool more = rice[0] || rice[1];
        if constexpr (kSlots == 4) more = more || rice[2] || rice[3];
        if (__ballot(more) == 0) break;
        codes(0);
        if (nslots > 1) codes(1);
        if constexpr (kSlots == 4) {
          if (nslots > 2) codes(2);
          if (nslots > 3) codes(3);
        }
      }
      // compact the survivors (in candidate order) into the first slots
      uint32_t cnt = 0;
      bool all_fin = true;
#pragma unroll
      for (uint32_t i = 0; i < kSlots; ++i) {
        if (i < nslots) {
          const uint64_t m = __ballot(alive[i]);
          const uint32_t at = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
          if (alive[i]) {
            list[2 * at] = cur[i];
            list[2 * at + 1] = org[i] | (rng[i] << 16) | (fin[i] ? kGuessFin : 0u);
          }
          cnt += (uint32_t)__builtin_popcountll(m);
          all_fin = all_fin && __ballot(alive[i] && !fin[i]) == 0;
        }
      }
      lds_fence();
      if (cnt == 0 || all_fin) break;
      // few survivors: the remaining steps survivor by survivor (candidate
      // order) with the wave-parallel parse, ~1/20 of a lane-serial step each
      // (any bs: codes past its 2048-bit window are walked one by one)
      if (cnt <= kGuessWaveMax && step + 1 < steps) {
        const uint64_t t_tail = memtime();
        uint32_t n_tail = 0;
        tailed = true;
        if (lane == 0) atomicAdd(&g_parse_diag[8], (unsigned long long)(t_tail - t_serial));
        ScanRegs sreg;
        for (uint32_t idx = 0; idx < cnt; ++idx) {
          uint32_t cur = __builtin_amdgcn_readfirstlane(list[2 * idx]);
          const uint32_t o = __builtin_amdgcn_readfirstlane(list[2 * idx + 1]);
          uint32_t lo = (o >> 16) & 15u, hi = (o >> 20) & 15u;
          bool ok = true;
          for (uint32_t st2 = step + 1; st2 < steps && ok && !(o & kGuessFin); ++st2) {
            const uint32_t* w = st + (cur >> 5);
            const uint32_t v = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(w[1], w[0], cur & 31u)) & 15u;
            lo = min(lo, v);
            hi = max(hi, v);
            const uint32_t nc = seg_sb_end_wave(st, tab, cur, bs, lane, sreg, end_rel);
            ++n_tail;
            // (accepting sub-blocks longer than the window as a finished chain,
            // before the walk past it existed, let false chains through random
            // bits survive: 150 reruns per 16 MiB generator stream)
            ok = hi - lo <= range && (lo != 0 || hi == 0) && nc != rpp_internal::kSegNone;
            if (ok && nc + 4 > end_rel) {  // the staged words end: finished (as above) after kGuessMinSteps
              ok = st2 >= kGuessMinSteps;
              break;
            }
            cur = nc;
          }
          if (ok) {
            if (lane == 0) {
              atomicAdd(&g_parse_diag[9], (unsigned long long)(memtime() - t_tail));
              atomicAdd(&g_parse_diag[10], (unsigned long long)n_tail);
              atomicAdd(&g_parse_diag[4], (unsigned long long)n_chunks);
              atomicAdd(&g_parse_diag[5], (unsigned long long)n_steps);
              atomicAdd(&g_parse_diag[6], (unsigned long long)n_slotsteps);
            }
            return found(o & 0xFFFFu);
          }
        }
        if (lane == 0) {
          atomicAdd(&g_parse_diag[9], (unsigned long long)(memtime() - t_tail));
          atomicAdd(&g_parse_diag[10], (unsigned long long)n_tail);
        }
#pragma unroll
        for (uint32_t i = 0; i < kSlots; ++i) alive[i] = false;  // (none survived)
        break;
      }
      nslots = (cnt + kWave - 1) / kWave;
#pragma unroll
      for (uint32_t i = 0; i < kSlots; ++i) {
        const uint32_t idx = kWave * i + lane;
        alive[i] = idx < cnt;
        cur[i] = alive[i] ? list[2 * idx] : 0u;
        const uint32_t o = alive[i] ? list[2 * idx + 1] : 0u;
        org[i] = o & 0xFFFFu;
        rng[i] = (o >> 16) & 0xFFu;
        fin[i] = (o & kGuessFin) != 0;
      }
      lds_fence();
    }
    if (!tailed && lane == 0) atomicAdd(&g_parse_diag[8], (unsigned long long)(memtime() - t_serial));
    uint32_t m = kSegNone;
#pragma unroll
    for (uint32_t i = 0; i < kSlots; ++i)
      if (alive[i]) m = min(m, org[i]);
    m = wave_min_u32(m);
    if (m != kSegNone || c0 + kSlots * kWave >= maxsb) {
      if (lane == 0) {
        atomicAdd(&g_parse_diag[4], (unsigned long long)n_chunks);
        atomicAdd(&g_parse_diag[5], (unsigned long long)n_steps);
        atomicAdd(&g_parse_diag[6], (unsigned long long)n_slotsteps);
      }
      if (m != kSegNone) return found(m);
    }
  }
  return kSegNone;
}

// One wave per unit of rpp_internal::SegView (SEG = true, the only
// instantiation launched: launch_parse_seg): a unit of a split stream
// (ricepp_internal.h) records into its position list / overshoot list; a
// stream of one unit is left to the fused kernel.  (SEG = false, one wave per
// stream writing sb_pos, was the whole-batch two-stage decode, measured
// slower than the fused kernel on every workload and removed.)
template <uint32_t CS, bool SEG>
__global__ __launch_bounds__(kWave* kDecMaxWaves) void rpp_parse_kernel(ParseParams p) {
  using namespace rpp_internal;
  extern __shared__ __attribute__((aligned(16))) uint4 dsm[];
  if constexpr (SEG) {
    // rerun passes (one wave per workgroup): most units have nothing to do;
    // leave before loading the tables
    if (p.sv.pass != 0) {
      const uint32_t w = blockIdx.x * p.waves + threadIdx.x / kWave;
      if (w >= (uint32_t)p.sv.unit_base[p.nblocks] || p.sv.ustate[kUsWords * w + kUsRerun] == kSegNone) return;
    }
  }
  {
    copy_tables(dsm);
  }
  __syncthreads();
  const uint4* tab = dsm;
  const uint32_t lane = lane_id();
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  uint32_t ring_w = kTabBytes / 4 + wv * p.wave_words;
  asm("" : "+s"(ring_w));
  uint32_t* ring = reinterpret_cast<uint32_t*>(dsm) + ring_w;
  const uint32_t bs = p.bs;
  const uint32_t lane24 = kSegBits * lane;
  // guess staging: the wave's words but the 540 of the candidate list
  const uint32_t stage_w = p.wave_words - (kListLead + kListWords);
  // One work item: a stream (SEG = false) or a unit.  Pass 0 of the
  // segmented decode takes units from a queue (one 16-wave workgroup per CU,
  // each wave unit after unit), so that every CU parses whatever the stream
  // mix and the side-stream fused launch leave it; the other launches map one
  // item per wave.
  auto work = [&](const uint32_t wid) {
    // ---- the stream (and, SEG, the unit) of this wave ----
    uint32_t b = wid, u = 0, u0 = 0, ju = 0, nunits = 1;
    if constexpr (SEG) {
      if (wid >= p.sv.units_max) return;
      if (wid >= (uint32_t)p.sv.unit_base[p.nblocks]) return;
      u = wid;
      b = __builtin_amdgcn_readfirstlane(p.sv.unit_map[u]);
      u0 = (uint32_t)p.sv.unit_base[b];
      nunits = (uint32_t)p.sv.unit_base[b + 1] - u0;
      ju = u - u0;
      if (nunits == 1) return;  // (decoded by the fused kernel)
      if (p.sv.pass != 0 && p.sv.ustate[kUsWords * u + kUsRerun] == kSegNone) return;
    } else {
      if (b >= p.nblocks) return;  // no barrier below this point
    }
    const bool multi = SEG && nunits > 1;

    // ---- per-stream setup (wave-uniform) ----
    // SEG: the wave works in its unit's frame (ricepp_internal.h): bit 0 is
    // the unit's first bit S_abs = ju 2^L of the stream, the stream is read
    // from byte S_abs / 8 on (a multiple of 128: alignment kept), and the
    // positions it stores are relative to the unit they belong to
    const uint32_t L = p.sv.seg_log2;
    int32_t status = RPP_OK;
    uint32_t N = 0, nbytes = 0, mis = 0, lim = 0;
    uint64_t Eend64 = 0;
    const uint8_t* in = p.in;
    {
      const uint64_t n64 = p.n_samples[b];
      const uint64_t ioff = p.in_off[b];
      const uint64_t nb64 = p.in_bytes[b];
      if (!rpp_internal::seg_stream_fits(n64, nb64, CS)) {
        status = RPP_INVALID_ARGUMENT;
      } else {
        N = (uint32_t)n64;
        mis = (uint32_t)(ioff & 3u);
        in = p.in + (ioff - mis);
        // last readable bit + 1 (seg_read_limit), bytes from the aligned base
        const uint64_t lim64 = seg_read_limit(mis, nb64), nbytes64 = nb64 + mis;
        const uint64_t sabs = multi ? (uint64_t)ju << L : 0u;
        in += sabs >> 3;
        nbytes = nbytes64 > (sabs >> 3) ? (uint32_t)min<uint64_t>(nbytes64 - (sabs >> 3), kSegWinBytes) : 0u;
        lim = lim64 > sabs ? (uint32_t)min<uint64_t>(lim64 - sabs, kSegWinBits) : 0u;
        if (multi) Eend64 = seg_last_bit(mis, nb64, N, bs, CS) - sabs;
      }
    }
    uint32_t* const pos_out = multi ? nullptr : p.sb_pos + p.sb_base[b];
    const bool aligned16 = ((uintptr_t)in & 15u) == 0;
    const uint32_t chunk_len = CS * bs;
    const uint32_t nchunks = status == RPP_OK ? (N + chunk_len - 1) / chunk_len : 0u;

    // ---- SEG: the unit's region [S, E) of header positions (frame: S = 0) ----
    const bool serial = multi && p.sv.pass == 2;
    uint32_t S = 0, E = 0;
    bool last = false;
    if (multi) {
      last = ju + 1 == nunits;
      E = last ? (uint32_t)(Eend64 + 1) : 1u << L;
      // (a serial pass parses to the stream's end: one that would leave the
      // frame stops at kSegSerialEnd, past its region, and the fused kernel
      // takes the stream)
      if (serial) E = (uint32_t)min<uint64_t>(Eend64 + 1, kSegSerialEnd);
    }

    // ---- SEG: the first header of the unit ----
    // A guess: the first candidate bit in [S + c_first, S + max sub-block) whose
    // chain of kSpecSteps sub-blocks looks like ricepp output (seg_guess).
    uint32_t grange = 3;  // the header range of the guess's chains (seg_guess), which the parse checks
    auto do_guess = [&](uint32_t c_first) -> uint32_t {
      const uint32_t kStW = stage_w;
      const uint32_t w0 = S >> 5;
      for (uint32_t i = lane; i < kStW; i += kWave) ring[i] = stream_word(in, nbytes, w0 + i);
      lds_fence();
      const uint64_t tg = memtime();
      uint32_t g = seg_guess(ring, ring + kStW, min(32u * kStW - 64u, lim - S), bs, lane, c_first, 3, tab);
      grange = 3;
      // none: the true chain's headers may span a wider range for a few
      // sub-blocks; a second search with range 5 (its candidates are checked
      // by the parse with that range)
      if (g == kSegNone && c_first == 0) {
        g = seg_guess(ring, ring + kStW, min(32u * kStW - 64u, lim - S), bs, lane, 0, 5, tab);
        grange = 5;
      }
      if (lane == 0) atomicAdd(&g_parse_diag[0], (unsigned long long)(memtime() - tg));
      lds_fence();  // (the ring is refilled next)
      return g == kSegNone ? kSegNone : S + g;
    };
    uint32_t P = 8u * mis + 16u * CS;  // codec.h:81-86: the initial values
    bool guessed = false;     // (verify the chain from P)
    uint32_t P_first = 0;     // the first guess, taken unverified if no later candidate verifies
    uint32_t* const us = p.sv.ustate + kUsWords * u;
    if (multi) {
      uint32_t flags = 0;
      if (p.sv.pass != 0) {
        P = us[kUsRerun];  // a header of the exact chain (stitch)
        flags = kUfRerunDone;
      } else if (ju != 0) {
        // (searched beforehand by several waves: rpp_seg_guess_kernel)
        const uint32_t pre = __builtin_amdgcn_readfirstlane(us[kUsGuess]);
        // (a guess of rpp_seg_guess_kernel is not checked again here: a wrong
        // one costs a rerun of the unit, in parallel with any others, where a
        // one-wave re-guess would hold up the whole pass)
        P = P_first = pre == kSegNone ? do_guess(0) : pre == kSegNoGuess ? kSegNone : pre;
        guessed = pre == kSegNone;
        if (P == kSegNone) flags = kUfNoGuess;
      }
      if (lane == 0) {
        us[kUsNovr] = 0;
        us[kUsStart] = P;
        us[kUsRerun] = kSegNone;
        us[kUsFlags] = flags;
        us[kUsNpos] = 0;
      }
      if (serial)  // (the serial pass lists the positions of every later unit)
        for (uint32_t k = ju + 1 + lane; k < nunits; k += kWave) p.sv.ustate[kUsWords * (u0 + k) + kUsNpos] = 0;
      if (serial && lane == 0) {  // the stitch bookkeeping of the rest of the stream
        p.sv.uov[u - 1] = kSegOvr - 1;
        p.sv.ulo[u] = 0;  // (list indices: every position this pass lists is exact)
        for (uint32_t k = ju + 1; k < nunits; ++k) {
          p.sv.ulo[u0 + k] = 0;
          p.sv.uov[u0 + k - 1] = 0;
        }
        p.sv.uov[u0 + nunits - 1] = 0;
        p.sv.sst[b] = nunits;
      }
      if (P == kSegNone) return;
    }

    for (uint32_t attempt = 0;; ++attempt) {
      // ---- LDS ring of the stream's words (as rpp_decode_kernel) ----
      uint32_t fill_w = multi ? (P >> 5) & ~(kChunkWords - 1) : 0u;
      bool pend = false;
      auto retire = [&]() {
        if (pend) {
          vm_drain();
          fill_w += kChunkWords;
          pend = false;
        }
      };
      auto refill_sync = [&]() {
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
      auto request = [&]() {
        if (4u * (fill_w + kChunkWords) > nbytes) return;
        const uint32_t slot = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)&ring[fill_w & kRingMask]);
        const uint8_t* src = in + 4u * fill_w;
        if (aligned16) {
          glds16(src + 16u * lane, slot);
        } else {
    #pragma unroll
          for (uint32_t q = 0; q < 4; ++q) glds4(src + 256u * q + 4u * lane, slot + 256u * q);
        }
        if ((fill_w & kRingMask) == 0)
          glds4(src + 4u * lane, __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)&ring[kRingWords]));
        pend = true;
      };
      refill_sync();
      refill_sync();
      lds_fence();
      auto ensure = [&](uint32_t w) {
        if (fill_w < w + kAhead) {
          retire();
          while (fill_w < w + kAhead) refill_sync();
          lds_fence();
        }
      };
      auto wptr = [&](uint32_t w) -> const uint32_t* { return ring + (w & kRingMask); };
      auto load_x = [&](uint32_t sb, uint32_t& xl) {
        const uint32_t* q = wptr(sb >> 5);
        xl = __builtin_amdgcn_alignbit(q[1], q[0], sb & 31u);
      };
      auto ring_keep = [&](uint32_t q) {
        if (pend && fill_w < (q >> 5) + kAhead + 128) retire();
        if (!pend && fill_w <= (q >> 5) + 766) request();
      };

      // ---- sub-block start positions, buffered 64 at a time in one VGPR,
      //      then to sb_pos (one-unit streams) or to the list of the unit
      //      whose region holds them (the serial pass crosses units) ----
      uint32_t pbuf = 0, pcnt = 0, pstart = 0;
      uint32_t novr = 0;
      bool stop = false;
      uint32_t lk = ju;  // (SEG) the unit whose list is being written
      uint32_t loff = 0;  // (SEG) its first bit in the wave's frame: list entries are relative to it
      uint64_t lbase = multi ? p.sv.pl_base[u] : 0;
      uint32_t lcap = multi ? (uint32_t)(p.sv.pl_base[u + 1] - lbase) : 0;
      auto flush = [&]() {
        if (multi) {
          if (pstart + pcnt > lcap) {  // below 1 bit per sample: the fused kernel takes the stream
            stop = true;
            if (lane == 0) atomicOr(p.sv.sflags + b, kSfListFull);
          } else if (lane < pcnt) {
            p.sv.plist[lbase + pstart + lane] = pbuf - loff;
          }
        } else {
          if (lane < pcnt) pos_out[pstart + lane] = pbuf;
        }
        pstart += pcnt;
        pcnt = 0;
      };
      auto close_list = [&]() {
        if (lane == 0) p.sv.ustate[kUsWords * (u0 + lk) + kUsNpos] = min(pstart, lcap);
      };
      auto record = [&](uint32_t pos) {
        if (multi && pos >= E) {  // past the region: the overshoot list, or the end
          if (last || serial) {
            stop = true;
            if (lane == 0) atomicOr(p.sv.sflags + b, kSfPastRegion);
          } else {
            // (relative to the next unit's first bit, E)
            if (lane == 0 && novr < kSegOvr) p.sv.ovr[kSegOvr * u + novr] = pos - E;
            if (++novr >= kSegOvr) stop = true;
          }
          return;
        }
        if (serial && (pos >> L) != lk - ju) {  // into the next unit's region
          flush();
          close_list();
          lk = ju + (pos >> L);
          loff = (pos >> L) << L;
          lbase = p.sv.pl_base[u0 + lk];
          lcap = (uint32_t)(p.sv.pl_base[u0 + lk + 1] - lbase);
          pstart = 0;
        }
        pbuf = lane == pcnt ? pos : pbuf;
        if (++pcnt == kWave) flush();
      };

      // SEG, a guessed start: the first kSpecVerify headers of the chain must
      // keep to the guess's rule (seg_guess), else the guess was wrong and the
      // next candidate is tried.  Until then no position has left pbuf
      // (kSpecVerify < 64), so a rejected chain leaves nothing behind.
      uint32_t vcnt = guessed ? 0u : kSpecVerify, vlo = 15, vhi = 0;
      bool vfail = false;
      auto note = [&](uint32_t v) {
        if (vcnt < kSpecVerify) {
          ++vcnt;
          vlo = min(vlo, v);
          vhi = max(vhi, v);
          if (vhi - vlo > grange || (vlo == 0 && vhi != 0)) vfail = stop = true;
        }
      };

      if (!multi && status == RPP_OK && P > lim) status = RPP_TRUNCATED_INPUT;
      // a unit of a split stream parses bs-sample sub-blocks until its region
      // ends (the ragged last chunk is re-parsed by rpp_seg_tail_kernel)
      const uint32_t nsb = multi ? 0xFFFFFFFFu : nchunks * CS;
      const bool fast_bs = bs == 2 * kWave || bs == 16 || bs == 32 || bs == 64;
      // (a unit runs the window loop for any bs <= 128: it only needs the
      // sub-block's end; longer sub-blocks never end in a 1536-bit window)
      const uint32_t nsb_fast = multi ? (bs <= 2 * kWave ? 0xFFFFFFFFu : 0u) : fast_bs ? (N / chunk_len) * CS : 0u;
      ScanRegs sreg;

      uint32_t s = 0;
      const uint64_t t_chain = multi ? memtime() : 0;
      const uint32_t P0 = P;
      while (s < nsb && status == RPP_OK && !stop) {
        // ---- fast loop: Rice sub-blocks of bs codes with fs in [LO, HI] lying
        //      in one window, ring resident; the parse of sub-block s+1 is issued
        //      as soon as the end of s is known ----
        auto fast = [&]<uint32_t MT, uint32_t LO, uint32_t HI>() {
          // fs 8..13: 32-bit lane segments and jacobi entry states (w32_count)
          constexpr bool W32 = LO >= 8;
          constexpr uint32_t SB = W32 ? 32u : kSegBits;
          const uint32_t n = bs;
          auto seg_bits = [&](uint32_t q) {
            if constexpr (W32) {
              const uint32_t* w = ring + (((q >> 5) + lane) & kRingMask);
              return __builtin_amdgcn_alignbit(w[1], w[0], q & 31u);
            } else {
              const uint32_t o = lane24 + (q & 31u);
              uint32_t oi = o >> 5;
              asm("" : "+v"(oi));
              const uint32_t* w = ring + ((q >> 5) & kRingMask) + oi;
              return __builtin_amdgcn_alignbit(w[1], w[0], o);
            }
          };
          auto fs_of = [](uint32_t h) {
            uint32_t r;
            asm("s_and_b32 %0, %1, 15\n\ts_max_u32 %0, %0, %2\n\ts_min_u32 %0, %0, %3\n\ts_sub_u32 %0, %0, 1"
                : "=&s"(r)
                : "s"(h), "n"(LO + 1), "n"(HI + 1)
                : "scc");
            return r;
          };
          auto header_ok = [](uint32_t h) { return (uint32_t)((h & 15u) - (LO + 1) <= HI - LO); };
          // end (next header) of the sub-block at bit q, if it lies in the window
          auto parse = [&](uint32_t q, uint32_t fs, uint4 e0, uint4 e1, uint4 e2, uint4 e3, uint32_t& Pe) -> bool {
            const uint32_t k = fs + 1;
            uint32_t tm, cnt, incl;
            uint64_t finm;
            if constexpr (W32) {
              uint32_t unused_rider;
              w32_count(e0, e1, e2, e3, n, 0u, sreg, tm, cnt, incl, finm, unused_rider);
            } else {
              const Map8 M01 = comp8(Map8{e1.x, e1.y}, Map8{e0.x, e0.y});
              Map8 M = comp8(Map8{e2.x, e2.y}, M01);
              M = scan8_shr1(M, sreg.r1);
              M = scan8_shr2(M, sreg.r2);
              M = scan8_shr4(M, sreg.r4);
              M = scan8_shr8(M, sreg.r8);
              M = scan8_bc15(M, sreg.b15);
              M = scan8_bc31(M, sreg.b31);
              const Map8 X = shift8_wave(M, sreg.w1);
              const uint32_t sel = __builtin_amdgcn_perm(X.hi, X.lo, 0xFFFFFF04u);
              const uint32_t a0 = __builtin_amdgcn_perm(e0.w, e0.z, sel);
              const uint32_t a1 = __builtin_amdgcn_perm(e1.w, e1.z, __builtin_amdgcn_perm(e0.y, e0.x, sel));
              const uint32_t a2 = __builtin_amdgcn_perm(e2.w, e2.z, __builtin_amdgcn_perm(M01.hi, M01.lo, sel));
              tm = __builtin_amdgcn_perm(a2, __builtin_amdgcn_perm(a1, a0, 0x0C0C0400u), 0x0C040100u);
              cnt = __builtin_popcount(tm);
              incl = wave_incl_sum(cnt);
              finm = __ballot(incl >= n);
            }
            const uint32_t excl = incl - cnt;
            uint32_t t[MT];
    #pragma unroll
            for (uint32_t j = 0; j < MT; ++j) {
              t[j] = ffbl(tm);
              tm &= tm - 1;
            }
            const uint32_t r = n - 1 - excl;
            uint32_t tpk = t[0] | (t[1] << 8) | ((t[2] | (t[3] << 8)) << 16);
            if constexpr (MT > 4) {
              const uint32_t tpk1 = t[4] | (t[5] << 8) | ((t[6] | (t[7] << 8)) << 16);
              tpk = r < 4 ? tpk : tpk1;
            }
            if constexpr (MT > 8) {
              const uint32_t tpk2 = t[8] | (t[9] << 8) | ((t[10] | (t[11] << 8)) << 16);
              tpk = r < 8 ? tpk : tpk2;
            }
            const uint32_t tend = __builtin_amdgcn_ubfe(tpk, 8 * (r & 3u), 8);
            const uint32_t lz = (uint32_t)__builtin_ctzll(finm | (1ull << 63));
            Pe = q + SB * lz + readlane(tend, (int)lz) + k;
            return finm != 0;
          };
          auto lookups = [&](uint32_t xl, uint32_t fs, uint4& e0, uint4& e1, uint4& e2, uint4& e3) {
            const uint4* tb = tab + 256u * fs;
            e0 = tb[xl & 0xFFu];
            e1 = tb[__builtin_amdgcn_ubfe(xl, 8, 8)];
            e2 = tb[__builtin_amdgcn_ubfe(xl, 16, 8)];
            if constexpr (W32) e3 = tb[xl >> 24];
            else e3 = make_uint4(0u, 0u, 0u, 0u);
          };
          uint32_t pn_limit, trig_w;
          auto ring_bounds = [&]() {
            pn_limit = min(lim - 4u, 32u * (fill_w - kAhead) + 31u);
            trig_w = pend ? fill_w - (kAhead + 127u) : (fill_w > 766u ? fill_w - 766u : 0u);
          };
          ring_bounds();
          uint32_t Pn;
          const uint32_t xl = seg_bits(P);
          const uint32_t h = __builtin_amdgcn_readfirstlane(xl);
          uint32_t fs = fs_of(h);
          uint4 e0, e1, e2, e3;
          lookups(xl, fs, e0, e1, e2, e3);
          bool ok = parse(P, fs, e0, e1, e2, e3, Pn) && header_ok(h);
          uint32_t hc = h;  // header of the sub-block at P
          while (ok) {
            // sub-block s at P ends at Pn; parse s+1 at Pn
            const bool nxt = s + 1 < nsb_fast && Pn <= pn_limit && !stop;
            const uint32_t xlB = seg_bits(Pn);
            const uint32_t hB = __builtin_amdgcn_readfirstlane(xlB);
            const uint32_t fsB = fs_of(hB);
            lookups(xlB, fsB, e0, e1, e2, e3);
            uint32_t PnB;
            ok = parse(Pn, fsB, e0, e1, e2, e3, PnB) && header_ok(hB) && nxt;
            record(P);
            if (multi) note(hc & 15u);
            hc = hB;
            ++s;
            P = Pn;
            if (!ok) {
              if (P > lim) status = RPP_TRUNCATED_INPUT;
              break;
            }
            Pn = PnB;
            fs = fsB;
            if ((Pn >> 5) >= trig_w) {
              ring_keep(Pn);
              ring_bounds();
            }
          }
        };
        while (s < nsb_fast && status == RPP_OK && !stop && fill_w >= (P >> 5) + kAhead && P + 4 <= lim) {
          const uint32_t* w = ring + ((P >> 5) & kRingMask);
          const uint32_t h = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(w[1], w[0], P & 31u)) & 15u;
          const uint32_t s0 = s;
          if (h - 6u <= 2u) fast.template operator()<4, 5, 7>();
          else if (h - 3u <= 2u) fast.template operator()<8, 2, 4>();
          else if (h - 9u <= 5u) fast.template operator()<4, 8, 13>();
          else if (h == 2u) fast.template operator()<12, 1, 4>();
          if (s == s0) break;  // the general path takes this sub-block
        }
        if (s >= nsb || status != RPP_OK || stop) break;
        // ---- general path: one sub-block of any kind ----
        const uint32_t cbase = (s / CS) * chunk_len;
        const uint32_t n = multi ? bs : min(N - cbase, chunk_len) / CS;
        ensure(P >> 5);
        if (multi) {  // (the end of the stream's last sub-block is a position too)
          record(P);
          if (stop) break;
        }
        if (P + 4 > lim) {  // decode.h:60: the 4-bit header
          status = RPP_TRUNCATED_INPUT;
          break;
        }
        if (!multi) record(P);
        uint32_t xl;
        load_x(P + kSegBits * lane, xl);
        const uint32_t fsp1 = __builtin_amdgcn_readfirstlane(xl) & 15u;
        if (multi) {
          note(fsp1);
          if (vfail) break;
        }
        if (fsp1 == 0) {  // decode.h:79-80
          P += 4;
        } else if (fsp1 == 15) {  // decode.h:72-77: n raw 16-bit values
          if ((uint64_t)P + 4 + 16ull * n > lim) {
            status = RPP_TRUNCATED_INPUT;
            break;
          }
          P += 4 + 16 * n;
        } else {  // decode.h:62-71: n Rice codes; find the end of code n-1
          const uint32_t fs = fsp1 - 1;
          const uint4* tb = tab + 256u * fs;
          uint32_t q0 = P, s0 = 4, done = 0;
          for (;;) {
            const uint4 e0 = tb[xl & 0xFFu], e1 = tb[__builtin_amdgcn_ubfe(xl, 8, 8)],
                        e2 = tb[__builtin_amdgcn_ubfe(xl, 16, 8)];
            uint32_t tm, xexit;
            if (fs < 8) {
              Map8 M = comp8(Map8{e2.x, e2.y}, comp8(Map8{e1.x, e1.y}, Map8{e0.x, e0.y}));
              M = scan_step8<kDppRowShr1>(M);
              M = scan_step8<kDppRowShr2>(M);
              M = scan_step8<kDppRowShr4>(M);
              M = scan_step8<kDppRowShr8>(M);
              M = scan_step8<kDppRowBcast15, 0xA>(M);
              M = scan_step8<kDppRowBcast31, 0xC>(M);
              const Map8 X{dpp_keep<kDppWaveShr1>(kId0, M.lo), dpp_keep<kDppWaveShr1>(kId1, M.hi)};
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
            const uint32_t cnt = __builtin_popcount(tm);
            const uint32_t incl = wave_incl_sum(cnt);
            const uint32_t need = n - done;
            const uint64_t fin = __ballot(incl >= need);
            if (fin) {
              // terminator need-1-excl of the first lane reaching need
              const uint32_t lz = (uint32_t)__builtin_ctzll(fin);
              uint32_t tmv = readlane(tm, (int)lz);
              const uint32_t r = need - 1 - (readlane(incl, (int)lz) - readlane(cnt, (int)lz));
              for (uint32_t j = 0; j < r; ++j) tmv &= tmv - 1;
              P = q0 + kSegBits * lz + (uint32_t)__builtin_ctz(tmv) + fsp1;
              break;
            }
            done += wave_last(incl);
            s0 = wave_last(xexit);
            q0 += kWinBits;
            if (q0 >= lim) {  // the open unary search would read past the input
              status = RPP_TRUNCATED_INPUT;
              break;
            }
            ensure(q0 >> 5);
            load_x(q0 + kSegBits * lane, xl);
          }
          if (status != RPP_OK) break;
          if (P > lim) {
            status = RPP_TRUNCATED_INPUT;
            break;
          }
        }
        ++s;
        ring_keep(P);
      }
      retire();
      if (vfail) {  // the guess failed its check: the next candidate that chains
        P = attempt < kGuessRetries ? do_guess(P0 - S + 1) : kSegNone;
        if (P == kSegNone) {  // none: the first guess after all (its chain may just vary more)
          P = P_first;
          guessed = false;
        }
        continue;
      }
      if (multi) {
        flush();
        close_list();
        vm_drain();
        if (lane == 0) {
          atomicAdd(&g_parse_diag[1], (unsigned long long)(memtime() - t_chain));
          atomicAdd(&g_parse_diag[2], (unsigned long long)s);
          atomicAdd(&g_parse_diag[3], 1ull);
          if (attempt) atomicAdd(&g_parse_diag[7], (unsigned long long)attempt);
          us[kUsStart] = P0;
          us[kUsNovr] = min(novr, kSegOvr);
          if (status != RPP_OK) us[kUsFlags] |= kUfTrunc;
        }
        return;
      }
      if (status == RPP_OK) record(P);  // the end of the last sub-block
      flush();
      if (lane == 0) p.status[b] = status;
      return;
    }
  };
  const bool queue = SEG && p.sv.pass == 0;
  const uint32_t items = queue ? (uint32_t)p.sv.unit_base[p.nblocks] : 0u;
  for (;;) {
    uint32_t wid = blockIdx.x * p.waves + wv;
    if (queue) {
      uint32_t w = 0;
      if (lane == 0) w = atomicAdd(p.sv.queue, 1u);
      wid = __builtin_amdgcn_readfirstlane(w);
      if (wid >= items) break;
    }
    work(wid);
    if (!queue) break;
  }
}

}  // namespace

// The first guess of every unit j >= 1 of a split stream, searched by
// kGuessWaves waves at once (one workgroup per unit): wave w takes the
// 128-candidate chunks w, w + kGuessWaves, ... of seg_guess's search and
// stops at chunks beyond the lowest survivor any wave has found (LDS); the
// unit's guess is that lowest survivor, the candidate the one-wave search
// returns.  For batches of few units (single long streams), where
// the parse's work queue would run one wave per CU and the lane-serial guess
// is most of a unit's time.
// (16 waves, one workgroup per CU: 8 waves took 1.5-5 % longer on single
// 16 MiB streams, 16 x 1 MiB and 32 MiB frames; 4 waves x 4 slots and
// 16 x 4 slower still -- tools/one_stream_prof.py, profiles/r05_guess_waves_ab.txt)
constexpr uint32_t kGuessWaves = 16;
constexpr uint32_t kGuessSlots = 2;  // candidates per lane of a chunk (128-candidate chunks)
constexpr uint32_t kGuessListWords = 2 * kGuessSlots * kWave;  // a wave's survivors: (position, origin | range)
__host__ __device__ constexpr size_t guess_lds_bytes(uint32_t bs) {
  // (the staged words of parse_wave_words, once per workgroup: 76 KiB at bs <= 128, two workgroups per CU)
  return kTabBytes + 4 * ((size_t)parse_wave_words(bs) - (kListLead + kListWords) + kGuessWaves * kGuessListWords);
}
template <uint32_t CS>
__global__ __launch_bounds__(kWave* kGuessWaves) void rpp_seg_guess_kernel(ParseParams p) {
  using namespace rpp_internal;
  extern __shared__ __attribute__((aligned(16))) uint4 dsm[];
  __shared__ uint32_t best;
  const uint32_t u = blockIdx.x;
  if (u >= p.sv.units_max || u >= (uint32_t)p.sv.unit_base[p.nblocks]) return;  // (uniform: one unit per workgroup)
  const uint32_t b = p.sv.unit_map[u];
  const uint32_t u0 = (uint32_t)p.sv.unit_base[b], nunits = (uint32_t)p.sv.unit_base[b + 1] - u0;
  const uint32_t ju = u - u0;
  if (nunits <= 1 || ju == 0) return;
  const uint64_t n64 = p.n_samples[b], ioff = p.in_off[b], nb64 = p.in_bytes[b];
  if (!rpp_internal::seg_stream_fits(n64, nb64, CS)) return;
  {
    copy_tables(dsm);
  }
  if (threadIdx.x == 0) best = kSegNone;
  __syncthreads();
  const uint4* tab = dsm;
  const uint32_t lane = lane_id();
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  // the unit's staged words, shared by the waves, then a survivor list per wave
  const uint32_t stage_w = p.wave_words - (kListLead + kListWords);
  uint32_t* ring = reinterpret_cast<uint32_t*>(dsm) + kTabBytes / 4;
  uint32_t* list = ring + stage_w + wv * kGuessListWords;
  // the unit's frame (as in rpp_parse_kernel): bit 0 at its first bit
  const uint32_t mis = (uint32_t)(ioff & 3u);
  const uint64_t sabs = (uint64_t)ju << p.sv.seg_log2;
  const uint64_t lim64 = seg_read_limit(mis, nb64), nbytes64 = nb64 + mis;
  const uint32_t nbytes =
      nbytes64 > (sabs >> 3) ? (uint32_t)min<uint64_t>(nbytes64 - (sabs >> 3), kSegWinBytes) : 0u;
  const uint8_t* in = p.in + (ioff - mis) + (sabs >> 3);
  const uint32_t lim = lim64 > sabs ? (uint32_t)min<uint64_t>(lim64 - sabs, kSegWinBits) : 0u;
  const uint32_t S = 0;
  const uint32_t w0 = 0;
  for (uint32_t i = threadIdx.x; i < stage_w; i += blockDim.x) ring[i] = stream_word(in, nbytes, w0 + i);
  __syncthreads();
  const uint32_t end_rel = S < lim ? min(32u * stage_w - 64u, lim - S) : 0u;
  const uint64_t tg = memtime();
  // chains of kSpecVerify sub-blocks, the check the one-wave parse makes of a
  // guess: the lowest survivor is the candidate that parse would settle on
  // after rejecting the ones before it (the parse trusts this guess); range 5
  // when none keeps range 3; failing both, the kSpecSteps survivor the parse
  // would take unchecked in the end
  uint32_t g = kSegNone;
  for (uint32_t k = 0; k < 4 && g == kSegNone; ++k) {
    if (k != 0) {
      if (threadIdx.x == 0) best = kSegNone;
      __syncthreads();
    }
    (void)seg_guess<kGuessSlots>(ring, list, end_rel, p.bs, lane, 0, k & 1 ? 5u : 3u, tab, wv, kGuessWaves, &best,
                    k < 2 ? kSpecVerify : kSpecSteps);
    __syncthreads();
    g = best;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    p.sv.ustate[kUsWords * u + kUsGuess] = g == kSegNone ? kSegNoGuess : S + g;
    atomicAdd(&g_parse_diag[0], (unsigned long long)(memtime() - tg));
  }
}

extern "C" {

// diagnostics only (not in the C ABI header): the segmented parse's counters
int rpp_parse_diag_read(unsigned long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_parse_diag), sizeof(g_parse_diag)) != hipSuccess) return RPP_HIP_ERROR;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_parse_diag), z, sizeof(z)) != hipSuccess) return RPP_HIP_ERROR;
  }
  return RPP_OK;
}

}  // extern "C"

namespace rpp_internal {

// (below this many units the parse's work queue leaves wave slots idle: each
// unit's guess gets kGuessWaves waves of its own)
// (a bound on the batch's worst-case unit count.  Raised to 16384 / 65536 in
// round 6, the guess kernel made the 7.7 Gbit generator stream slower, 10.1 ->
// 10.7 ms, with 1 rerun instead of 8, and the configs[3] mix 9 % slower:
// profiles/r06_guess_bound_ab.jsonl)
constexpr uint32_t kGuessKernelMaxUnits = 2048;
int launch_seg_guess(const rpp_config* cfg, const uint8_t* d_in, const uint64_t* d_in_offsets,
                     const uint64_t* d_in_bytes, uint32_t nblocks, const uint64_t* d_n_samples, const SegView& sv,
                     hipStream_t stream) {
  if (nblocks == 0 || sv.units_max == 0 || sv.units_max > kGuessKernelMaxUnits) return RPP_OK;
  const uint32_t wave_words = parse_wave_words(cfg->block_size);
  const size_t lds = guess_lds_bytes(cfg->block_size);
  static void (*const kernels[2])(ParseParams) = {rpp_seg_guess_kernel<1>, rpp_seg_guess_kernel<2>};
  static const hipError_t attr_err = set_max_dynamic_lds(kernels, guess_lds_bytes(kLongSbBs));
  if (attr_err != hipSuccess) return RPP_HIP_ERROR;
  ParseParams p{d_in, d_in_offsets, d_in_bytes, d_n_samples, nullptr, nullptr, nullptr, nblocks,
                cfg->block_size, kGuessWaves, sv, wave_words};
  hipLaunchKernelGGL(kernels[cfg->component_stream_count - 1], dim3(sv.units_max), dim3(kWave * kGuessWaves), lds,
                     stream, p);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}

// CUs of the current device, queried once per device (callers on any thread:
// the facade's driver threads run segmented decodes concurrently)
int device_cu_count() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  cache[dev].store(n, std::memory_order_relaxed);
  return n;
}

int launch_parse_seg(const rpp_config* cfg, const uint8_t* d_in, const uint64_t* d_in_offsets,
                     const uint64_t* d_in_bytes, uint32_t nblocks, const uint64_t* d_n_samples,
                     const uint64_t* d_sb_base, uint32_t* d_sb_pos, int32_t* d_status, const SegView& sv,
                     hipStream_t stream) {
  if (nblocks == 0 || sv.units_max == 0) return RPP_OK;
  // pass 0: a work queue, one workgroup per CU; rerun passes have a few units
  // to do: one wave per workgroup, one unit each
  const int cus = device_cu_count();
  // (pass 0: as many waves per workgroup as the unit bound needs to give every
  // CU some, at most 16, so that a batch of few units still spreads over all CUs)
  const uint32_t wave_words = parse_wave_words(cfg->block_size);
  const uint32_t wmax = kDecMaxWaves * kWaveLdsWords / wave_words;
  const uint32_t W = sv.pass == 0 ? std::min<uint32_t>(wmax, std::max<uint32_t>(1, (sv.units_max + cus - 1) / cus))
                                  : 1u;
  const uint32_t grid = sv.pass == 0 ? std::min<uint32_t>((uint32_t)cus, (sv.units_max + W - 1) / W) : sv.units_max;
  const size_t lds = kTabBytes + (size_t)W * wave_words * 4;
  static void (*const kernels[2])(ParseParams) = {rpp_parse_kernel<1, true>, rpp_parse_kernel<2, true>};
  static const hipError_t attr_err =
      set_max_dynamic_lds(kernels, kTabBytes + (size_t)kDecMaxWaves * kWaveLdsWords * 4);
  if (attr_err != hipSuccess) return RPP_HIP_ERROR;
  ParseParams p{d_in, d_in_offsets, d_in_bytes, d_n_samples, d_sb_base, d_sb_pos, d_status, nblocks,
                cfg->block_size, W, sv, wave_words};
  hipLaunchKernelGGL(kernels[cfg->component_stream_count - 1], dim3(grid), dim3(kWave * W), lds, stream, p);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}

}  // namespace rpp_internal
