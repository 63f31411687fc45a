// ricepp_wave.h -- device primitives shared by the ricepp kernel translation
// units: pixel traits, lane / DPP moves and wave scans, LDS and vector-memory
// fences, asynchronous global -> LDS copies, single-instruction helpers and
// the zero-padded stream read.  Everything is inlined; internal linkage, so
// each translation unit has its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kWave = 64;

// ---------------------------------------------------------------------------
// pixel traits (ricepp/ricepp_cpuspecific_traits.h:63-75)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v >> 8) | (v << 8)) & 0xFFFFu; }
__device__ __forceinline__ uint32_t px_read(uint32_t v, uint32_t be, uint32_t ulsb) {
  v &= 0xFFFFu;
  if (be) v = bswap16(v);
  return v >> ulsb;
}
__device__ __forceinline__ uint32_t px_write(uint32_t v, uint32_t be, uint32_t ulsb) {
  v = (v << ulsb) & 0xFFFFu;
  return be ? bswap16(v) : v;
}

// ---------------------------------------------------------------------------
// wave helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// DPP controls (gfx9 encoding)
constexpr int kDppQuadXor1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;     // quad_perm [2,3,0,1]
constexpr int kDppRowShr1 = 0x111;
constexpr int kDppRowShr2 = 0x112;
constexpr int kDppRowShr4 = 0x114;
constexpr int kDppRowShr8 = 0x118;
constexpr int kDppWaveShr1 = 0x138;
constexpr int kDppRowMirror = 0x140;
constexpr int kDppRowHalfMirror = 0x141;
constexpr int kDppRowBcast15 = 0x142;
constexpr int kDppRowBcast31 = 0x143;

template <int Ctrl, int RowMask = 0xF>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  // lanes whose source is outside the row / not selected read 0
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, Ctrl, RowMask, 0xF, false);
}

// Inclusive prefix sum over the 64 lanes (all active).
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
  v += dpp<kDppRowShr1>(v);
  v += dpp<kDppRowShr2>(v);
  v += dpp<kDppRowShr4>(v);
  v += dpp<kDppRowShr8>(v);
  v += dpp<kDppRowBcast15, 0xA>(v);
  v += dpp<kDppRowBcast31, 0xC>(v);
  return v;
}

// Inclusive prefix max over the 64 lanes (all active, values >= 0).
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
  v = max(v, dpp<kDppRowShr1>(v));
  v = max(v, dpp<kDppRowShr2>(v));
  v = max(v, dpp<kDppRowShr4>(v));
  v = max(v, dpp<kDppRowShr8>(v));
  v = max(v, dpp<kDppRowBcast15, 0xA>(v));
  v = max(v, dpp<kDppRowBcast31, 0xC>(v));
  return v;
}

// Orders this wave's LDS accesses (one wave's DS operations execute in
// order); unlike __syncthreads() it does not drain vmcnt, so outstanding
// global loads (prefetches) and stores stay in flight.  One-wave workgroups.
__device__ __forceinline__ void wave_lds_fence() { asm volatile("" ::: "memory"); }

// DPP move; lanes without a source in range keep `old`.  Called with every
// lane active (a DPP source lane that is switched off reads as out of range).
template <int Ctrl, int RowMask = 0xF>
__device__ __forceinline__ uint32_t dpp_keep(uint32_t old, uint32_t v) {
  // lanes without a source in range keep `old`
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, Ctrl, RowMask, 0xF, false);
}

// Value of lane l-1 (0 for lane 0).
__device__ __forceinline__ uint32_t from_left(uint32_t v) { return dpp<kDppWaveShr1>(v); }

__device__ __forceinline__ uint32_t readlane(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(uint32_t v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ uint32_t as_u32(us2 v) { return __builtin_bit_cast(uint32_t, v); }

// pixel write (ricepp_cpuspecific_traits.h:69-73) of two packed samples (low,
// high); sel = v_perm selector that byte-swaps each half (big endian) or not;
// SH: unused_lsb_count != 0 (the write shifts)
template <bool SH>
__device__ __forceinline__ uint32_t px_write2(uint32_t v, uint32_t sel, uint32_t ulsb) {
  if (SH) v = as_u32(as_us2(v) << (us2)(unsigned short)ulsb);
  return __builtin_amdgcn_perm(v, v, sel);
}

// Orders this wave's LDS accesses without waiting on its global stores
// (LDS operations of one wave complete in order; a full __syncthreads()
// would also drain vmcnt, i.e. wait for the previous chunk's output stores).
__device__ __forceinline__ void lds_fence() { asm volatile("" ::: "memory"); }

// Asynchronous global -> LDS copies (global_load_lds): lane l's 16 (4) bytes
// land at LDS byte address m0 + 16 l (4 l).  Issued by asm, so the compiler
// neither waits for them nor counts them: the caller retires them with
// vm_drain() before the words are read.
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t m0) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(m0) : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, uint32_t m0) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(m0) : "memory");
}
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Waits for all but the last `after` vector-memory instructions (vmcnt
// decrements in issue order on gfx9), bucketed to a few immediates; a lower
// count only waits longer.
__device__ __forceinline__ void vm_wait_all_but(uint32_t after) {
  if (after >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (after >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (after >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// (a << s) | b in one v_lshl_or_b32 (s uniform)
__device__ __forceinline__ uint32_t lshl_or(uint32_t a, uint32_t sh, uint32_t b) {
  uint32_t r;
  asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(sh), "v"(b));
  return r;
}
// -(x & 1) in one v_bfe_i32
__device__ __forceinline__ uint32_t neg_lsb(uint32_t x) {
  uint32_t r;
  asm("v_bfe_i32 %0, %1, 0, 1" : "=v"(r) : "v"(x));
  return r;
}

// 16 * byte B of x in one VOP2 operation (SDWA source select)
template <int B>
__device__ __forceinline__ uint32_t sdwa_byte16(uint32_t x) {
  uint32_t r;
  if constexpr (B == 0)
    asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(x));
  else if constexpr (B == 1)
    asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(x));
  else if constexpr (B == 2)
    asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(x));
  else
    asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(x));
  return r;
}

// v_ffbl_b32: index of the lowest set bit, 0xFFFFFFFF for 0
__device__ __forceinline__ uint32_t ffbl(uint32_t x) {
  uint32_t r;
  asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// 32-bit word `w` of the stream, zero past the end (bitstream_reader.h:165-166
// zero-pads the last packet; reading beyond it is checked separately).
__device__ __forceinline__ uint32_t stream_word(const uint8_t* in, uint32_t nbytes, uint32_t w) {
  const uint32_t byte0 = w * 4u;
  if (byte0 >= nbytes) return 0u;
  if (nbytes - byte0 >= 4) return *reinterpret_cast<const uint32_t*>(in + byte0);
  uint32_t v = 0;
  for (uint32_t k = 0; k < nbytes - byte0; ++k) v |= (uint32_t)in[byte0 + k] << (8 * k);
  return v;
}

}  // namespace
