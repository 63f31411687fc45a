// similarity_kernels.hip -- the inode scan's similarity hashes on MI355X: nilsimsa (a 256-bit
// locality-sensitive digest) and the 32-bit 4-byte-histogram digest (the rpp_similarity_* group of
// include/ricepp_amd.h; inode_::scan_full / scan_fragments / scan_range,
// src/writer/internal/inode_manager.cpp:399-537).
//
// Both hashes are histograms: 256 counters, incremented at bucket indices computed from the 5 (nilsimsa) or
// 4 (similarity) bytes that end at each position.  Counts add in any order, so a message is cut into chunks of
// kChunkBytes that run on different workgroups and are summed into the message's state with integer atomics;
// the state does not depend on scheduling.
//
//   update    a fixed grid of kGridBlocks workgroups.  Every workgroup walks the batch in tiles of 256 files:
//             a block scan of the tile's chunk counts (sizes are read on the device, nothing comes from the
//             host), then chunk k of the batch belongs to workgroup k % kGridBlocks.  A chunk is processed by
//             the whole workgroup, 16 positions per thread and step: one unaligned 16-byte load plus the 4 bytes
//             before it (the chunk's left context comes from the data itself; only position 0 of the call takes
//             it from the state's window).  Nilsimsa reads one 16-byte row of an LDS table per byte value (the
//             eight T[(v + n) & 255] and the eight T[v ^ T[n]]) and issues eight no-return LDS adds per
//             position into the wave's private uint32 histogram; similarity does two multiplies and one add.
//             After the chunk the four histograms are summed and the nonzero bins added to the state with
//             global atomics (uint64 / uint32).
//   tail      one thread per message, after the update kernel in stream order: shifts the message's last bytes
//             into the window and adds its size.  The update kernel only reads these two fields and this
//             kernel is their only writer, so there is no race between a message's first chunk and its end.
//   finalize  one wave per message; the state is left unchanged.
//
// Nothing outside [offset, offset + size) of a message is read.  Every 64-bit shift has a constant amount.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ricepp_amd.h"

namespace {

constexpr uint32_t kChunkBytes = 32768;  // rpp_similarity_chunk_bytes()
constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kRun = 16;            // positions per thread and step
constexpr uint32_t kGridBlocks = 1024;   // 256 CUs x 4 workgroups
constexpr uint32_t kFinalWaves = 4;      // messages per workgroup of the finalize kernel
static_assert(8ull * kChunkBytes < (1ull << 32), "a workgroup's uint32 counters cannot overflow within one chunk");
static_assert(kChunkBytes % (kThreads * kRun) == 0 && (kGridBlocks & (kGridBlocks - 1)) == 0);

// ---- state (documented in include/ricepp_amd.h); all zero = the initial state ----

struct NilState {
  uint64_t acc[256];
  uint64_t size;
  uint8_t window[4];  // the last four bytes in message order (window[3] the latest), zero before the start
  uint8_t pad[4];
};
struct SimState {
  uint32_t acc[256];
  uint32_t val;  // the last four bytes, the latest in the low byte
  uint32_t pad;
  uint64_t size;
};
static_assert(sizeof(NilState) == 2064 && sizeof(SimState) == 1040);

// ---- the transition table: the published Nilsimsa recurrence ----

struct Tran {
  uint8_t t[256];
};
constexpr Tran make_tran() {
  Tran r{};
  uint32_t j = 0;
  for (int i = 0; i < 256; ++i) {
    j = (53 * j + 1) & 255;
    j += j;
    if (j > 255) j -= 255;
    for (int k = 0; k < i;) {  // bump past values already taken, searching again from the start
      if (r.t[k] == j) {
        j = (j + 1) & 255;
        k = 0;
      } else {
        ++k;
      }
    }
    r.t[i] = (uint8_t)j;
  }
  return r;
}
constexpr Tran kTran = make_tran();
static_assert(kTran.t[0] == 0x02 && kTran.t[1] == 0xD6 && kTran.t[2] == 0x9E && kTran.t[3] == 0x6F &&
              kTran.t[254] == 0x72 && kTran.t[255] == 0x4E);

// row v: bytes 0..7 = T[(v + n) & 255], bytes 8..15 = T[v ^ T[n]], n = 0..7
struct Rows {
  uint32_t w[256][4];
};
constexpr Rows make_rows() {
  Rows r{};
  for (uint32_t v = 0; v < 256; ++v)
    for (uint32_t n = 0; n < 8; ++n) {
      r.w[v][n >> 2] |= (uint32_t)kTran.t[(v + n) & 255] << (8 * (n & 3));
      r.w[v][2 + (n >> 2)] |= (uint32_t)kTran.t[v ^ kTran.t[n]] << (8 * (n & 3));
    }
  return r;
}
__device__ const Rows d_rows = make_rows();

constexpr uint32_t tran3(const Tran& t, uint32_t a, uint32_t b, uint32_t c, uint32_t n) {
  return ((t.t[(a + n) & 255] ^ (t.t[b] * (2 * n + 1))) + t.t[c ^ t.t[n]]) & 255;
}

__host__ __device__ constexpr uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x21f0aaadu;
  x ^= x >> 15;
  x *= 0x735a2d97u;
  x ^= x >> 15;
  return x;
}
__host__ __device__ constexpr uint32_t sim_bucket(uint32_t val) { return mix32(val + 0x9e3779b9u) >> 24; }

// ---- device ----

struct SimJob {
  const uint8_t* data;
  const uint64_t* offs;
  const uint64_t* sizes;
  const uint8_t* select;
  uint8_t* states;
  uint32_t n;
};

template <int Kind>
constexpr uint32_t state_bytes() {
  return Kind == RPP_SIMILARITY_NILSIMSA ? sizeof(NilState) : sizeof(SimState);
}

__device__ __forceinline__ void bump(uint32_t* hist, uint32_t bin) {
  (void)__hip_atomic_fetch_add(hist + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, uint32_t i) { return (w >> (8 * i)) & 255; }

// the increments of one position whose global position is at least 4; r0..r4 = the rows of w0..w4
__device__ __forceinline__ void nil_full(const uint4& r0, const uint4& r1, const uint4& r2, const uint4& r3,
                                         const uint4& r4, uint32_t* hist) {
  const uint32_t t1 = byte_of(r1.x, 0), t2 = byte_of(r2.x, 0), t3 = byte_of(r3.x, 0);
  bump(hist, ((byte_of(r0.x, 0) ^ t1) + byte_of(r2.z, 0)) & 255);
  bump(hist, ((byte_of(r0.x, 1) ^ (t1 * 3)) + byte_of(r3.z, 1)) & 255);
  bump(hist, ((byte_of(r0.x, 2) ^ (t2 * 5)) + byte_of(r3.z, 2)) & 255);
  bump(hist, ((byte_of(r0.x, 3) ^ (t1 * 7)) + byte_of(r4.z, 3)) & 255);
  bump(hist, ((byte_of(r0.y, 0) ^ (t2 * 9)) + byte_of(r4.w, 0)) & 255);
  bump(hist, ((byte_of(r0.y, 1) ^ (t3 * 11)) + byte_of(r4.w, 1)) & 255);
  bump(hist, ((byte_of(r4.y, 2) ^ (t1 * 13)) + byte_of(r0.w, 2)) & 255);
  bump(hist, ((byte_of(r4.y, 3) ^ (t3 * 15)) + byte_of(r0.w, 3)) & 255);
}

// tran3 over the LDS rows (T[v] is byte 0 of row v)
template <uint32_t N>
__device__ __forceinline__ uint32_t tran3_lds(const uint4* rows, uint32_t a, uint32_t b, uint32_t c) {
  constexpr uint32_t tn = kTran.t[N];
  const uint32_t ta = rows[(a + N) & 255].x & 255, tb = rows[b].x & 255, tc = rows[c ^ tn].x & 255;
  return ((ta ^ (tb * (2 * N + 1))) + tc) & 255;
}

// one position at global position gp, any gp (the slow path: the first bytes of a message and ragged ends);
// win = the four bytes before it, the latest in the top byte
template <int Kind>
__device__ __forceinline__ void step_any(uint32_t w0, uint32_t win, uint64_t gp, uint32_t* hist, const uint4* rows) {
  if constexpr (Kind == RPP_SIMILARITY_NILSIMSA) {
    const uint32_t w1 = win >> 24, w2 = (win >> 16) & 255, w3 = (win >> 8) & 255, w4 = win & 255;
    if (gp >= 2) bump(hist, tran3_lds<0>(rows, w0, w1, w2));
    if (gp >= 3) {
      bump(hist, tran3_lds<1>(rows, w0, w1, w3));
      bump(hist, tran3_lds<2>(rows, w0, w2, w3));
    }
    if (gp >= 4) {
      bump(hist, tran3_lds<3>(rows, w0, w1, w4));
      bump(hist, tran3_lds<4>(rows, w0, w2, w4));
      bump(hist, tran3_lds<5>(rows, w0, w3, w4));
      bump(hist, tran3_lds<6>(rows, w4, w1, w0));
      bump(hist, tran3_lds<7>(rows, w4, w3, w0));
    }
  } else {
    // val = the three bytes before and w0, big endian
    if (gp >= 3) bump(hist, sim_bucket((__builtin_bswap32(win) << 8) | w0));
  }
}

__device__ __forceinline__ uint32_t ld32u(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

template <int Kind>
__device__ __forceinline__ uint64_t state_size(const uint8_t* st) {
  if constexpr (Kind == RPP_SIMILARITY_NILSIMSA) return reinterpret_cast<const NilState*>(st)->size;
  else return reinterpret_cast<const SimState*>(st)->size;
}
// the state's last four bytes, the latest in the top byte
template <int Kind>
__device__ __forceinline__ uint32_t state_window(const uint8_t* st) {
  if constexpr (Kind == RPP_SIMILARITY_NILSIMSA) return ld32u(reinterpret_cast<const NilState*>(st)->window);
  else return __builtin_bswap32(reinterpret_cast<const SimState*>(st)->val);
}

// chunk c of message b, by the whole workgroup; hist = the workgroup's kWaves histograms (all zero on entry
// and on return)
template <int Kind>
__device__ void process_chunk(const SimJob& j, uint32_t b, uint64_t c, uint32_t* hist_all, const uint4* rows) {
  const uint8_t* p = j.data + j.offs[b];
  const uint64_t size = j.sizes[b];
  uint8_t* st = j.states + (size_t)b * state_bytes<Kind>();
  const uint64_t g0 = state_size<Kind>(st);
  const uint64_t lo = c * kChunkBytes;
  const uint64_t hi = size - lo < kChunkBytes ? size : lo + kChunkBytes;
  uint32_t* hist = hist_all + 256 * (threadIdx.x >> 6);
  for (uint64_t q = lo + kRun * threadIdx.x; q < hi; q += (uint64_t)kRun * kThreads) {
    // the four bytes before q: from the data, or at the start of the call from the state
    uint32_t win = q ? ld32u(p + q - 4) : state_window<Kind>(st);
    if (q + kRun <= hi && g0 + q >= 4) {
      uint4 d;
      __builtin_memcpy(&d, p + q, 16);
      const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
      if constexpr (Kind == RPP_SIMILARITY_NILSIMSA) {
        uint4 r4 = rows[win & 255], r3 = rows[(win >> 8) & 255], r2 = rows[(win >> 16) & 255], r1 = rows[win >> 24];
#pragma unroll
        for (uint32_t e = 0; e < kRun; ++e) {
          const uint4 r0 = rows[byte_of(dw[e >> 2], e & 3)];
          nil_full(r0, r1, r2, r3, r4, hist);
          r4 = r3;
          r3 = r2;
          r2 = r1;
          r1 = r0;
        }
      } else {
        uint32_t val = __builtin_bswap32(win);
#pragma unroll
        for (uint32_t e = 0; e < kRun; ++e) {
          val = (val << 8) | byte_of(dw[e >> 2], e & 3);
          bump(hist, sim_bucket(val));
        }
      }
    } else {
      const uint32_t cnt = hi - q < kRun ? (uint32_t)(hi - q) : kRun;
      for (uint32_t e = 0; e < cnt; ++e) {
        const uint32_t w0 = p[q + e];
        step_any<Kind>(w0, win, g0 + q + e, hist, rows);
        win = (win >> 8) | (w0 << 24);
      }
    }
  }
  __syncthreads();
  // bin threadIdx.x: the sum of the waves' counts goes to the state
  uint32_t s = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    s += hist_all[256 * w + threadIdx.x];
    hist_all[256 * w + threadIdx.x] = 0;
  }
  if (s) {
    if constexpr (Kind == RPP_SIMILARITY_NILSIMSA)
      atomicAdd(reinterpret_cast<unsigned long long*>(reinterpret_cast<NilState*>(st)->acc + threadIdx.x),
                (unsigned long long)s);
    else
      atomicAdd(reinterpret_cast<SimState*>(st)->acc + threadIdx.x, s);
  }
  __syncthreads();
}

template <int Kind>
__global__ __launch_bounds__(kThreads) void rpp_similarity_update_kernel(SimJob j) {
  __shared__ uint4 s_rows[256];
  __shared__ uint32_t s_hist[kWaves * 256];
  __shared__ uint64_t s_incl[kThreads];
  __shared__ uint64_t s_wave[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if constexpr (Kind == RPP_SIMILARITY_NILSIMSA)
    s_rows[t] = make_uint4(d_rows.w[t][0], d_rows.w[t][1], d_rows.w[t][2], d_rows.w[t][3]);
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) s_hist[256 * w + t] = 0;
  uint64_t base = 0;  // chunks of the batch before this tile
  for (uint64_t tile = 0; tile < j.n; tile += kThreads) {
    const uint64_t b = tile + t;
    uint64_t v = 0;
    if (b < j.n && (!j.select || j.select[b])) v = (j.sizes[b] + (kChunkBytes - 1)) / kChunkBytes;
    // inclusive block scan of the chunk counts
#pragma unroll
    for (uint32_t d = 1; d < 64; d *= 2) {
      const uint64_t o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) v += s_wave[w];
    s_incl[t] = v;
    __syncthreads();
    const uint64_t total = s_incl[kThreads - 1];
    // this workgroup's chunks: batch chunk index k with k % kGridBlocks == blockIdx.x
    uint64_t k = (blockIdx.x - (uint32_t)base) & (kGridBlocks - 1);  // relative to the tile
    for (; k < total; k += kGridBlocks) {
      uint32_t lo = 0, hi = kThreads - 1;  // the first file of the tile with s_incl > k
      while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (s_incl[mid] > k) hi = mid;
        else lo = mid + 1;
      }
      const uint64_t before = lo ? s_incl[lo - 1] : 0;
      process_chunk<Kind>(j, (uint32_t)(tile + lo), k - before, s_hist, s_rows);
    }
    base += total;
    __syncthreads();
  }
}

template <int Kind>
__global__ __launch_bounds__(kThreads) void rpp_similarity_tail_kernel(SimJob j) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= j.n || (j.select && !j.select[b])) return;
  const uint64_t size = j.sizes[b];
  if (size == 0) return;
  const uint8_t* p = j.data + j.offs[b];
  uint8_t* st = j.states + (size_t)b * state_bytes<Kind>();
  uint32_t win = state_window<Kind>(st);
  for (uint64_t i = size < 4 ? 0 : size - 4; i < size; ++i) win = (win >> 8) | ((uint32_t)p[i] << 24);
  if constexpr (Kind == RPP_SIMILARITY_NILSIMSA) {
    NilState* s = reinterpret_cast<NilState*>(st);
    __builtin_memcpy(s->window, &win, 4);
    s->size += size;
  } else {
    SimState* s = reinterpret_cast<SimState*>(st);
    s->val = __builtin_bswap32(win);
    s->size += size;
  }
}

// one wave per message
template <int Kind>
__global__ __launch_bounds__(64 * kFinalWaves) void rpp_similarity_finalize_kernel(const uint8_t* states,
                                                                                    const uint8_t* select, uint32_t n,
                                                                                    uint8_t* digests) {
  const uint32_t lane = threadIdx.x & 63, b = blockIdx.x * kFinalWaves + (threadIdx.x >> 6);
  if (b >= n || (select && !select[b])) return;  // (uniform in the wave)
  const uint8_t* st = states + (size_t)b * state_bytes<Kind>();
  if constexpr (Kind == RPP_SIMILARITY_NILSIMSA) {
    const NilState* s = reinterpret_cast<const NilState*>(st);
    const uint64_t size = s->size;
    const uint64_t total = size < 3 ? 0 : size == 3 ? 1 : size == 4 ? 4 : 8 * size - 28;
    const uint64_t threshold = total / 256;
    uint64_t word[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) word[k] = __ballot(s->acc[64 * k + lane] > threshold);  // bits 64k .. 64k + 63
    if (lane < 4) {
      const uint64_t w = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
      __builtin_memcpy(digests + 32 * (size_t)b + 8 * lane, &w, 8);
    }
  } else {
    const SimState* s = reinterpret_cast<const SimState*>(st);
    // keys order by count, then by the lower index; four rounds of a wave-wide maximum
    uint64_t key[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) key[k] = ((uint64_t)s->acc[64 * k + lane] << 8) | (255 - (64 * k + lane));
    uint32_t out = 0;
#pragma unroll
    for (uint32_t round = 0; round < 4; ++round) {
      uint64_t best = key[0];
#pragma unroll
      for (uint32_t k = 1; k < 4; ++k) best = key[k] > best ? key[k] : best;
#pragma unroll
      for (uint32_t d = 32; d; d /= 2) {
        const uint64_t o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
      }
      const uint32_t idx = 255 - (uint32_t)(best & 255);
      out = (out << 8) | idx;
      if ((idx & 63) == lane) {  // the winner leaves (a key of zero is below every remaining one)
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          if (k == (idx >> 6)) key[k] = 0;
      }
    }
    if (lane == 0) __builtin_memcpy(digests + 4 * (size_t)b, &out, 4);
  }
}

__global__ void rpp_similarity_has_kernel(const uint64_t* sizes, const uint8_t* select, uint64_t max_size, uint32_t n,
                                          uint8_t* has) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  has[b] = (!select || select[b]) && !(max_size && sizes[b] > max_size) ? 1 : 0;
}

// ---- host ----

int launched() { return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR; }

bool known(int kind) { return kind == RPP_SIMILARITY_NILSIMSA || kind == RPP_SIMILARITY_HISTOGRAM; }

template <int Kind>
int launch_update(const SimJob& j, hipStream_t s) {
  hipLaunchKernelGGL(rpp_similarity_update_kernel<Kind>, dim3(kGridBlocks), dim3(kThreads), 0, s, j);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  hipLaunchKernelGGL(rpp_similarity_tail_kernel<Kind>, dim3((j.n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, j);
  return launched();
}

int launch_update(int kind, const SimJob& j, hipStream_t s) {
  return kind == RPP_SIMILARITY_NILSIMSA ? launch_update<RPP_SIMILARITY_NILSIMSA>(j, s)
                                         : launch_update<RPP_SIMILARITY_HISTOGRAM>(j, s);
}

int launch_finalize(int kind, const uint8_t* states, const uint8_t* select, uint32_t n, uint8_t* digests,
                    hipStream_t s) {
  const dim3 grid((n + kFinalWaves - 1) / kFinalWaves), block(64 * kFinalWaves);
  if (kind == RPP_SIMILARITY_NILSIMSA)
    hipLaunchKernelGGL(rpp_similarity_finalize_kernel<RPP_SIMILARITY_NILSIMSA>, grid, block, 0, s, states, select, n,
                       digests);
  else
    hipLaunchKernelGGL(rpp_similarity_finalize_kernel<RPP_SIMILARITY_HISTOGRAM>, grid, block, 0, s, states, select, n,
                       digests);
  return launched();
}

}  // namespace

extern "C" int rpp_similarity_kind(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "nilsimsa")) return RPP_SIMILARITY_NILSIMSA;
  if (!strcmp(name, "similarity")) return RPP_SIMILARITY_HISTOGRAM;
  return -1;
}

extern "C" uint64_t rpp_similarity_state_bytes(int kind) {
  return kind == RPP_SIMILARITY_NILSIMSA ? sizeof(NilState) : kind == RPP_SIMILARITY_HISTOGRAM ? sizeof(SimState) : 0;
}

extern "C" int rpp_similarity_digest_bytes(int kind) {
  return kind == RPP_SIMILARITY_NILSIMSA ? 32 : kind == RPP_SIMILARITY_HISTOGRAM ? 4 : 0;
}

extern "C" uint64_t rpp_similarity_chunk_bytes(void) { return kChunkBytes; }

extern "C" int rpp_similarity_update_batch(int kind, const uint8_t* d_data, const uint64_t* d_offsets,
                                           const uint64_t* d_sizes, const uint8_t* d_select, uint32_t n,
                                           void* d_states, void* stream) {
  if (!known(kind)) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_states) return RPP_INVALID_ARGUMENT;
  const SimJob j{d_data, d_offsets, d_sizes, d_select, static_cast<uint8_t*>(d_states), n};
  return launch_update(kind, j, (hipStream_t)stream);
}

extern "C" int rpp_similarity_finalize_batch(int kind, const void* d_states, const uint8_t* d_select, uint32_t n,
                                             uint8_t* d_digests, void* stream) {
  if (!known(kind)) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_states || !d_digests) return RPP_INVALID_ARGUMENT;
  return launch_finalize(kind, static_cast<const uint8_t*>(d_states), d_select, n, d_digests, (hipStream_t)stream);
}

// workspace: one state per file
extern "C" uint64_t rpp_similarity_hash_workspace_bytes(int kind, uint32_t n) {
  return rpp_similarity_state_bytes(kind) * (uint64_t)n;
}

extern "C" int rpp_similarity_hash_batch(int kind, const uint8_t* d_data, const uint64_t* d_offsets,
                                         const uint64_t* d_sizes, const uint8_t* d_select, uint64_t max_size,
                                         uint32_t n, uint8_t* d_digests, uint8_t* d_has, void* d_workspace,
                                         uint64_t workspace_bytes, void* stream) {
  if (!known(kind)) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_digests || !d_has || !d_workspace ||
      workspace_bytes < rpp_similarity_hash_workspace_bytes(kind, n))
    return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* states = static_cast<uint8_t*>(d_workspace);
  // d_has = selected and not above max_size; it is the select mask of everything after it
  hipLaunchKernelGGL(rpp_similarity_has_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_sizes, d_select, max_size, n,
                     d_has);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  if (hipMemsetAsync(states, 0, rpp_similarity_hash_workspace_bytes(kind, n), s) != hipSuccess) return RPP_HIP_ERROR;
  const SimJob j{d_data, d_offsets, d_sizes, d_has, states, n};
  const int st = launch_update(kind, j, s);
  if (st != RPP_OK) return st;
  return launch_finalize(kind, states, d_has, n, d_digests, s);
}

// ---- the host restatement: the same states, no GPU ----

extern "C" int rpp_similarity_host_update(int kind, void* state, const uint8_t* data, uint64_t size) {
  if (!known(kind) || !state || (!data && size)) return RPP_INVALID_ARGUMENT;
  if (kind == RPP_SIMILARITY_NILSIMSA) {
    NilState s;
    memcpy(&s, state, sizeof s);
    uint32_t w1 = s.window[3], w2 = s.window[2], w3 = s.window[1], w4 = s.window[0];
    for (uint64_t i = 0; i < size; ++i) {
      const uint32_t w0 = data[i];
      const uint64_t p = s.size + i;
      if (p >= 2) ++s.acc[tran3(kTran, w0, w1, w2, 0)];
      if (p >= 3) {
        ++s.acc[tran3(kTran, w0, w1, w3, 1)];
        ++s.acc[tran3(kTran, w0, w2, w3, 2)];
      }
      if (p >= 4) {
        ++s.acc[tran3(kTran, w0, w1, w4, 3)];
        ++s.acc[tran3(kTran, w0, w2, w4, 4)];
        ++s.acc[tran3(kTran, w0, w3, w4, 5)];
        ++s.acc[tran3(kTran, w4, w1, w0, 6)];
        ++s.acc[tran3(kTran, w4, w3, w0, 7)];
      }
      w4 = w3;
      w3 = w2;
      w2 = w1;
      w1 = w0;
    }
    s.size += size;
    s.window[3] = (uint8_t)w1;
    s.window[2] = (uint8_t)w2;
    s.window[1] = (uint8_t)w3;
    s.window[0] = (uint8_t)w4;
    memcpy(state, &s, sizeof s);
  } else {
    SimState s;
    memcpy(&s, state, sizeof s);
    for (uint64_t i = 0; i < size; ++i) {
      s.val = (s.val << 8) | data[i];
      if (s.size + i >= 3) ++s.acc[sim_bucket(s.val)];
    }
    s.size += size;
    memcpy(state, &s, sizeof s);
  }
  return RPP_OK;
}

extern "C" int rpp_similarity_host_finalize(int kind, const void* state, uint8_t* out) {
  if (!known(kind) || !state || !out) return RPP_INVALID_ARGUMENT;
  if (kind == RPP_SIMILARITY_NILSIMSA) {
    NilState s;
    memcpy(&s, state, sizeof s);
    const uint64_t total = s.size < 3 ? 0 : s.size == 3 ? 1 : s.size == 4 ? 4 : 8 * s.size - 28;
    const uint64_t threshold = total / 256;
    memset(out, 0, 32);
    for (uint32_t i = 0; i < 256; ++i)
      if (s.acc[i] > threshold) out[i >> 3] |= (uint8_t)(1u << (i & 7));
  } else {
    SimState s;
    memcpy(&s, state, sizeof s);
    uint32_t v = 0;
    bool taken[256] = {};
    for (int round = 0; round < 4; ++round) {
      int best = -1;
      for (int i = 0; i < 256; ++i)
        if (!taken[i] && (best < 0 || s.acc[i] > s.acc[best])) best = i;  // (ties: the lower index stays)
      taken[best] = true;
      v = (v << 8) | (uint32_t)best;
    }
    memcpy(out, &v, 4);
  }
  return RPP_OK;
}
