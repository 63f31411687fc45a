// segment_kernels.hip -- the segmenter's match search on MI355X (the rpp_segment_* group of
// include/ricepp_amd.h; src/writer/segmenter.cpp, include/dwarfs/writer/internal/cyclic_hash.h): the
// rsync window hash at every frame position of incoming data, the block index (hash, offset, entered per
// step-aligned window, plus the one-hash bloom filters), the filtered and ordered hit list of an extent, and
// verify-and-extend of candidates.  The sequential control loop of the segmenter stays with the caller.
//
// The hash of the L-byte window at byte q is a = sum x[q+i], b = sum (L-i) x[q+i], both mod 2^16.  All
// arithmetic below is uint32 that wraps mod 2^32, which is exact mod 2^16.
//
//   plan      one workgroup: positions and tiles per extent (sizes are read on the device), their exclusive
//             scans, and the status of the call (an extent of 2^32 frames or more, more tiles than the
//             caller's bound, more hashes than the caller's capacity: nothing is processed).
//   tile      one workgroup per tile of kTile positions of one extent, kRun consecutive positions per thread.
//             The workgroup sums the tile's first window (A0 = sum x_k, B0 = sum k x_k, k relative to the
//             tile); every thread sums, per frame f of its run, the frame that enters the window (at byte
//             L + f g) minus the one that leaves it (at byte f g), plain and weighted by k; a block scan of the
//             threads' totals gives every position r its a = A0 + P1(r) and b = (L + r g) a - (B0 + P2(r)).
//             So a tile reads its L - 1 bytes of halo and nothing depends on another tile.  mode 0 stores the
//             hashes; mode 1 counts the positions whose hash tests positive in the filter; mode 2, after the
//             tile counts were scanned, writes the hits in position order (a block scan of the threads' hit
//             counts: no atomics decide an order).
//   index     one wave per slot hashes its window directly (16 bytes per lane and step) and finds whether it
//             is L equal bytes v; the first such slot of a block per v is found with an atomic minimum, and a
//             second launch marks the entered slots and ORs their bits into the block's and the global filter.
//   extend    one wave per candidate: the window compare, then the backward and the forward extension, 16
//             bytes per lane and step, the first mismatch by ballot.
//
// Nothing outside an extent's or a block's bytes is read.  No 64-bit shift has a variable amount: filter words
// are addressed as uint32 halves (the same bytes, little endian).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ricepp_amd.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kRun = 16;                    // positions per thread
constexpr uint32_t kTile = kThreads * kRun;      // rpp_segment_tile_frames()
constexpr uint32_t kIndexGridY = 1024;           // slot chunks of one block in flight
constexpr uint64_t kMaxFrames = 1ull << 32;      // an extent or a block must be shorter

struct Geometry {
  uint32_t W, g, L, step;  // frames, bytes, bytes, frames
  uint32_t mask32;         // (64-bit filter words - 1): (h >> 6) & mask32 selects the word
};

bool config_ok(const rpp_segment_config* c) {
  if (!c) return false;
  if (c->window_bits < 1 || c->window_bits > 20 || c->granularity < 1 || c->granularity > 64) return false;
  if (c->increment_shift > 31) return false;
  const uint64_t fb = c->filter_bits;
  return fb >= 64 && fb <= (1ull << 32) && (fb & (fb - 1)) == 0;
}

Geometry geometry(const rpp_segment_config* c) {
  Geometry G;
  G.W = 1u << c->window_bits;
  G.g = c->granularity;
  G.L = G.W * G.g;
  const uint32_t s = G.W >> c->increment_shift;
  G.step = s ? s : 1;
  G.mask32 = (uint32_t)(c->filter_bits / 64 - 1);
  return G;
}

__host__ __device__ inline uint64_t positions_of(uint64_t frames, uint32_t W) {
  return frames >= W && frames < kMaxFrames ? frames - W + 1 : 0;
}
__host__ __device__ inline uint64_t slots_of(uint64_t frames, uint32_t W, uint32_t step) {
  return frames >= W && frames < kMaxFrames ? (frames - W) / step + 1 : 0;
}

// ---- device ----

struct Plan {  // the head of every workspace
  uint64_t tiles;   // tiles (hash, scan) of the call; 0 when the status is not RPP_OK
  uint64_t total;   // positions (hash), slots (index)
  int32_t status;
  uint32_t pad;
};

__device__ __forceinline__ uint32_t ld8(const uint8_t* p) { return *p; }

// inclusive scan over the workgroup's kThreads values; s_wave: kWaves entries; all threads call it
template <typename T>
__device__ __forceinline__ T block_inclusive(T v, T* s_wave) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d *= 2) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();  // (s_wave may still be read from an earlier scan)
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  for (uint32_t w = 0; w < wave; ++w) v += s_wave[w];
  return v;
}

// plan of a hash or scan call; one workgroup
__global__ __launch_bounds__(kThreads) void rpp_segment_plan_kernel(const uint64_t* sizes, uint32_t n, uint32_t W,
                                                                    uint64_t tile_cap, uint64_t pos_cap, Plan* plan,
                                                                    uint64_t* tile_start, uint64_t* pos_start) {
  __shared__ uint64_t s_wave[kWaves];
  __shared__ uint64_t s_tot[2];
  __shared__ int s_bad;
  const uint32_t t = threadIdx.x;
  if (t == 0) s_bad = 0;
  __syncthreads();
  uint64_t tiles_before = 0, pos_before = 0;
  for (uint64_t base = 0; base < n; base += kThreads) {
    const uint64_t b = base + t;
    uint64_t np = 0;
    if (b < n) {
      const uint64_t f = sizes[b];
      if (f >= kMaxFrames) s_bad = 1;  // (benign race: every writer stores 1)
      np = positions_of(f, W);
    }
    const uint64_t nt = (np + kTile - 1) / kTile;
    const uint64_t it = block_inclusive(nt, s_wave);
    const uint64_t ip = block_inclusive(np, s_wave);
    if (b < n) {
      tile_start[b] = tiles_before + it - nt;
      pos_start[b] = pos_before + ip - np;
    }
    if (t == kThreads - 1) {
      s_tot[0] = it;
      s_tot[1] = ip;
    }
    __syncthreads();
    tiles_before += s_tot[0];
    pos_before += s_tot[1];
    __syncthreads();
  }
  if (t == 0) {
    tile_start[n] = tiles_before;
    pos_start[n] = pos_before;
    int32_t st = RPP_OK;
    if (s_bad || tiles_before > tile_cap) st = RPP_INVALID_ARGUMENT;
    else if (pos_before > pos_cap) st = RPP_OUTPUT_TOO_SMALL;
    plan->tiles = st == RPP_OK ? tiles_before : 0;
    plan->total = pos_before;
    plan->status = st;
    plan->pad = 0;
  }
}

struct TileJob {
  const uint8_t* data;
  const uint64_t* offs;   // bytes
  const uint64_t* sizes;  // frames
  uint32_t n;
  Geometry G;
  const Plan* plan;
  const uint64_t* tile_start;  // n + 1
  const uint64_t* pos_start;   // n + 1
  // mode 0
  uint32_t* hashes;
  // modes 1, 2
  const uint32_t* filter32;
  uint32_t* tile_counts;
  const uint64_t* tile_hit_start;
  rpp_segment_hit* hits;
  uint64_t capacity;
};

__device__ __forceinline__ bool filter_test(const uint32_t* f32, uint32_t mask32, uint32_t h) {
  const uint32_t w = f32[(((h >> 6) & mask32) << 1) | ((h >> 5) & 1)];
  return (w >> (h & 31)) & 1;
}

// bytes [0, cnt) of p as a sum and a sum weighted by (k0 + i); 16-byte loads where cnt allows
__device__ __forceinline__ void sum_span(const uint8_t* p, uint32_t cnt, uint32_t k0, uint32_t& s1, uint32_t& s2) {
  uint32_t i = 0;
  for (; i + 16 <= cnt; i += 16) {
    uint4 d;
    __builtin_memcpy(&d, p + i, 16);
    const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (uint32_t e = 0; e < 16; ++e) {
      const uint32_t x = (dw[e >> 2] >> (8 * (e & 3))) & 255;
      s1 += x;
      s2 += (k0 + i + e) * x;
    }
  }
  for (; i < cnt; ++i) {
    const uint32_t x = ld8(p + i);
    s1 += x;
    s2 += (k0 + i) * x;
  }
}

// GT: the granularity as a compile-time constant (1, 2, 3, 4, 6), or 0 for the variable path
template <uint32_t GT>
__global__ __launch_bounds__(kThreads) void rpp_segment_tile_kernel(TileJob j, uint32_t mode) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_red[2 * kWaves];
  __shared__ uint32_t s_ext;
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint64_t k = blockIdx.x;
  if (k >= j.plan->tiles) return;  // (uniform: also every tile of a call whose plan failed)
  if (t == 0) {  // the last extent whose first tile is at or before k
    uint32_t lo = 0, hi = j.n - 1;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (j.tile_start[mid] <= k) lo = mid;
      else hi = mid - 1;
    }
    s_ext = lo;
  }
  __syncthreads();
  const uint32_t b = s_ext;
  const uint32_t g = GT ? GT : j.G.g, L = j.G.L, W = j.G.W;
  const uint64_t frames = j.sizes[b];
  const uint64_t npos = frames - W + 1;
  const uint64_t p0 = (k - j.tile_start[b]) * kTile;       // the tile's first position
  const uint32_t cnt = npos - p0 < kTile ? (uint32_t)(npos - p0) : kTile;
  const uint8_t* base = j.data + j.offs[b] + p0 * g;        // tile-relative byte 0

  // A0, B0 of the tile's first window
  uint32_t a0 = 0, b0 = 0;
  {
    const uint32_t chunks = L / 16;
    for (uint32_t c = t; c < chunks; c += kThreads) sum_span(base + 16 * c, 16, 16 * c, a0, b0);
    if (t == 0) sum_span(base + 16 * chunks, L - 16 * chunks, 16 * chunks, a0, b0);
#pragma unroll
    for (uint32_t d = 32; d; d /= 2) {
      a0 += __shfl_xor(a0, d, 64);
      b0 += __shfl_xor(b0, d, 64);
    }
    if (lane == 0) {
      s_red[2 * wave] = a0;
      s_red[2 * wave + 1] = b0;
    }
    __syncthreads();
    a0 = b0 = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      a0 += s_red[2 * w];
      b0 += s_red[2 * w + 1];
    }
  }

  // per frame f of the run: d1 = sum(in) - sum(out), d2 = sum(k in) - sum(k out), k relative to the tile
  const uint32_t r0 = t * kRun;
  uint32_t d1[kRun], d2[kRun];
  // frames of the run whose entering frame exists: position p0 + r0 + f + 1 needs frame p0 + r0 + f + W
  const uint64_t first_in = p0 + r0 + W;
  const uint32_t have = first_in >= frames ? 0 : frames - first_in < kRun ? (uint32_t)(frames - first_in) : kRun;
  const uint8_t* po = base + (uint64_t)r0 * g;
  const uint8_t* pi = po + L;
  if (GT && have == kRun) {
    uint32_t wo[4 * (GT ? GT : 1)], wi[4 * (GT ? GT : 1)];
    __builtin_memcpy(wo, po, 16 * (GT ? GT : 1));
    __builtin_memcpy(wi, pi, 16 * (GT ? GT : 1));
    const uint32_t kb = r0 * g;
#pragma unroll
    for (uint32_t f = 0; f < kRun; ++f) {
      uint32_t s1 = 0, s2 = 0, sin = 0;
#pragma unroll
      for (uint32_t i = 0; i < (GT ? GT : 1); ++i) {
        const uint32_t c = f * (GT ? GT : 1) + i;
        const uint32_t xo = (wo[c >> 2] >> (8 * (c & 3))) & 255, xi = (wi[c >> 2] >> (8 * (c & 3))) & 255;
        s1 += xi - xo;
        s2 += (kb + c) * (xi - xo);
        sin += xi;
      }
      d1[f] = s1;
      d2[f] = s2 + L * sin;
    }
  } else {
#pragma unroll
    for (uint32_t f = 0; f < kRun; ++f) {
      uint32_t s1 = 0, s2 = 0;
      if (f < have) {
        for (uint32_t i = 0; i < g; ++i) {
          const uint32_t c = f * g + i, kk = r0 * g + c;
          const uint32_t xo = ld8(po + c), xi = ld8(pi + c);
          s1 += xi - xo;
          s2 += (kk + L) * xi - kk * xo;
        }
      }
      d1[f] = s1;
      d2[f] = s2;
    }
  }
  uint32_t t1 = 0, t2 = 0;
#pragma unroll
  for (uint32_t f = 0; f < kRun; ++f) {
    t1 += d1[f];
    t2 += d2[f];
  }
  uint32_t pa = a0 + block_inclusive(t1, s_wave) - t1;
  uint32_t pb = b0 + block_inclusive(t2, s_wave) - t2;

  uint32_t h[kRun];
#pragma unroll
  for (uint32_t f = 0; f < kRun; ++f) {
    const uint32_t bb = (L + (r0 + f) * g) * pa - pb;
    h[f] = (pa & 0xffffu) | (bb << 16);
    pa += d1[f];
    pb += d2[f];
  }
  const uint32_t mine = r0 >= cnt ? 0 : cnt - r0 < kRun ? cnt - r0 : kRun;  // positions of the run in the tile

  if (mode == 0) {
    uint32_t* out = j.hashes + j.pos_start[b] + p0 + r0;
#pragma unroll
    for (uint32_t f = 0; f < kRun; ++f)
      if (f < mine) out[f] = h[f];
    return;
  }
  uint32_t hitmask = 0;
#pragma unroll
  for (uint32_t f = 0; f < kRun; ++f)
    if (f < mine && filter_test(j.filter32, j.G.mask32, h[f])) hitmask |= 1u << f;
  const uint32_t c = __popc(hitmask);
  const uint32_t incl = block_inclusive(c, s_wave);
  if (mode == 1) {
    if (t == kThreads - 1) j.tile_counts[k] = incl;
    return;
  }
  uint64_t at = j.tile_hit_start[k] + (incl - c);
#pragma unroll
  for (uint32_t f = 0; f < kRun; ++f)
    if ((hitmask >> f) & 1) {
      if (at < j.capacity) {
        rpp_segment_hit hit;
        hit.pos = (uint32_t)(p0 + r0 + f);
        hit.hash = h[f];
        j.hits[at] = hit;
      }
      ++at;
    }
}

// exclusive scan of the tile counts, the hit ranges of the extents, the result; one workgroup
__global__ __launch_bounds__(kThreads) void rpp_segment_hit_scan_kernel(const Plan* plan, const uint32_t* tile_counts,
                                                                        uint64_t* tile_hit_start,
                                                                        const uint64_t* tile_start, uint32_t n,
                                                                        uint64_t capacity, uint64_t* hit_start,
                                                                        rpp_segment_scan_result* result) {
  __shared__ uint64_t s_wave[kWaves];
  __shared__ uint64_t s_tot;
  const uint32_t t = threadIdx.x;
  const uint64_t tiles = plan->tiles;
  uint64_t before = 0;
  for (uint64_t base = 0; base < tiles; base += kThreads) {
    const uint64_t i = base + t;
    const uint64_t v = i < tiles ? tile_counts[i] : 0;
    const uint64_t incl = block_inclusive(v, s_wave);
    if (i < tiles) tile_hit_start[i] = before + incl - v;
    if (t == kThreads - 1) s_tot = incl;
    __syncthreads();
    before += s_tot;
    __syncthreads();
  }
  if (t == 0) tile_hit_start[tiles] = before;
  __syncthreads();  // (the workgroup's own global stores are visible to it after the barrier)
  if (hit_start)
    for (uint64_t b = t; b <= n; b += kThreads) {
      const uint64_t ts = plan->status == RPP_OK ? tile_start[b] : 0;
      hit_start[b] = ts >= tiles ? before : tile_hit_start[ts];
    }
  if (t == 0) {
    result->count = before;
    result->status = plan->status != RPP_OK ? plan->status : before > capacity ? RPP_OUTPUT_TOO_SMALL : RPP_OK;
    result->reserved = 0;
  }
}

__global__ void rpp_segment_status_kernel(const Plan* plan, int32_t* status) { *status = plan->status; }

// ---- index ----

__global__ __launch_bounds__(kThreads) void rpp_segment_index_plan_kernel(const uint64_t* sizes, uint32_t n, uint32_t W,
                                                                          uint32_t step, uint64_t slot_cap, Plan* plan,
                                                                          uint64_t* slot_start, int32_t* status) {
  __shared__ uint64_t s_wave[kWaves];
  __shared__ uint64_t s_tot;
  __shared__ int s_bad;
  const uint32_t t = threadIdx.x;
  if (t == 0) s_bad = 0;
  __syncthreads();
  uint64_t before = 0;
  for (uint64_t base = 0; base < n; base += kThreads) {
    const uint64_t b = base + t;
    uint64_t ns = 0;
    if (b < n) {
      const uint64_t f = sizes[b];
      if (f >= kMaxFrames) s_bad = 1;
      ns = slots_of(f, W, step);
    }
    const uint64_t incl = block_inclusive(ns, s_wave);
    if (b < n) slot_start[b] = before + incl - ns;
    if (t == kThreads - 1) s_tot = incl;
    __syncthreads();
    before += s_tot;
    __syncthreads();
  }
  if (t == 0) {
    slot_start[n] = before;
    const int32_t st = s_bad ? RPP_INVALID_ARGUMENT : before > slot_cap ? RPP_OUTPUT_TOO_SMALL : RPP_OK;
    plan->tiles = 0;
    plan->total = before;
    plan->status = st;
    plan->pad = 0;
    *status = st;
  }
}

struct IndexJob {
  const uint8_t* data;
  const uint64_t* offs;
  const uint64_t* sizes;
  uint32_t n;
  Geometry G;
  const Plan* plan;
  const uint64_t* slot_start;
  uint32_t* first;  // n x 256: the first slot of the block whose window is all v
  uint32_t* hash;
  uint32_t* offset;
  uint8_t* entered;  // after the hash kernel: 1, or 2 for a window of equal bytes
  uint32_t* block_filters32;
  uint32_t* global_filter32;
};

// one wave per slot; grid (blocks of the batch, slot chunks)
__global__ __launch_bounds__(kThreads) void rpp_segment_index_hash_kernel(IndexJob j) {
  if (j.plan->status != RPP_OK) return;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const uint32_t L = j.G.L;
  const uint64_t ns = slots_of(j.sizes[b], j.G.W, j.G.step);
  const uint8_t* blk = j.data + j.offs[b];
  for (uint64_t s = (uint64_t)blockIdx.y * kWaves + wave; s < ns; s += (uint64_t)gridDim.y * kWaves) {
    const uint64_t off = s * j.G.step;  // frames
    const uint8_t* p = blk + off * j.G.g;
    const uint32_t v = ld8(p);
    const uint32_t v4 = v * 0x01010101u;
    uint32_t a = 0, wsum = 0;  // wsum = sum i x_i
    bool same = true;
    for (uint32_t i = 16 * lane; i < L; i += 16 * 64) {
      if (i + 16 <= L) {
        uint4 d;
        __builtin_memcpy(&d, p + i, 16);
        same = same && d.x == v4 && d.y == v4 && d.z == v4 && d.w == v4;
        const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (uint32_t e = 0; e < 16; ++e) {
          const uint32_t x = (dw[e >> 2] >> (8 * (e & 3))) & 255;
          a += x;
          wsum += (i + e) * x;
        }
      } else {
        for (uint32_t e = i; e < L; ++e) {
          const uint32_t x = ld8(p + e);
          same = same && x == v;
          a += x;
          wsum += e * x;
        }
      }
    }
#pragma unroll
    for (uint32_t d = 32; d; d /= 2) {
      a += __shfl_xor(a, d, 64);
      wsum += __shfl_xor(wsum, d, 64);
    }
    const bool all_same = __all(same);
    if (lane == 0) {
      const uint64_t at = j.slot_start[b] + s;
      const uint32_t bb = L * a - wsum;
      j.hash[at] = (a & 0xffffu) | (bb << 16);
      j.offset[at] = (uint32_t)off;
      j.entered[at] = all_same ? 2 : 1;
      if (all_same) atomicMin(j.first + 256 * (size_t)b + v, (uint32_t)s);
    }
  }
}

// one thread per slot; grid (blocks of the batch, slot chunks)
__global__ __launch_bounds__(kThreads) void rpp_segment_index_enter_kernel(IndexJob j) {
  if (j.plan->status != RPP_OK) return;
  const uint32_t b = blockIdx.x;
  const uint64_t ns = slots_of(j.sizes[b], j.G.W, j.G.step);
  const uint8_t* blk = j.data + j.offs[b];
  const uint32_t words32 = 2 * (j.G.mask32 + 1);
  for (uint64_t s = (uint64_t)blockIdx.y * kThreads + threadIdx.x; s < ns; s += (uint64_t)gridDim.y * kThreads) {
    const uint64_t at = j.slot_start[b] + s;
    uint32_t e = j.entered[at];
    if (e == 2) {
      const uint32_t v = ld8(blk + s * j.G.step * j.G.g);
      e = j.first[256 * (size_t)b + v] == (uint32_t)s ? 1 : 0;
      j.entered[at] = (uint8_t)e;
    }
    if (e) {
      const uint32_t h = j.hash[at];
      const uint32_t w = (((h >> 6) & j.G.mask32) << 1) | ((h >> 5) & 1), bit = 1u << (h & 31);
      atomicOr(j.block_filters32 + (size_t)b * words32 + w, bit);
      atomicOr(j.global_filter32 + w, bit);
    }
  }
}

// ---- extend ----

// the bytes of two 16-byte pieces that agree, counted from the low (Forward) or the high address
template <bool Forward>
__device__ __forceinline__ uint32_t agree16(const uint8_t* x, const uint8_t* y) {
  uint64_t a[2], c[2];
  __builtin_memcpy(a, x, 16);
  __builtin_memcpy(c, y, 16);
  const uint64_t lo = a[0] ^ c[0], hi = a[1] ^ c[1];
  if (Forward) return lo ? (uint32_t)__builtin_ctzll(lo) / 8 : hi ? 8 + (uint32_t)__builtin_ctzll(hi) / 8 : 16;
  return hi ? (uint32_t)__builtin_clzll(hi) / 8 : lo ? 8 + (uint32_t)__builtin_clzll(lo) / 8 : 16;
}

// the length of the common run of x and y, at most `limit` bytes, forwards from x[0], y[0] or backwards from
// x[-1], y[-1]; by one wave, every lane returns the result
template <bool Forward>
__device__ uint64_t common_run(const uint8_t* x, const uint8_t* y, uint64_t limit) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t base = 0; base < limit; base += 1024) {
    const uint64_t d = base + 16 * lane;  // the distance of the lane's piece
    const uint32_t cnt = d >= limit ? 0 : limit - d < 16 ? (uint32_t)(limit - d) : 16;
    uint32_t m = 0;
    if (cnt == 16) {
      m = Forward ? agree16<true>(x + d, y + d) : agree16<false>(x - d - 16, y - d - 16);
    } else {
      for (; m < cnt; ++m) {
        const int64_t o = Forward ? (int64_t)(d + m) : -(int64_t)(d + m) - 1;
        if (x[o] != y[o]) break;
      }
    }
    const uint64_t stop = __ballot(m != 16);
    if (stop) {
      const uint32_t l = (uint32_t)__builtin_ctzll(stop);
      return base + 16 * l + __shfl(m, l, 64);
    }
  }
  return limit;
}

__device__ __forceinline__ bool candidate_ok(const rpp_segment_candidate& c, uint32_t W) {
  return (uint64_t)c.off + W <= c.block_frames && (uint64_t)c.pos + W <= c.end && c.begin <= c.pos;
}

__global__ __launch_bounds__(kThreads) void rpp_segment_extend_kernel(const uint8_t* ext_data, const uint8_t* blk_data,
                                                                      const rpp_segment_candidate* cand, uint32_t n,
                                                                      Geometry G, rpp_segment_match* out) {
  const uint32_t lane = threadIdx.x & 63, i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= n) return;  // (uniform in the wave)
  const rpp_segment_candidate c = cand[i];
  rpp_segment_match m;
  m.off = c.off;
  m.pos = c.pos;
  m.size = 0;
  if (candidate_ok(c, G.W)) {
    const uint64_t g = G.g;
    const uint8_t* x = ext_data + c.extent_offset + c.pos * g;
    const uint8_t* y = blk_data + c.block_offset + c.off * g;
    if (common_run<true>(x, y, G.L) == G.L) {
      const uint64_t begin = c.pos > c.off && c.pos - c.off > c.begin ? c.pos - c.off : c.begin;
      const uint64_t reach = (uint64_t)c.pos + c.block_frames - c.off;
      const uint64_t end = reach < c.end ? reach : c.end;
      const uint64_t prefix = common_run<false>(x, y, (c.pos - begin) * g) / g;
      const uint64_t suffix = common_run<true>(x + G.L, y + G.L, (end - c.pos - G.W) * g) / g;
      m.off = (uint32_t)(c.off - prefix);
      m.pos = (uint32_t)(c.pos - prefix);
      m.size = (uint32_t)(G.W + prefix + suffix);
    }
  }
  if (lane == 0) out[i] = m;
}

// ---- host ----

int launched() { return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR; }

uint64_t align16(uint64_t v) { return (v + 15) & ~15ull; }

uint64_t tile_cap_of(uint32_t n, uint64_t total_frames) { return total_frames / kTile + n; }

struct HashWs {
  uint64_t tile_start, pos_start, counts, hit_start, bytes;
};
HashWs hash_ws(uint32_t n, uint64_t total_frames, bool scan) {
  HashWs w;
  w.tile_start = align16(sizeof(Plan));
  w.pos_start = w.tile_start + align16(8ull * (n + 1ull));
  w.counts = w.pos_start + align16(8ull * (n + 1ull));
  const uint64_t cap = tile_cap_of(n, total_frames);
  w.hit_start = w.counts + (scan ? align16(4 * cap) : 0);
  w.bytes = w.hit_start + (scan ? align16(8 * (cap + 1)) : 0);
  return w;
}

void launch_tile(const TileJob& j, uint32_t mode, uint64_t tiles, hipStream_t s) {
  const dim3 grid((uint32_t)tiles), block(kThreads);
  switch (j.G.g) {
    case 1: hipLaunchKernelGGL(rpp_segment_tile_kernel<1>, grid, block, 0, s, j, mode); break;
    case 2: hipLaunchKernelGGL(rpp_segment_tile_kernel<2>, grid, block, 0, s, j, mode); break;
    case 3: hipLaunchKernelGGL(rpp_segment_tile_kernel<3>, grid, block, 0, s, j, mode); break;
    case 4: hipLaunchKernelGGL(rpp_segment_tile_kernel<4>, grid, block, 0, s, j, mode); break;
    case 6: hipLaunchKernelGGL(rpp_segment_tile_kernel<6>, grid, block, 0, s, j, mode); break;
    default: hipLaunchKernelGGL(rpp_segment_tile_kernel<0>, grid, block, 0, s, j, mode); break;
  }
}

// the rolling hash of the host restatement: add the in-byte, subtract len * out
struct Rolling {
  uint32_t a = 0, b = 0, len;
  explicit Rolling(uint32_t l) : len(l) {}
  void push(uint8_t in) {  // while the window fills
    a += in;
    b += a;
  }
  void roll(uint8_t out, uint8_t in) {
    a = a - out + in;
    b = b - len * out + a;
  }
  uint32_t value() const { return (a & 0xffffu) | (b << 16); }
};

void host_filter_set(uint64_t* f, uint32_t mask, uint32_t h) { f[(h >> 6) & mask] |= 1ull << (h & 63); }
bool host_filter_test(const uint64_t* f, uint32_t mask, uint32_t h) { return (f[(h >> 6) & mask] >> (h & 63)) & 1; }

}  // namespace

extern "C" int rpp_segment_check_config(const rpp_segment_config* cfg) {
  return config_ok(cfg) ? RPP_OK : RPP_UNSUPPORTED_CONFIG;
}

extern "C" uint64_t rpp_segment_tile_frames(void) { return kTile; }

extern "C" uint64_t rpp_segment_positions(const rpp_segment_config* cfg, uint64_t frames) {
  return config_ok(cfg) ? positions_of(frames, 1u << cfg->window_bits) : 0;
}

extern "C" uint64_t rpp_segment_index_slots(const rpp_segment_config* cfg, uint64_t frames) {
  if (!config_ok(cfg)) return 0;
  const Geometry G = geometry(cfg);
  return slots_of(frames, G.W, G.step);
}

extern "C" uint64_t rpp_segment_hash_workspace_bytes(uint32_t n, uint64_t total_frames) {
  return hash_ws(n, total_frames, false).bytes;
}
extern "C" uint64_t rpp_segment_scan_workspace_bytes(uint32_t n, uint64_t total_frames) {
  return hash_ws(n, total_frames, true).bytes;
}
extern "C" uint64_t rpp_segment_index_workspace_bytes(uint32_t n) { return align16(sizeof(Plan)) + 1024ull * n; }

extern "C" int rpp_segment_hash_batch(const rpp_segment_config* cfg, const uint8_t* d_data, const uint64_t* d_offsets,
                                      const uint64_t* d_sizes, uint32_t n, uint64_t total_frames, uint32_t* d_hashes,
                                      uint64_t hash_capacity, uint64_t* d_hash_start, int32_t* d_status,
                                      void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (n == 0) return RPP_OK;
  const HashWs w = hash_ws(n, total_frames, false);
  const uint64_t cap = tile_cap_of(n, total_frames);
  if (!d_data || !d_offsets || !d_sizes || !d_hash_start || !d_status || !d_workspace || workspace_bytes < w.bytes ||
      (!d_hashes && hash_capacity) || cap >= (1ull << 31))
    return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = static_cast<uint8_t*>(d_workspace);
  const Geometry G = geometry(cfg);
  Plan* plan = reinterpret_cast<Plan*>(ws);
  uint64_t* tile_start = reinterpret_cast<uint64_t*>(ws + w.tile_start);
  hipLaunchKernelGGL(rpp_segment_plan_kernel, dim3(1), dim3(kThreads), 0, s, d_sizes, n, G.W, cap, hash_capacity, plan,
                     tile_start, d_hash_start);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  hipLaunchKernelGGL(rpp_segment_status_kernel, dim3(1), dim3(1), 0, s, plan, d_status);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  if (cap == 0) return RPP_OK;
  TileJob j{};
  j.data = d_data;
  j.offs = d_offsets;
  j.sizes = d_sizes;
  j.n = n;
  j.G = G;
  j.plan = plan;
  j.tile_start = tile_start;
  j.pos_start = d_hash_start;
  j.hashes = d_hashes;
  launch_tile(j, 0, cap, s);
  return launched();
}

extern "C" int rpp_segment_scan_batch(const rpp_segment_config* cfg, const uint8_t* d_data, const uint64_t* d_offsets,
                                      const uint64_t* d_sizes, uint32_t n, uint64_t total_frames,
                                      const uint64_t* d_filter, rpp_segment_hit* d_hits, uint64_t capacity,
                                      uint64_t* d_hit_start, rpp_segment_scan_result* d_result, void* d_workspace,
                                      uint64_t workspace_bytes, void* stream) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (!d_result) return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hipMemsetAsync(d_result, 0, sizeof *d_result, s) == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
  const HashWs w = hash_ws(n, total_frames, true);
  const uint64_t cap = tile_cap_of(n, total_frames);
  if (!d_data || !d_offsets || !d_sizes || !d_filter || !d_workspace || workspace_bytes < w.bytes ||
      (!d_hits && capacity) || cap >= (1ull << 31))
    return RPP_INVALID_ARGUMENT;
  uint8_t* ws = static_cast<uint8_t*>(d_workspace);
  const Geometry G = geometry(cfg);
  Plan* plan = reinterpret_cast<Plan*>(ws);
  uint64_t* tile_start = reinterpret_cast<uint64_t*>(ws + w.tile_start);
  uint64_t* pos_start = reinterpret_cast<uint64_t*>(ws + w.pos_start);
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + w.counts);
  uint64_t* tile_hit_start = reinterpret_cast<uint64_t*>(ws + w.hit_start);
  hipLaunchKernelGGL(rpp_segment_plan_kernel, dim3(1), dim3(kThreads), 0, s, d_sizes, n, G.W, cap, ~0ull, plan,
                     tile_start, pos_start);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  TileJob j{};
  j.data = d_data;
  j.offs = d_offsets;
  j.sizes = d_sizes;
  j.n = n;
  j.G = G;
  j.plan = plan;
  j.tile_start = tile_start;
  j.pos_start = pos_start;
  j.filter32 = reinterpret_cast<const uint32_t*>(d_filter);
  j.tile_counts = counts;
  j.tile_hit_start = tile_hit_start;
  j.hits = d_hits;
  j.capacity = capacity;
  if (cap) {
    launch_tile(j, 1, cap, s);
    if (launched() != RPP_OK) return RPP_HIP_ERROR;
  }
  hipLaunchKernelGGL(rpp_segment_hit_scan_kernel, dim3(1), dim3(kThreads), 0, s, plan, counts, tile_hit_start,
                     tile_start, n, capacity, d_hit_start, d_result);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  if (cap) launch_tile(j, 2, cap, s);
  return launched();
}

extern "C" int rpp_segment_index_batch(const rpp_segment_config* cfg, const uint8_t* d_data, const uint64_t* d_offsets,
                                       const uint64_t* d_sizes, uint32_t n, uint64_t max_block_frames,
                                       uint32_t* d_hash, uint32_t* d_offset, uint8_t* d_entered, uint64_t slot_capacity,
                                       uint64_t* d_slot_start, uint64_t* d_block_filters, uint64_t* d_global_filter,
                                       int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_slot_start || !d_block_filters || !d_global_filter || !d_status ||
      !d_workspace || workspace_bytes < rpp_segment_index_workspace_bytes(n) || n >= (1u << 31) ||
      (slot_capacity && (!d_hash || !d_offset || !d_entered)))
    return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = static_cast<uint8_t*>(d_workspace);
  const Geometry G = geometry(cfg);
  Plan* plan = reinterpret_cast<Plan*>(ws);
  uint32_t* first = reinterpret_cast<uint32_t*>(ws + align16(sizeof(Plan)));
  hipLaunchKernelGGL(rpp_segment_index_plan_kernel, dim3(1), dim3(kThreads), 0, s, d_sizes, n, G.W, G.step,
                     slot_capacity, plan, d_slot_start, d_status);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  if (hipMemsetAsync(first, 0xff, 1024ull * n, s) != hipSuccess) return RPP_HIP_ERROR;
  const uint64_t max_slots = slots_of(max_block_frames < kMaxFrames ? max_block_frames : kMaxFrames - 1, G.W, G.step);
  if (max_slots == 0 || slot_capacity == 0) return RPP_OK;
  IndexJob j{d_data, d_offsets, d_sizes, n, G, plan, d_slot_start, first, d_hash, d_offset, d_entered,
             reinterpret_cast<uint32_t*>(d_block_filters), reinterpret_cast<uint32_t*>(d_global_filter)};
  auto chunks = [&](uint64_t per) {
    const uint64_t c = (max_slots + per - 1) / per;
    return (uint32_t)(c < kIndexGridY ? c : kIndexGridY);
  };
  hipLaunchKernelGGL(rpp_segment_index_hash_kernel, dim3(n, chunks(kWaves)), dim3(kThreads), 0, s, j);
  if (launched() != RPP_OK) return RPP_HIP_ERROR;
  hipLaunchKernelGGL(rpp_segment_index_enter_kernel, dim3(n, chunks(kThreads)), dim3(kThreads), 0, s, j);
  return launched();
}

extern "C" int rpp_segment_extend_batch(const rpp_segment_config* cfg, const uint8_t* d_extent_data,
                                        const uint8_t* d_block_data, const rpp_segment_candidate* d_candidates,
                                        uint32_t n, rpp_segment_match* d_matches, void* stream) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (n == 0) return RPP_OK;
  if (!d_extent_data || !d_block_data || !d_candidates || !d_matches) return RPP_INVALID_ARGUMENT;
  hipLaunchKernelGGL(rpp_segment_extend_kernel, dim3((n + kWaves - 1) / kWaves), dim3(kThreads), 0,
                     (hipStream_t)stream, d_extent_data, d_block_data, d_candidates, n, geometry(cfg), d_matches);
  return launched();
}

// ---- the host restatement: the rolling update and a sequential index build, no GPU ----

extern "C" int rpp_segment_host_hashes(const rpp_segment_config* cfg, const uint8_t* data, uint64_t frames,
                                       uint32_t* out) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (frames >= kMaxFrames) return RPP_INVALID_ARGUMENT;
  const Geometry G = geometry(cfg);
  if (frames < G.W) return RPP_OK;
  if (!data || !out) return RPP_INVALID_ARGUMENT;
  Rolling r(G.L);
  for (uint32_t i = 0; i < G.L; ++i) r.push(data[i]);
  out[0] = r.value();
  for (uint64_t p = 1; p + G.W <= frames; ++p) {
    const uint8_t* q = data + (p - 1) * G.g;
    for (uint32_t i = 0; i < G.g; ++i) r.roll(q[i], q[i + G.L]);
    out[p] = r.value();
  }
  return RPP_OK;
}

extern "C" int rpp_segment_host_index(const rpp_segment_config* cfg, const uint8_t* block, uint64_t frames,
                                      uint32_t* hash, uint32_t* offset, uint8_t* entered, uint64_t* block_filter,
                                      uint64_t* global_filter) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (frames >= kMaxFrames) return RPP_INVALID_ARGUMENT;
  const Geometry G = geometry(cfg);
  if (frames < G.W) return RPP_OK;
  if (!block || !hash || !offset || !entered || !block_filter || !global_filter) return RPP_INVALID_ARGUMENT;
  // the block fills byte by byte, as append_bytes sees it: the window ending at frame m * step is slot m
  Rolling r(G.L);
  bool seen[256] = {};
  uint64_t run = 0;  // equal bytes ending at the current one
  uint64_t slot = 0;
  const uint64_t bytes = frames * G.g;
  for (uint64_t i = 0; i < bytes; ++i) {
    run = i && block[i] == block[i - 1] ? run + 1 : 1;
    if (i < G.L) r.push(block[i]);
    else r.roll(block[i - G.L], block[i]);
    if ((i + 1) % G.g) continue;
    const uint64_t f = (i + 1) / G.g;  // frames so far
    if (f < G.W || f % G.step) continue;
    const uint32_t h = r.value();
    bool enter = true;
    if (run >= G.L) {
      enter = !seen[block[i]];
      seen[block[i]] = true;
    }
    hash[slot] = h;
    offset[slot] = (uint32_t)(f - G.W);
    entered[slot] = enter ? 1 : 0;
    if (enter) {
      host_filter_set(block_filter, G.mask32, h);
      host_filter_set(global_filter, G.mask32, h);
    }
    ++slot;
  }
  return RPP_OK;
}

extern "C" int rpp_segment_host_scan(const rpp_segment_config* cfg, const uint8_t* data, uint64_t frames,
                                     const uint64_t* filter, rpp_segment_hit* hits, uint64_t capacity,
                                     uint64_t* count) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (!count || frames >= kMaxFrames) return RPP_INVALID_ARGUMENT;
  *count = 0;
  const Geometry G = geometry(cfg);
  if (frames < G.W) return RPP_OK;
  if (!data || !filter || (!hits && capacity)) return RPP_INVALID_ARGUMENT;
  Rolling r(G.L);
  for (uint32_t i = 0; i < G.L; ++i) r.push(data[i]);
  uint64_t c = 0;
  for (uint64_t p = 0;; ++p) {
    const uint32_t h = r.value();
    if (host_filter_test(filter, G.mask32, h)) {
      if (c < capacity) hits[c] = rpp_segment_hit{(uint32_t)p, h};
      ++c;
    }
    if (p + 1 + G.W > frames) break;
    const uint8_t* q = data + p * G.g;
    for (uint32_t i = 0; i < G.g; ++i) r.roll(q[i], q[i + G.L]);
  }
  *count = c;
  return c > capacity ? RPP_OUTPUT_TOO_SMALL : RPP_OK;
}

extern "C" int rpp_segment_host_extend(const rpp_segment_config* cfg, const uint8_t* extent_data,
                                       const uint8_t* block_data, const rpp_segment_candidate* candidates, uint32_t n,
                                       rpp_segment_match* matches) {
  if (!config_ok(cfg)) return RPP_UNSUPPORTED_CONFIG;
  if (n == 0) return RPP_OK;
  if (!extent_data || !block_data || !candidates || !matches) return RPP_INVALID_ARGUMENT;
  const Geometry G = geometry(cfg);
  for (uint32_t i = 0; i < n; ++i) {
    const rpp_segment_candidate& c = candidates[i];
    rpp_segment_match m{c.off, c.pos, 0};
    const bool ok = (uint64_t)c.off + G.W <= c.block_frames && (uint64_t)c.pos + G.W <= c.end && c.begin <= c.pos;
    const uint8_t* x = extent_data + c.extent_offset;
    const uint8_t* y = block_data + c.block_offset;
    const uint64_t g = G.g;
    if (ok && memcmp(x + c.pos * g, y + c.off * g, G.L) == 0) {
      uint64_t begin = c.begin, end = c.end;
      if (c.pos > c.off && c.pos - c.off > begin) begin = c.pos - c.off;
      if ((uint64_t)c.pos + c.block_frames - c.off < end) end = (uint64_t)c.pos + c.block_frames - c.off;
      uint64_t pre = 0, suf = 0;  // bytes
      while (pre < (c.pos - begin) * g && x[c.pos * g - pre - 1] == y[c.off * g - pre - 1]) ++pre;
      const uint64_t xs = (c.pos + (uint64_t)G.W) * g, ys = (c.off + (uint64_t)G.W) * g;
      while (suf < (end - c.pos - G.W) * g && x[xs + suf] == y[ys + suf]) ++suf;
      pre /= g;
      suf /= g;
      m.off = (uint32_t)(c.off - pre);
      m.pos = (uint32_t)(c.pos - pre);
      m.size = (uint32_t)(G.W + pre + suf);
    }
    matches[i] = m;
  }
  return RPP_OK;
}
