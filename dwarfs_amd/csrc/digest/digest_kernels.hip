// digest_kernels.hip -- file digests by name on MI355X: MD5, SHA-1, SHA-224 /
// 256 / 384 / 512, SHA-512/224, SHA3-224 / 256 / 384 / 512, BLAKE2b-512 and
// BLAKE2s-256 over batches of files (rpp_digest_batch of include/ricepp_amd.h):
// what `dwarfsck --checksum=ALGO` and `mkdwarfs --file-hash=ALGO` accept beyond
// the XXH3 hashes (dwarfs::checksum hands every other name to EVP_get_digestbyname,
// src/checksum.cpp:264-280).
//
// The shape of rpp_sha512_256_kernel (section/section_kernels.hip): one lane per
// file -- a Merkle-Damgard or sponge chain does not split inside a message --
// and, while the batch is small, one wave per file (file i -> wave i % W, lane
// i / W), so that few files run on many SIMDs instead of in the lanes of one.
// Whole blocks of a payload on a 16-byte boundary (SHA-3: 8-byte) are read by
// 16-byte loads; the padded tail, and every block of a payload that is not on
// such a boundary, is assembled byte by byte.  The message schedule, and the 25
// lanes of the Keccak state, are in registers: every index is a compile-time
// constant (digest_common.h, which the host definition shares).
//
// One kernel template per compression function: the MD5, SHA-1, SHA-256 and
// SHA-512 rounds (the IV and the truncation chosen by `algo`), Keccak-f[1600]
// by rate, BLAKE2 by word size.  Every shift and rotate has a compile-time
// constant amount.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "digest_common.h"
#include "ricepp_amd.h"

namespace {

using namespace rpp_digest;

constexpr uint32_t kLaneWavesMax = 4096;  // 256 CUs x 4 SIMDs x 4 waves

struct Job {
  const uint8_t* data;
  const uint64_t* offs;
  const uint64_t* sizes;
  const uint8_t* select;  // file b is skipped (not read, nothing written) where select[b] == 0
  uint8_t* out;
  uint32_t out_stride;  // = the digest's bytes
  int algo;
};

// message of (wave w of W, lane l), as lane_message / lane_waves of section_kernels.hip
__device__ inline uint64_t lane_message(uint32_t nwaves) {
  return (uint64_t)threadIdx.x * nwaves + blockIdx.x;
}
uint32_t lane_waves(uint32_t n) {
  const uint32_t full = (n + 63) / 64, spread = n < kLaneWavesMax ? n : kLaneWavesMax;
  return full > spread ? full : spread;
}

struct File {
  const uint8_t* p;
  uint64_t len;
  uint8_t* out;
};
__device__ inline bool load_file(const Job& j, uint32_t n, uint32_t nwaves, File& f) {
  const uint64_t id = lane_message(nwaves);
  if (id >= n) return false;
  if (j.select && !j.select[id]) return false;
  f.p = j.data + j.offs[id];
  f.len = j.sizes[id];
  f.out = j.out + (size_t)j.out_stride * id;
  return true;
}

template <class H>
__global__ __launch_bounds__(64) void rpp_digest_md_kernel(Job job, uint32_t n, uint32_t nwaves) {
  File f;
  if (load_file(job, n, nwaves, f)) md_digest<H>(f.p, f.len, job.algo, job.out_stride / 4, f.out);
}

template <int Rate>
__global__ __launch_bounds__(64) void rpp_digest_keccak_kernel(Job job, uint32_t n, uint32_t nwaves) {
  File f;
  if (load_file(job, n, nwaves, f)) keccak_digest<Rate>(f.p, f.len, job.out_stride / 4, f.out);
}

template <class W>
__global__ __launch_bounds__(64) void rpp_digest_blake2_kernel(Job job, uint32_t n, uint32_t nwaves) {
  File f;
  if (load_file(job, n, nwaves, f)) blake2_digest<W>(f.p, f.len, job.out_stride / 4, f.out);
}

template <class K>
int launch(K kernel, const Job& job, uint32_t n, hipStream_t s) {
  const uint32_t nw = lane_waves(n);
  hipLaunchKernelGGL(kernel, dim3(nw), dim3(64), 0, s, job, n, nw);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}

}  // namespace

extern "C" int rpp_digest_batch(int algo, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                const uint8_t* d_select, uint32_t n, uint8_t* d_digest, void* stream) {
  const int nbytes = rpp_digest_bytes(algo);
  if (nbytes == 0) return RPP_INVALID_ARGUMENT;
  if (n == 0) return RPP_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_digest) return RPP_INVALID_ARGUMENT;
  const Job job{d_data, d_offsets, d_sizes, d_select, d_digest, (uint32_t)nbytes, algo};
  hipStream_t s = (hipStream_t)stream;
  switch (algo) {
    case RPP_DIGEST_XXH3_64:
      return rpp_file_hash_batch(RPP_HASH_XXH3_64, d_data, d_offsets, d_sizes, d_select, n, d_digest, stream);
    case RPP_DIGEST_XXH3_128:
      return rpp_file_hash_batch(RPP_HASH_XXH3_128, d_data, d_offsets, d_sizes, d_select, n, d_digest, stream);
    case RPP_DIGEST_SHA512_256:
      return rpp_file_hash_batch(RPP_HASH_SHA512_256, d_data, d_offsets, d_sizes, d_select, n, d_digest, stream);
    case RPP_DIGEST_MD5: return launch(rpp_digest_md_kernel<Md5>, job, n, s);
    case RPP_DIGEST_SHA1: return launch(rpp_digest_md_kernel<Sha1>, job, n, s);
    case RPP_DIGEST_SHA224:
    case RPP_DIGEST_SHA256: return launch(rpp_digest_md_kernel<Sha256>, job, n, s);
    case RPP_DIGEST_SHA384:
    case RPP_DIGEST_SHA512:
    case RPP_DIGEST_SHA512_224: return launch(rpp_digest_md_kernel<Sha512>, job, n, s);
    case RPP_DIGEST_SHA3_224: return launch(rpp_digest_keccak_kernel<144>, job, n, s);
    case RPP_DIGEST_SHA3_256: return launch(rpp_digest_keccak_kernel<136>, job, n, s);
    case RPP_DIGEST_SHA3_384: return launch(rpp_digest_keccak_kernel<104>, job, n, s);
    case RPP_DIGEST_SHA3_512: return launch(rpp_digest_keccak_kernel<72>, job, n, s);
    case RPP_DIGEST_BLAKE2B512: return launch(rpp_digest_blake2_kernel<uint64_t>, job, n, s);
    case RPP_DIGEST_BLAKE2S256: return launch(rpp_digest_blake2_kernel<uint32_t>, job, n, s);
  }
  return RPP_INVALID_ARGUMENT;
}
