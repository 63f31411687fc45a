// incompressible_host_impl.h -- the body of rpp_incompressible_host_scan over any
// frame-size function, so that the call with the `long` word
// (incompressible_long_host.cpp) restates nothing.  The definition is at the top
// of incompressible_host.cpp.  Plain C++.
#pragma once

#include <stdint.h>

#include <vector>

#include "../lz4_common.h"
#include "../zstd_enc_common.h"
#include "ricepp_amd.h"

namespace rpp_incompressible {

// encode(piece, n, frame, capacity, &size) is an encoder's host call with the words bound; a piece above max_block
// bytes has the status of an over-size piece.
template <class Encode>
int host_scan(const uint8_t* in, const uint64_t* in_offsets, const uint64_t* in_bytes, uint32_t npieces,
              const uint32_t* piece_base, uint32_t nextents, double max_ratio, uint32_t generate_fragments,
              uint64_t max_block, Encode encode, uint64_t* sizes, uint32_t* verdicts, uint64_t* totals,
              uint64_t* frag_rows, uint32_t* frag_count, int32_t* status) {
  if (npieces == 0) return RPP_OK;  // nothing is written, as in the batch call
  if (!in || !in_offsets || !in_bytes || !sizes || !verdicts || !frag_rows || !status ||
      (nextents && (!piece_base || !totals || !frag_count)))
    return RPP_INVALID_ARGUMENT;
  for (uint32_t e = 0; e < nextents; ++e)
    if (piece_base[e] > piece_base[e + 1] || piece_base[e + 1] > npieces) return RPP_INVALID_ARGUMENT;
  std::vector<uint8_t> frame;
  for (uint32_t p = 0; p < npieces; ++p) {
    const uint64_t n = in_bytes[p];
    sizes[p] = 0;
    verdicts[p] = 0;
    status[p] = n <= max_block ? RPP_OK : RPP_INVALID_ARGUMENT;
    if (status[p] != RPP_OK) continue;
    frame.resize(rpp_zstd_bound(n));
    const int st = encode(in + in_offsets[p], n, frame.data(), frame.size(), &sizes[p]);
    if (st != RPP_OK) return st;
    verdicts[p] = double(sizes[p]) >= max_ratio * double(n) ? 1u : 0u;
  }
  for (uint32_t e = 0; e < nextents; ++e) {
    uint64_t* const t = totals + uint64_t(e) * RPP_INCOMPRESSIBLE_TOTALS;
    t[0] = t[1] = t[2] = t[3] = 0;
    uint32_t count = 0;
    for (uint32_t p = piece_base[e]; p < piece_base[e + 1]; ++p) {
      t[0] += in_bytes[p];
      t[1] += sizes[p];
      t[2] += 1;
      t[3] += verdicts[p];
      if (!generate_fragments) continue;
      uint64_t* const row = frag_rows + 2 * uint64_t(piece_base[e] + count);
      if (count && row[-2] == verdicts[p]) {  // add_fragment: the last fragment grows
        row[-1] += in_bytes[p];
      } else {
        row[0] = verdicts[p];
        row[1] = in_bytes[p];
        ++count;
      }
    }
    t[4] = t[2] > 0 && double(t[1]) >= max_ratio * double(t[0]) ? 1 : 0;
    frag_count[e] = count;
  }
  return RPP_OK;
}

}  // namespace rpp_incompressible
