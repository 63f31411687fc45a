// C++ test of the incompressible categorizer's host scan
// (dwarfs_amd/csrc/scan/incompressible_host.cpp), built by build_incompressible.sh
// with AddressSanitizer and UBSan into a program of its own: no GPU, no library,
// nothing loaded into another process.  It generates its inputs: extents of text,
// of random bytes, of both in turns, and empty ones, cut at several block sizes.
// Every array the scan reads or writes is a heap block of exactly its size, so a
// byte read or written outside them stops the program.  Checked: every piece's
// size against rpp_zstd_host_encode_search's for the piece alone, the verdict
// and the totals recomputed here, and the fragment rows against a run-length
// loop; without generate_fragments no row is written.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ricepp_amd.h"

static int failures = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    if (!(cond)) {                                                                             \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (run %d)\n", __FILE__, __LINE__, #cond, run); \
      ++failures;                                                                              \
    }                                                                                          \
  } while (0)

template <typename T>
struct Exact {  // a heap block of exactly n elements (n == 0: one byte that is never offered)
  T* p;
  explicit Exact(size_t n, int fill = 0) : p(static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1))) {
    if (n) std::memset(p, fill, n * sizeof(T));
  }
  ~Exact() { std::free(p); }
};

static uint32_t rng_state = 12345;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static void append(std::vector<uint8_t>& out, bool random, size_t n) {
  static const char text[] = "The archive grows by one more block while the scanner reads on. ";
  for (size_t i = 0; i < n; ++i) out.push_back(random ? uint8_t(rnd()) : uint8_t(text[i % (sizeof text - 1)]));
}

int main() {
  int run = 0;
  const uint64_t block_sizes[] = {256, 1000, 32768, 40000};
  const uint32_t words[][2] = {{0, 0}, {RPP_ZSTD_ENC_TABLES | RPP_ZSTD_ENC_REPEAT, 0}, {3, 8 | RPP_SEARCH_LAZY}};
  for (uint64_t bs : block_sizes)
    for (const auto& w : words)
      for (uint32_t frag = 0; frag < 2; ++frag, ++run) {
        // extents: empty, text, random, mixed in turns of 3000 bytes, empty, one byte, a multiple of bs, empty
        std::vector<uint8_t> data;
        std::vector<uint64_t> ext;
        auto close = [&](size_t from) { ext.push_back(data.size() - from); };
        size_t at = 0;
        close(at);
        append(data, false, 5000);
        close(at), at = data.size();
        append(data, true, 4097);
        close(at), at = data.size();
        for (int k = 0; k < 14; ++k) append(data, k & 1, 3000);
        close(at), at = data.size();
        close(at);
        append(data, true, 1);
        close(at), at = data.size();
        append(data, false, size_t(2 * bs));
        close(at), at = data.size();
        close(at);
        std::vector<uint64_t> offs, lens;
        std::vector<uint32_t> base{0};
        uint64_t o = 0;
        for (uint64_t n : ext) {
          for (uint64_t q = 0; q < n; q += bs) {
            offs.push_back(o + q);
            lens.push_back(n - q < bs ? n - q : bs);
          }
          o += n;
          base.push_back(uint32_t(offs.size()));
        }
        const uint32_t np = uint32_t(offs.size()), ne = uint32_t(ext.size());
        Exact<uint8_t> in(data.size());
        std::memcpy(in.p, data.data(), data.size());
        Exact<uint64_t> d_off(np), d_len(np), sizes(np, 0xff), totals(size_t(ne) * RPP_INCOMPRESSIBLE_TOTALS, 0xff),
            rows(size_t(np) * 2, 0xff);
        Exact<uint32_t> d_base(ne + 1), verdicts(np, 0xff), count(ne, 0xff);
        Exact<int32_t> status(np, 0xff);
        std::memcpy(d_off.p, offs.data(), np * sizeof(uint64_t));
        std::memcpy(d_len.p, lens.data(), np * sizeof(uint64_t));
        std::memcpy(d_base.p, base.data(), (ne + 1) * sizeof(uint32_t));
        const double ratio = 0.99;
        CHECK(rpp_incompressible_host_scan(in.p, d_off.p, d_len.p, np, d_base.p, ne, ratio, frag, w[0], w[1], sizes.p,
                                           verdicts.p, totals.p, rows.p, count.p, status.p) == RPP_OK);
        for (uint32_t p = 0; p < np; ++p) {
          const uint64_t n = lens[p], cap = rpp_zstd_bound(n);
          Exact<uint8_t> piece{size_t(n)}, frame{size_t(cap)};
          std::memcpy(piece.p, data.data() + offs[p], size_t(n));
          uint64_t want = 0;
          CHECK(rpp_zstd_host_encode_search(piece.p, n, w[0], w[1], frame.p, cap, &want, nullptr) == RPP_OK);
          CHECK(status.p[p] == RPP_OK && sizes.p[p] == want);
          CHECK(verdicts.p[p] == (double(want) >= ratio * double(n) ? 1u : 0u));
        }
        for (uint32_t e = 0; e < ne; ++e) {
          uint64_t t[4] = {0, 0, 0, 0};
          std::vector<uint64_t> want;  // category, bytes, ...
          for (uint32_t p = base[e]; p < base[e + 1]; ++p) {
            t[0] += lens[p], t[1] += sizes.p[p], t[2] += 1, t[3] += verdicts.p[p];
            if (!want.empty() && want[want.size() - 2] == verdicts.p[p]) want.back() += lens[p];
            else want.push_back(verdicts.p[p]), want.push_back(lens[p]);
          }
          const uint64_t* got = totals.p + size_t(e) * RPP_INCOMPRESSIBLE_TOTALS;
          CHECK(std::memcmp(got, t, sizeof t) == 0 && t[0] == ext[e]);
          CHECK(got[4] == (t[2] > 0 && double(t[1]) >= ratio * double(t[0]) ? 1u : 0u));
          const uint32_t rows_want = frag ? uint32_t(want.size() / 2) : 0;
          CHECK(count.p[e] == rows_want);
          for (uint32_t r = 0; r < base[e + 1] - base[e]; ++r) {
            const uint64_t* row = rows.p + 2 * size_t(base[e] + r);
            if (r < rows_want) CHECK(row[0] == want[2 * r] && row[1] == want[2 * r + 1]);
            else CHECK(row[0] == ~UINT64_C(0) && row[1] == ~UINT64_C(0));  // not written
          }
        }
        // the mixed extent holds both verdicts once the pieces are small enough
        if (frag && bs <= 1000) CHECK(count.p[3] > 2);
        // argument rules
        CHECK(rpp_incompressible_host_scan(in.p, d_off.p, d_len.p, np, d_base.p, ne, ratio, frag, 4, 0, sizes.p,
                                           verdicts.p, totals.p, rows.p, count.p, status.p) == RPP_INVALID_ARGUMENT);
        CHECK(rpp_incompressible_host_scan(in.p, d_off.p, d_len.p, np, d_base.p, ne, ratio, frag, 0, 3, sizes.p,
                                           verdicts.p, totals.p, rows.p, count.p, status.p) == RPP_INVALID_ARGUMENT);
        CHECK(rpp_incompressible_host_scan(nullptr, nullptr, nullptr, 0, nullptr, 0, ratio, frag, 0, 0, nullptr, nullptr,
                                           nullptr, nullptr, nullptr, nullptr) == RPP_OK);
      }
  if (failures) {
    std::fprintf(stderr, "incompressible_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("incompressible_test: OK (%d runs)\n", run);
  return 0;
}
