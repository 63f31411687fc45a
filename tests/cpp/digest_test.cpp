// digest_test.cpp -- the host definition of the named digests (rpp_digest_algo,
// rpp_digest_bytes, rpp_digest_host; dwarfs_amd/csrc/digest/digest_host.cpp) in
// a program of its own, built with AddressSanitizer and UBSan by build_digest.sh.
//
//   digest_test SWEEP_FILE
//
// It checks the published "abc" and empty-message vectors of each standard, the
// name rules, and every line `name length hexdigest` of SWEEP_FILE: the message
// is byte k = (31 k + length) & 0xFF, hashed at every misalignment 0..15 from a
// heap buffer that ends with the message's last byte, into a digest buffer of
// exactly the digest's size (so a read or write past either end is reported),
// with a select mask that skips a second file whose pointer must not be followed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ricepp_amd.h"

namespace {

int failures = 0;

void check(bool ok, const char* what, const std::string& detail = "") {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s %s\n", what, detail.c_str());
  }
}

std::string hex(const std::vector<uint8_t>& v) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint8_t b : v) {
    s += d[b >> 4];
    s += d[b & 15];
  }
  return s;
}

// the digest of `msg` placed `mis` bytes behind a 16-byte boundary, in exact-size buffers
std::string digest_at(int algo, const std::vector<uint8_t>& msg, size_t mis) {
  const size_t nbytes = (size_t)rpp_digest_bytes(algo);
  std::vector<uint8_t> exact(mis + msg.size() ? mis + msg.size() : 1);  // (never a null pointer)
  uint8_t* heap = static_cast<uint8_t*>(malloc(mis + msg.size() + 16));
  const size_t shift = (16 - (reinterpret_cast<uintptr_t>(heap) & 15)) & 15;
  // heap + shift is a 16-byte boundary; the message starts `mis` behind it and ends at most 15 bytes before the
  // block's end -- a second copy in `exact` ends exactly on its allocation's last byte
  uint8_t* at = heap + shift + mis;
  if (!msg.empty()) memcpy(at, msg.data(), msg.size());
  if (!msg.empty()) memcpy(exact.data() + mis, msg.data(), msg.size());
  std::vector<uint8_t> out(2 * nbytes, 0xA5), out2(nbytes, 0);
  const uint64_t offsets[2] = {0, UINT64_MAX / 2}, sizes[2] = {msg.size(), UINT64_MAX / 4};
  const uint8_t select[2] = {1, 0};  // (file 1 lies nowhere: it must not be read)
  check(rpp_digest_host(algo, at, offsets, sizes, select, 2, out.data()) == RPP_OK, "rpp_digest_host");
  for (size_t k = nbytes; k < 2 * nbytes; ++k) check(out[k] == 0xA5, "an unselected row was written");
  const uint64_t off2[1] = {mis}, size2[1] = {msg.size()};
  check(rpp_digest_host(algo, exact.data(), off2, size2, nullptr, 1, out2.data()) == RPP_OK, "rpp_digest_host (exact)");
  out.resize(nbytes);
  check(out == out2, "the same message at two addresses", hex(out) + " " + hex(out2));
  free(heap);
  return hex(out);
}

struct Published {
  const char *name, *abc, *empty;
};
const Published kPublished[] = {
    {"md5", "900150983cd24fb0d6963f7d28e17f72", "d41d8cd98f00b204e9800998ecf8427e"},
    {"sha1", "a9993e364706816aba3e25717850c26c9cd0d89d", "da39a3ee5e6b4b0d3255bfef95601890afd80709"},
    {"sha224", "23097d223405d8228642a477bda255b32aadbce4bda0b3f7e36c9da7",
     "d14a028c2a3a2bc9476102bb288234c415a2b01f828ea62ac5b3e42f"},
    {"sha256", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
     "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"},
    {"sha384", "cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed8086072ba1e7cc2358baeca134c825a7",
     "38b060a751ac96384cd9327eb1b1e36a21fdb71114be07434c0cc7bf63f6e1da274edebfe76f65fbd51ad2f14898b95b"},
    {"sha512",
     "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
     "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
     "cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce"
     "47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e"},
    {"sha512-224", "4634270f707b6a54daae7530460842e20e37ed265ceee9a43e8924aa",
     "6ed0dd02806fa89e25de060c19d3ac86cabb87d6a0ddd05c333b84f4"},
    {"sha3-224", "e642824c3f8cf24ad09234ee7d3c766fc9a3a5168d0c94ad73b46fdf",
     "6b4e03423667dbb73b6e15454f0eb1abd4597f9a1b078e3f5b5a6bc7"},
    {"sha3-256", "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532",
     "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"},
    {"sha3-384", "ec01498288516fc926459f58e2c6ad8df9b473cb0fc08c2596da7cf0e49be4b298d88cea927ac7f539f1edf228376d25",
     "0c63a75b845e4f7d01107d852e4c2485c51a50aaaa94fc61995e71bbee983a2ac3713831264adb47fb6bd1e058d5f004"},
    {"sha3-512",
     "b751850b1a57168a5693cd924b6b096e08f621827444f70d884f5d0240d2712e"
     "10e116e9192af3c91a7ec57647e3934057340b4cf408d5a56592f8274eec53f0",
     "a69f73cca23a9ac5c8b567dc185a756e97c982164fe25859e0d1dcc1475c80a6"
     "15b2123af1f5f94c11e3e9402c3ac558f500199d95b6d3e301758586281dcd26"},
    {"blake2b512",
     "ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1"
     "7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923",
     "786a02f742015903c6c6fd852552d272912f4740e15847618a86e217f71f5419"
     "d25e1031afee585313896444934eb04b903a685b1448b755d56f701afe9be2ce"},
    {"blake2s256", "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982",
     "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"},
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: digest_test SWEEP_FILE\n");
    return 2;
  }
  const std::vector<uint8_t> abc = {'a', 'b', 'c'};
  for (const Published& p : kPublished) {
    const int algo = rpp_digest_algo(p.name);
    check(algo >= 0 && rpp_digest_bytes(algo) * 2 == (int)strlen(p.abc), "name and size", p.name);
    for (size_t mis = 0; mis < 16; ++mis) {
      check(digest_at(algo, abc, mis) == p.abc, "published abc", p.name);
      check(digest_at(algo, {}, mis) == p.empty, "published empty message", p.name);
    }
  }
  check(rpp_digest_algo("SHA256") == rpp_digest_algo("sha256") && rpp_digest_algo("Sha3-512") >= 0, "letter case");
  check(rpp_digest_algo("XXH3-128") < 0 && rpp_digest_algo("xxh3-128") >= 0, "xxh3 names are exact");
  check(rpp_digest_algo("shake128") < 0 && rpp_digest_algo("") < 0 && rpp_digest_algo(nullptr) < 0, "unknown names");
  check(rpp_digest_bytes(-1) == 0 && rpp_digest_bytes(RPP_DIGEST_COUNT) == 0, "unknown values");
  check(rpp_digest_host(RPP_DIGEST_XXH3_128, abc.data(), nullptr, nullptr, nullptr, 0, nullptr) == RPP_INVALID_ARGUMENT,
        "xxh3 has no host form");
  check(rpp_digest_host(RPP_DIGEST_MD5, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == RPP_OK, "empty batch");
  check(rpp_digest_host(RPP_DIGEST_MD5, nullptr, nullptr, nullptr, nullptr, 1, nullptr) == RPP_INVALID_ARGUMENT,
        "null pointers with work to do");

  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  char name[64], want[160];
  unsigned long length;
  size_t lines = 0;
  while (fscanf(f, "%63s %lu %159s", name, &length, want) == 3) {
    const int algo = rpp_digest_algo(name);
    check(algo >= 0, "a name of the sweep file", name);
    if (algo < 0) continue;
    std::vector<uint8_t> msg(length);
    for (size_t k = 0; k < msg.size(); ++k) msg[k] = (uint8_t)((31 * k + length) & 0xFF);
    for (size_t mis = 0; mis < 16; ++mis)
      check(digest_at(algo, msg, mis) == want, "sweep", std::string(name) + " " + std::to_string(length));
    ++lines;
  }
  fclose(f);
  check(lines > 0, "the sweep file has lines");
  if (failures) {
    printf("digest_test: %d FAILED\n", failures);
    return 1;
  }
  printf("digest_test: OK (%zu sweep lines)\n", lines);
  return 0;
}
