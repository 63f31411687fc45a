#!/bin/bash
# Host-only sanitizer build of the named digests' host definition: digest_host.cpp (names, sizes and rpp_digest_host
# on the round functions of digest_common.h) and digest_test.cpp (which has the main), with AddressSanitizer +
# UndefinedBehaviorSanitizer.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
g++ -std=c++20 $SAN -Wall -Wextra -Iinclude dwarfs_amd/csrc/digest/digest_host.cpp tests/cpp/digest_test.cpp \
  -o tests/cpp/build/digest_test
