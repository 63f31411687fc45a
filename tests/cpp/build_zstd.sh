#!/bin/bash
# Host-only sanitizer build of the Zstandard host functions: zstd_host.cpp and zstd_test.cpp
# (which has the main) with AddressSanitizer + UndefinedBehaviorSanitizer.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
g++ -std=c++20 $SAN -Wall -Wextra -Iinclude -Idwarfs_amd/csrc dwarfs_amd/csrc/zstd_host.cpp tests/cpp/zstd_test.cpp \
  -o tests/cpp/build/zstd_test
