#!/bin/bash
# Host-only sanitizer build of the Zstandard host encoder with its `long` word: zstd_long_host.cpp with the frame
# writer (zstd_encode_host.cpp), the match search (lz4_host.cpp), the decoder (zstd_host.cpp) and zstd_long_test.cpp
# (which has the main), with AddressSanitizer + UndefinedBehaviorSanitizer.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
g++ -std=c++20 $SAN -Wall -Wextra -Iinclude -Idwarfs_amd/csrc dwarfs_amd/csrc/lz4_host.cpp dwarfs_amd/csrc/zstd_host.cpp \
  dwarfs_amd/csrc/zstd_encode_host.cpp dwarfs_amd/csrc/zstd_long_host.cpp tests/cpp/zstd_long_test.cpp \
  -o tests/cpp/build/zstd_long_test
