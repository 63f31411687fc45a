#!/bin/bash
# Host-only sanitizer build of the incompressible categorizer's host scan: incompressible_host.cpp with the
# Zstandard host encoder (zstd_encode_host.cpp), the match search (lz4_host.cpp) and incompressible_test.cpp
# (which has the main), with AddressSanitizer + UndefinedBehaviorSanitizer.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
g++ -std=c++20 $SAN -Wall -Wextra -Iinclude -Idwarfs_amd/csrc dwarfs_amd/csrc/lz4_host.cpp \
  dwarfs_amd/csrc/zstd_encode_host.cpp dwarfs_amd/csrc/scan/incompressible_host.cpp tests/cpp/incompressible_test.cpp \
  -o tests/cpp/build/incompressible_test
