#!/bin/bash
# Builds the C++ segmenter test against the product library.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
hipcc -O2 -std=c++20 -Iinclude -o tests/cpp/build/segment_test tests/cpp/segment_test.cpp \
  -Ldwarfs_amd/lib -lricepp_amd -Wl,-rpath,'$ORIGIN/../../../dwarfs_amd/lib'
