#!/bin/bash
# Builds the C++ duplicate-file test against the product library.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
hipcc -O2 -std=c++20 -Iinclude -o tests/cpp/build/dedup_test tests/cpp/dedup_test.cpp \
  -Ldwarfs_amd/lib -lricepp_amd -Wl,-rpath,'$ORIGIN/../../../dwarfs_amd/lib'
