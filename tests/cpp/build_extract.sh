#!/bin/bash
# Host-only sanitizer build of the file extraction's host gather: extract_host.cpp (the definition, with the chunk
# rules of extract_common.h) and extract_test.cpp (which has the main), with AddressSanitizer +
# UndefinedBehaviorSanitizer.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/cpp/build
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
g++ -std=c++20 $SAN -Wall -Wextra -Iinclude dwarfs_amd/csrc/extract/extract_host.cpp tests/cpp/extract_test.cpp \
  -o tests/cpp/build/extract_test
