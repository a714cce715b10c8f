#!/bin/bash
# Host-only AddressSanitizer + UBSan run of the parallel entropy decoder's host restatement
# (mx_jpeg.cpp mx_jpeg_decode_coefs_chunked over csrc/mx_jpeg_walk.h, the walk the kernels share): a
# stand-alone program reads the corpus of tests/jpeg_corpus.py from files of exactly their size, decodes
# every one at the minimum and the default subsequence size into a heap buffer of exactly coef_total
# int16 (one element past it is a sanitizer report) and checks status 0 and equality with
# mx_jpeg_decode_coefs; then every file again truncated at several points and with its scan damaged,
# where a clean run is asked and either a non-zero status or, again, the sequential decoder's result.
# CPU only, nothing is loaded into Python.
# Usage: tools/jpeg_decode_asan.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
cat > $out/drv.cpp <<'CPP'
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mx_det.h"
namespace mx { void set_error(const char* fmt, ...) { (void)fmt; } }
static uint8_t* exact(const std::vector<uint8_t>& d, size_t n) {  // a heap copy of exactly n bytes
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  memcpy(p, d.data(), n);
  return p;
}
// status 0 promises the sequential decoder's coefficients, damaged stream or not
static bool agrees(const uint8_t* file, int64_t n, const mx_jpeg_info* info, const int16_t* got) {
  std::vector<int16_t> ref((size_t)info->coef_total);
  return mx_jpeg_decode_coefs(file, n, info, ref.data()) == 0 &&
         memcmp(got, ref.data(), sizeof(int16_t) * ref.size()) == 0;
}
int main(int argc, char** argv) {
  int same = 0, differ = 0, flagged = 0, silent = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    std::vector<uint8_t> d;
    int c;
    while ((c = fgetc(f)) != EOF) d.push_back((uint8_t)c);
    fclose(f);
    mx_jpeg_info info;
    if (mx_jpeg_parse(d.data(), (int64_t)d.size(), &info) != 0) return 2;
    std::vector<int16_t> ref((size_t)info.coef_total);
    if (mx_jpeg_decode_coefs(d.data(), (int64_t)d.size(), &info, ref.data()) != 0) return 2;
    const size_t scan = d.size() - info.scan_off;
    for (int s : {64, 512, 100, 65536}) {
      int16_t* got = (int16_t*)malloc(sizeof(int16_t) * (size_t)info.coef_total);
      int32_t st = -1;
      uint8_t* file = exact(d, d.size());
      const int rc = mx_jpeg_decode_coefs_chunked(file, (int64_t)d.size(), &info, s, got, &st);
      (rc == 0 && st == 0 && memcmp(got, ref.data(), sizeof(int16_t) * ref.size()) == 0) ? ++same : ++differ;
      free(file);
      // cut inside the scan: the last MCUs are missing, whatever byte the cut falls on
      for (size_t cut : {scan / 2, scan / 3, scan - 3, (size_t)1, scan * 4 / 5 + 1}) {
        if (cut == 0 || cut + 2 >= scan) continue;
        file = exact(d, info.scan_off + cut);
        st = 0;
        if (mx_jpeg_decode_coefs_chunked(file, (int64_t)(info.scan_off + cut), &info, s, got, &st) != 0) ++differ;
        st ? ++flagged : ++silent;
        if (!st && !agrees(file, (int64_t)(info.scan_off + cut), &info, got)) ++differ;
        free(file);
      }
      // 64 one-bits, a stray marker and a run of zeros in the middle of the scan
      if (scan > 64) {
        const uint8_t ones[16] = {255, 0, 255, 0, 255, 0, 255, 0, 255, 0, 255, 0, 255, 0, 255, 0};
        const uint8_t mark[4] = {255, 0xD9, 255, 0xD0};
        for (int kind = 0; kind < 3; ++kind) {
          file = exact(d, d.size());
          uint8_t* mid = file + info.scan_off + scan / 2;
          if (kind == 0) memcpy(mid, ones, 16);
          if (kind == 1) memcpy(mid, mark, 4);
          if (kind == 2) memset(mid, 0, 24);
          st = 0;
          if (mx_jpeg_decode_coefs_chunked(file, (int64_t)d.size(), &info, s, got, &st) != 0) ++differ;
          st ? ++flagged : ++silent;
          if (!st && !agrees(file, (int64_t)d.size(), &info, got)) ++differ;
          free(file);
        }
      }
      free(got);
    }
  }
  printf("identical %d different %d; damaged: flagged %d, decoded without a flag %d\n", same, differ, flagged, silent);
  return differ ? 1 : 0;
}
CPP
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -std=c++17 -Iinclude \
    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
    robust-object-detection_amd/csrc/mx_jpeg.cpp $out/drv.cpp -o $out/drv
python3 - "$out" <<'PY'
import os, sys
root = os.getcwd()
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "robust-object-detection_amd"), root]
import jpeg_corpus as jc
for i in range(len(jc.SPECS)):
    open(f"{sys.argv[1]}/f{i:04d}.jpg", "wb").write(jc.jpeg_file(i))
PY
ASAN_OPTIONS=detect_leaks=0 $out/drv $out/f*.jpg
