// Stand-alone host check of the row-sparse RPN backward's geometry (csrc/mx_rpn_rows.h): list
// capacities of the pixel lists and of the K-step lists of the tile-list wgrad, and the bitmap workspace,
// swept over map sizes up to the 32-bit pixel limit. Built with -fsanitize=address,undefined by
// tests/test_rpn_rows_geo_host.py (or by hand):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I robust-object-detection_amd/csrc tools/rpn_rows_geo_check.cpp -o rpn_rows_geo_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mx_rpn_rows.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// the list layout a caller carves (conv.RowLists.build): lists back to back, then the counts;
// walks it the way the compaction kernel may write it (j < cap) on a real buffer
static void walk_layout(int64_t P, int64_t NB) {
  int64_t caps[mx::RPN_ROWS_LEVELS], total = 0;
  for (int l = 0; l < mx::RPN_ROWS_LEVELS; ++l) {
    caps[l] = mx::rpn_rows_capacity(P, NB, l);
    CHECK(caps[l] >= 0 && caps[l] <= P);
    if (l) CHECK(caps[l] >= caps[l - 1]);
    total += caps[l];
  }
  if (total > (1 << 22)) return;  // layout arithmetic only for the big sweeps
  std::vector<int32_t> buf((size_t)total + 4, -1);
  int64_t o = 0;
  for (int l = 0; l < mx::RPN_ROWS_LEVELS; ++l) {
    for (int64_t j = 0; j < caps[l]; ++j) buf[(size_t)(o + j)] = (int32_t)j;  // the worst case: a full list
    o += caps[l];
  }
  for (int l = 0; l < mx::RPN_ROWS_LEVELS; ++l) buf[(size_t)(o + l)] = (int32_t)P;
  CHECK(buf[(size_t)total + 3] == -1);
  // bitmap scratch: two ping-pong bitmaps, every word of a P-pixel map inside its half
  const int64_t words = mx::rpn_rows_words(P);
  const size_t ws = mx::rpn_rows_workspace(P);
  CHECK(words * 64 >= P && (words - 1) * 64 < P);
  CHECK(ws % 2 == 0 && ws / 2 >= (size_t)words * 8 && (ws / 2) % 256 == 0);
  std::vector<uint64_t> bm(ws / 8, 0);
  for (int half = 0; half < 2; ++half)
    for (int64_t p = 0; p < P; p += 63) bm[(size_t)(half * (ws / 16) + (p >> 6))] |= 1ull << (p & 63);
}

// K-step lists: capacities inside the map's K-step count, monotone in the level, and large enough for
// what they must hold -- every 32-pixel group a pixel's (2l+1) x (2l+1) neighbourhood can touch,
// checked by brute force on small maps with the worst case of NB isolated pixels
static void check_tiles(int64_t P, int64_t NB) {
  const int64_t T = mx::rpn_tiles_total(P);
  CHECK(T * 32 >= P && (T - 1) * 32 < P);
  int64_t prev = 0;
  for (int l = 0; l < mx::RPN_ROWS_LEVELS; ++l) {
    const int64_t c = mx::rpn_tiles_capacity(P, NB, l);
    CHECK(c >= prev && c <= T);
    prev = c;
  }
}
static void brute_tiles(int H, int W) {
  const int N = 2;
  const int64_t P = (int64_t)N * H * W;
  for (int l = 0; l < mx::RPN_ROWS_LEVELS; ++l) {
    const int64_t cap1 = mx::rpn_tiles_capacity(P, 1, l);
    for (int64_t p = 0; p < P; ++p) {  // one listed pixel anywhere: its neighbourhood's groups fit cap(NB = 1)
      const int w = (int)(p % W), h = (int)((p / W) % H);
      std::vector<uint8_t> hit((size_t)mx::rpn_tiles_total(P), 0);
      int64_t n = 0;
      for (int dh = -l; dh <= l; ++dh)
        for (int dw = -l; dw <= l; ++dw)
          if (h + dh >= 0 && h + dh < H && w + dw >= 0 && w + dw < W) {
            const int64_t q = p + (int64_t)dh * W + dw;
            if (!hit[(size_t)(q / 32)]++) ++n;
          }
      CHECK(n <= cap1);
    }
  }
}

int main() {
  const int64_t Ps[] = {1, 63, 64, 65, 70, 546, 4480, 50736, 134400, (1ll << 23) - 65, (1ll << 31) - 65};
  const int64_t NBs[] = {0, 1, 6, 40, 512, 4096, 1ll << 20, (1ll << 31) - 1};
  for (int64_t P : Ps)
    for (int64_t NB : NBs) {
      walk_layout(P, NB);
      check_tiles(P, NB);
    }
  CHECK(mx::rpn_rows_capacity(10, 4, 3) == -1 && mx::rpn_rows_capacity(-1, 4, 0) == -1);
  // the headline maps: P2 (2 x 200 x 336) and the canvas (2 x 151 x 168) at B = 256
  CHECK(mx::rpn_rows_capacity(134400, 512, 0) == 512 && mx::rpn_rows_capacity(134400, 512, 1) == 4608);
  CHECK(mx::rpn_rows_capacity(50736, 512, 2) == 12800);
  CHECK(mx::rpn_tiles_capacity(134400, 512, 0) == 512 && mx::rpn_tiles_capacity(134400, 512, 1) == 3072);
  CHECK(mx::rpn_tiles_capacity(50736, 512, 2) == 1586 && mx::rpn_tiles_capacity(10, 4, 3) == -1);
  const int hw[][2] = {{1, 1}, {1, 40}, {5, 7}, {13, 21}, {3, 33}, {9, 64}, {40, 56}};
  for (auto& d : hw) brute_tiles(d[0], d[1]);
  puts("rpn_rows_geo_check ok");
  return 0;
}
