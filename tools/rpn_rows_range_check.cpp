// Stand-alone host check of the rows-form geometry of the RPN head backward (csrc/mx_rpn_rows.h): the
// grid of a rows-form dgrad sized by a list's capacity, and the block ranges the listed-rows activation
// pass finds in an ascending pixel list by binary search -- every listed row lands in exactly one
// block, in ascending order, and no index outside the list is ever read. Built with
// -fsanitize=address,undefined by tests/test_rpn_rows_range_host.py (or by hand):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I robust-object-detection_amd/csrc tools/rpn_rows_range_check.cpp -o rpn_rows_range_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "mx_rpn_rows.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static void check_grid() {
  const int64_t caps[] = {0, 1, 63, 64, 65, 127, 128, 129, 512, 4608, 12800, 134400, (1ll << 31) - 65};
  for (int64_t cap : caps)
    for (int64_t t : {64, 128}) {
      const int64_t g = mx::rpn_rows_grid(cap, t);
      CHECK(g * t >= cap && (g == 0 ? cap == 0 : (g - 1) * t < cap));
      // every row a launched block may own lies in [0, g * t): the kernel masks rows >= min(count, cap)
      CHECK(g <= (1ll << 25));
    }
  CHECK(mx::rpn_rows_grid(-5, 128) == 0 && mx::rpn_rows_grid(10, 0) == 0);
  CHECK(mx::rpn_rows_grid(12800, 128) == 100 && mx::rpn_rows_grid(4608, 128) == 36);
}

// the activation pass's partition: RB blocks of rows_per_block rows over M; block b visits
// [lower_bound(r0), lower_bound(r1)) of the exactly-sized list (ASan sees any read past it)
static void check_ranges(int64_t M, int64_t n, int64_t rows_per_block) {
  std::vector<int32_t> all((size_t)M);
  for (int64_t i = 0; i < M; ++i) all[(size_t)i] = (int32_t)i;
  for (int64_t i = 0; i < n; ++i) std::swap(all[(size_t)i], all[(size_t)(i + (int64_t)(rnd() % (uint64_t)(M - i)))]);
  std::vector<int32_t> rows(all.begin(), all.begin() + n);  // n distinct pixels, exact size
  std::sort(rows.begin(), rows.end());
  const int64_t RB = (M + rows_per_block - 1) / rows_per_block;
  int64_t seen = 0, prev_hi = 0;
  for (int64_t b = 0; b < RB; ++b) {
    const int64_t r0 = b * rows_per_block, r1 = std::min(M, r0 + rows_per_block);
    const int64_t lo = mx::rpn_rows_lower_bound(rows.data(), n, r0), hi = mx::rpn_rows_lower_bound(rows.data(), n, r1);
    CHECK(lo == prev_hi && lo <= hi && hi <= n);
    for (int64_t j = lo; j < hi; ++j) {
      CHECK(rows[(size_t)j] >= r0 && rows[(size_t)j] < r1);
      const int64_t lane = (rows[(size_t)j] - r0) & 31;  // the dense loop's row lane
      CHECK(lane == (rows[(size_t)j] - r0) % 32);
    }
    seen += hi - lo;
    prev_hi = hi;
  }
  CHECK(seen == n && prev_hi == n);
  CHECK(mx::rpn_rows_lower_bound(rows.data(), n, -1) == 0 && mx::rpn_rows_lower_bound(rows.data(), n, M) == n);
  CHECK(mx::rpn_rows_lower_bound(nullptr, 0, 5) == 0 && mx::rpn_rows_lower_bound(rows.data(), -3, 5) == 0);
}

int main() {
  check_grid();
  const int64_t Ms[] = {1, 31, 32, 33, 546, 4480, 50736, 134400};
  for (int64_t M : Ms)
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)6, (int64_t)129, (int64_t)512, M})
      for (int64_t rpb : {(int64_t)1, (int64_t)32, (int64_t)64, (M + 127) / 128, M})
        if (n <= M && rpb >= 1) check_ranges(M, n, rpb);
  puts("rpn_rows_range_check ok");
  return 0;
}
