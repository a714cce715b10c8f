// mx_rpn_rows.h — host-side geometry of the row-sparse RPN-head backward (no HIP types: also built
// into the stand-alone sanitizer check tools/rpn_rows_geo_check.cpp).
//
// The RPN loss gives a gradient to at most B sampled anchors per image, so at most N*B pixels of a
// raw head map [N,H,W,5A] carry one (S0); a 3x3 conv's dgrad spreads them to the 3x3 neighbourhood
// (S1, at most 9x as many) and a second one to the 5x5 neighbourhood (S2, 25x). The lists live inside
// captured graphs, so every buffer is sized by these static capacities.
#pragma once
#include <stdint.h>

namespace mx {

static constexpr int RPN_ROWS_LEVELS = 3;

// capacity of list S<level> on a map of P = N*H*W pixels with NB = N * batch_size_per_image
inline int64_t rpn_rows_capacity(int64_t P, int64_t NB, int level) {
  if (P < 0 || NB < 0 || level < 0 || level >= RPN_ROWS_LEVELS) return -1;
  const int64_t spread = level == 0 ? 1 : (level == 1 ? 9 : 25);
  // NB * 25 cannot overflow for any NB a pixel index (< 2^31) can reach
  const int64_t nb = NB < P ? NB : P;
  const int64_t c = nb * spread;
  return c < P ? c : P;
}

// 64-bit bitmap words of a P-pixel map
inline int64_t rpn_rows_words(int64_t P) { return (P + 63) / 64; }

// bytes of the list builder's scratch: two ping-pong bitmaps (each 256-B aligned)
inline size_t rpn_rows_workspace(int64_t P) {
  const size_t w = (size_t)((rpn_rows_words(P) * 8 + 255) / 256 * 256);
  return 2 * w;
}

// K-step lists of the tile-list wgrad: the ascending indices p / 32 of the 32-pixel K-steps (aligned
// groups of 32 consecutive flat pixels, the x3 wgrad kernel's MFMA K-step) that hold a listed pixel.
// A listed pixel's 3x3 (5x5) neighbourhood is 3 (5) runs of consecutive flat indices, one per map
// row, and a run of at most 32 indices touches at most 2 groups.
static constexpr int RPN_TILE_PX = 32;
inline int64_t rpn_tiles_total(int64_t P) { return (P + RPN_TILE_PX - 1) / RPN_TILE_PX; }
inline int64_t rpn_tiles_capacity(int64_t P, int64_t NB, int level) {
  if (P < 0 || NB < 0 || level < 0 || level >= RPN_ROWS_LEVELS) return -1;
  const int64_t spread = level == 0 ? 1 : (level == 1 ? 6 : 10);
  const int64_t T = rpn_tiles_total(P);
  const int64_t nb = NB < T ? NB : T;
  const int64_t c = nb * spread;
  return c < T ? c : T;
}

// Row tiles of a rows-form dgrad launch: the grid is sized by the list's static capacity (the launch
// lives in captured graphs); blocks past the device count exit at once.
inline int64_t rpn_rows_grid(int64_t cap, int64_t tile_rows) {
  if (cap <= 0 || tile_rows <= 0) return 0;
  return (cap + tile_rows - 1) / tile_rows;
}

#if defined(__HIPCC__)
#define MX_ROWS_HD __host__ __device__
#else
#define MX_ROWS_HD
#endif

// First index j in [0, n) of the ascending list with rows[j] >= v (n when there is none): the
// listed-rows activation pass finds a block's range [lower_bound(r0), lower_bound(r1)) with it.
MX_ROWS_HD inline int64_t rpn_rows_lower_bound(const int32_t* rows, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n > 0 ? n : 0;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)rows[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace mx
