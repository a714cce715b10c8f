// mx_corrupt_tile.h — the output tile and the store side of the batched corruption kernels
// (mx_corrupt.hip: noise / blur / low-res; mx_weather.hip: night / haze / rain). A workgroup of
// CB_THREADS lanes (4 waves) owns CB_ROWS x CB_COLS output pixels of one u8 [H][W][3] image.
#pragma once
#include "mx_common.h"

namespace mx {

static constexpr int CB_ROWS = 16, CB_COLS = 80, CB_THREADS = 256;
static_assert((CB_COLS * 3 + 3 + 3) / 4 <= 64, "one lane per aligned dword of a tile row");

// The store side, shared by every op: val(r, e) is output byte e (x * 3 + c within the tile row) of tile
// row r. Lane g of the wave that owns row r writes the aligned dword g of the row's span.
template <typename Val>
__device__ __forceinline__ void cb_store_tile(uint8_t* dst, int W, int y0, int x0, int rows, int cols, Val val) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = cols * 3;
  for (int r = wave; r < rows; r += CB_THREADS / 64) {
    uint8_t* rowp = dst + ((int64_t)(y0 + r) * W + x0) * 3;
    const int mis = (int)((uintptr_t)rowp & 3);
    const int start = lane * 4 - mis;  // first byte of this lane's dword, relative to the row
    if (start >= len) continue;
    // the four values are computed once, on one path for the whole wave (a row's partial first or last
    // dword would otherwise send its wave through the arithmetic twice); a byte outside the row stands
    // in for its nearest neighbour inside, which this lane owns, and is not stored
    uint8_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = start + j;
      v[j] = val(r, e < 0 ? 0 : (e >= len ? len - 1 : e));
    }
    if (start >= 0 && start + 4 <= len) {
      *(uint32_t*)(rowp + start) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = start + j;
        if (e >= 0 && e < len) rowp[e] = v[j];
      }
    }
  }
}

}  // namespace mx
