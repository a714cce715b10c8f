// mx_rpn_sparse.hip — active-row lists of the RPN head's backward (gfx950).
//
// The gradient of a raw head map [N,H,W,C] (C = 5A, as mx_rpn_head_merge writes it) is exactly zero
// at every pixel none of whose anchors the sampler picked. Three kinds of launch turn it into ordered
// pixel lists without a sort and without atomics: a bitmap of the nonzero pixels (one ballot per
// wave), its 3x3 dilation (bitmap to bitmap, clipped to each image), and an ordered popcount scan of
// a bitmap by ONE block that writes the ascending flat pixel indices (n*H + h)*W + w.
// Every buffer is sized by a static capacity (mx_rpn_rows.h): a list that would overflow is cut at
// its capacity (nothing is written past it), its count still reports the true number of pixels and
// the sticky flag is set.
#include "mx_common.h"
#include "mx_rpn_rows.h"

namespace mx {

// bitmap[p >> 6] bit (p & 63) = any of the C values of pixel p has a nonzero bit pattern, sign ignored
__global__ void __launch_bounds__(256) rpn_rows_mark_kernel(const uint32_t* __restrict__ g, int64_t P, int C,
                                                             uint64_t* __restrict__ bitmap) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t any = 0;
  if (p < P) {
    const uint32_t* row = g + p * C;
    for (int c = 0; c < C; ++c) any |= row[c] & 0x7fffffffu;
  }
  const uint64_t word = __ballot(any != 0);
  // blocks are 4 whole waves: lanes 0..63 of a wave are pixels 64w .. 64w+63
  if ((threadIdx.x & 63) == 0 && p < P) bitmap[p >> 6] = word;
}

__device__ __forceinline__ uint32_t bit_at(const uint64_t* __restrict__ bm, int64_t q) {
  return (uint32_t)(bm[q >> 6] >> (q & 63)) & 1u;
}

// out = in dilated by the 3x3 neighbourhood inside each image (rows / columns do not wrap)
__global__ void __launch_bounds__(256) rpn_rows_dilate_kernel(const uint64_t* __restrict__ in, int64_t P, int H, int W,
                                                               uint64_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t any = 0;
  if (p < P) {
    const int w = (int)(p % W), h = (int)((p / W) % H);
#pragma unroll
    for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
      for (int dw = -1; dw <= 1; ++dw)
        if ((unsigned)(h + dh) < (unsigned)H && (unsigned)(w + dw) < (unsigned)W) any |= bit_at(in, p + dh * W + dw);
  }
  const uint64_t word = __ballot(any != 0);
  if ((threadIdx.x & 63) == 0 && p < P) out[p >> 6] = word;
}

// One block: rows[j] = index of the j-th set bit (ascending) for j < cap; *count = number of set bits
// (also past cap); *flag = 1 when that exceeds cap (never cleared here: sticky).
// TILES: the entries are the 32-pixel groups (bitmap half-words) with any bit set, index p / 32.
static constexpr int COMPACT_T = 1024;
template <bool TILES>
__device__ __forceinline__ void rpn_rows_compact_body(const uint64_t* __restrict__ bitmap, int64_t nwords,
                                                      int32_t* __restrict__ rows, int64_t cap,
                                                      int32_t* __restrict__ count, int32_t* __restrict__ flag) {
  __shared__ int wsum[COMPACT_T / 64];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < nwords; base += COMPACT_T) {
    const int64_t wi = base + tid;
    uint64_t word = wi < nwords ? bitmap[wi] : 0ull;
    if constexpr (TILES) word = ((word & 0xffffffffull) ? 1ull : 0ull) | ((word >> 32) ? 2ull : 0ull);
    const int n = __popcll(word);
    // inclusive scan inside the wave, then over the 16 wave totals
    int incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    int total = 0;
    for (int w = 0; w < COMPACT_T / 64; ++w) total += wsum[w];
    int64_t j = (int64_t)before + incl - n;
    while (word && j < cap) {
      const int b = __ffsll((unsigned long long)word) - 1;
      rows[j++] = (int32_t)(wi * (TILES ? 2 : 64) + b);
      word &= word - 1;
    }
    __syncthreads();
    if (tid == 0) carry_s += total;
    __syncthreads();
  }
  if (tid == 0) {
    const int total = carry_s;
    *count = total;
    if (total > cap) *flag = 1;
  }
}

template <bool TILES>
__global__ void __launch_bounds__(COMPACT_T) rpn_rows_compact_kernel(const uint64_t* __restrict__ bitmap, int64_t nwords,
                                                                      int32_t* __restrict__ rows, int64_t cap,
                                                                      int32_t* __restrict__ count,
                                                                      int32_t* __restrict__ flag) {
  rpn_rows_compact_body<TILES>(bitmap, nwords, rows, cap, count, flag);
}

// Both forms of one bitmap in one launch: block 0 the pixel list, block 1 (when launched) the K-step list.
__global__ void __launch_bounds__(COMPACT_T) rpn_rows_compact_both_kernel(const uint64_t* __restrict__ bitmap, int64_t nwords,
                                                                           int32_t* __restrict__ rows, int64_t cap,
                                                                           int32_t* __restrict__ count,
                                                                           int32_t* __restrict__ tiles, int64_t tcap,
                                                                           int32_t* __restrict__ tcount,
                                                                           int32_t* __restrict__ flag) {
  if (blockIdx.x == 0) rpn_rows_compact_body<false>(bitmap, nwords, rows, cap, count, flag);
  else rpn_rows_compact_body<true>(bitmap, nwords, tiles, tcap, tcount, flag);
}

}  // namespace mx

using namespace mx;

extern "C" int64_t mx_rpn_rows_capacity(int64_t P, int64_t NB, int level) { return rpn_rows_capacity(P, NB, level); }

extern "C" size_t mx_rpn_rows_workspace(int64_t P) { return P > 0 ? rpn_rows_workspace(P) : 0; }

template <bool TILES>
static int rows_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int levels, int32_t* rows0,
                                 int64_t cap0, int32_t* rows1, int64_t cap1, int32_t* rows2, int64_t cap2,
                                 int32_t* counts, int32_t* flag, void* ws, size_t ws_bytes, mx_stream_t stream) {
  MX_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1 && C < (1 << 16), "rpn rows: bad sizes");
  MX_CHECK_ARG(H < (1 << 20) && W < (1 << 20) && N * H * W < (1ll << 31) - 64,
               "rpn rows: map too large for 32-bit pixel indices");
  MX_CHECK_ARG(levels >= 1 && levels <= RPN_ROWS_LEVELS, "rpn rows: 1..3 lists");
  MX_CHECK_ARG(g && counts && flag && ws, "rpn rows: null argument");
  const int64_t P = N * H * W;
  MX_CHECK_ARG(ws_bytes >= rpn_rows_workspace(P), "rpn rows: workspace of %zu bytes required", rpn_rows_workspace(P));
  int32_t* const rows[RPN_ROWS_LEVELS] = {rows0, rows1, rows2};
  const int64_t caps[RPN_ROWS_LEVELS] = {cap0, cap1, cap2};
  for (int l = 0; l < levels; ++l)
    MX_CHECK_ARG(rows[l] && caps[l] >= 0 && caps[l] <= (TILES ? rpn_tiles_total(P) : P),
                 "rpn rows: list %d needs a buffer and a capacity in [0, entries of the map]", l);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nwords = rpn_rows_words(P);
  uint64_t* bm[2] = {(uint64_t*)ws, (uint64_t*)((char*)ws + rpn_rows_workspace(P) / 2)};
  const unsigned blocks = (unsigned)cdiv(P, 256);
  rpn_rows_mark_kernel<<<blocks, 256, 0, st>>>((const uint32_t*)(const void*)g, P, (int)C, bm[0]);
  MX_LAUNCH_CHECK();
  for (int l = 0; l < levels; ++l) {
    if (l > 0) {
      rpn_rows_dilate_kernel<<<blocks, 256, 0, st>>>(bm[(l - 1) & 1], P, (int)H, (int)W, bm[l & 1]);
      MX_LAUNCH_CHECK();
    }
    rpn_rows_compact_kernel<TILES><<<1, COMPACT_T, 0, st>>>(bm[l & 1], nwords, rows[l], caps[l], counts + l, flag);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

extern "C" int mx_rpn_rows_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int levels, int32_t* rows0,
                                 int64_t cap0, int32_t* rows1, int64_t cap1, int32_t* rows2, int64_t cap2,
                                 int32_t* counts, int32_t* flag, void* ws, size_t ws_bytes, mx_stream_t stream) {
  return rows_build<false>(g, N, H, W, C, levels, rows0, cap0, rows1, cap1, rows2, cap2, counts, flag, ws, ws_bytes, stream);
}

extern "C" int64_t mx_rpn_tiles_capacity(int64_t P, int64_t NB, int level) { return rpn_tiles_capacity(P, NB, level); }

extern "C" int mx_rpn_tiles_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int levels, int32_t* tiles0,
                                  int64_t cap0, int32_t* tiles1, int64_t cap1, int32_t* tiles2, int64_t cap2,
                                  int32_t* counts, int32_t* flag, void* ws, size_t ws_bytes, mx_stream_t stream) {
  return rows_build<true>(g, N, H, W, C, levels, tiles0, cap0, tiles1, cap1, tiles2, cap2, counts, flag, ws, ws_bytes,
                          stream);
}

// One mark, two dilations, and both forms compacted from the same three bitmaps: the pixel lists S0..S2
// (rows form of the dgrads and activation passes) and the K-step lists S0, S1 (tile-list wgrads).
extern "C" int mx_rpn_lists_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int32_t* rows0, int64_t cap0,
                                  int32_t* rows1, int64_t cap1, int32_t* rows2, int64_t cap2, int32_t* counts,
                                  int32_t* tiles0, int64_t tcap0, int32_t* tiles1, int64_t tcap1, int32_t* tcounts,
                                  int32_t* flag, void* ws, size_t ws_bytes, mx_stream_t stream) {
  MX_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1 && C < (1 << 16), "rpn lists: bad sizes");
  MX_CHECK_ARG(H < (1 << 20) && W < (1 << 20) && N * H * W < (1ll << 31) - 64,
               "rpn lists: map too large for 32-bit pixel indices");
  MX_CHECK_ARG(g && counts && tcounts && flag && ws, "rpn lists: null argument");
  const int64_t P = N * H * W;
  MX_CHECK_ARG(ws_bytes >= rpn_rows_workspace(P), "rpn lists: workspace of %zu bytes required", rpn_rows_workspace(P));
  int32_t* const rows[RPN_ROWS_LEVELS] = {rows0, rows1, rows2};
  const int64_t caps[RPN_ROWS_LEVELS] = {cap0, cap1, cap2};
  int32_t* const tiles[2] = {tiles0, tiles1};
  const int64_t tcaps[2] = {tcap0, tcap1};
  for (int l = 0; l < RPN_ROWS_LEVELS; ++l)
    MX_CHECK_ARG(rows[l] && caps[l] >= 0 && caps[l] <= P, "rpn lists: pixel list %d needs a buffer and a capacity in [0, P]", l);
  for (int l = 0; l < 2; ++l)
    MX_CHECK_ARG(tiles[l] && tcaps[l] >= 0 && tcaps[l] <= rpn_tiles_total(P),
                 "rpn lists: K-step list %d needs a buffer and a capacity in [0, ceil(P / 32)]", l);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nwords = rpn_rows_words(P);
  uint64_t* bm[2] = {(uint64_t*)ws, (uint64_t*)((char*)ws + rpn_rows_workspace(P) / 2)};
  const unsigned blocks = (unsigned)cdiv(P, 256);
  rpn_rows_mark_kernel<<<blocks, 256, 0, st>>>((const uint32_t*)(const void*)g, P, (int)C, bm[0]);
  MX_LAUNCH_CHECK();
  for (int l = 0; l < RPN_ROWS_LEVELS; ++l) {
    if (l > 0) {
      rpn_rows_dilate_kernel<<<blocks, 256, 0, st>>>(bm[(l - 1) & 1], P, (int)H, (int)W, bm[l & 1]);
      MX_LAUNCH_CHECK();
    }
    const bool both = l < 2;
    rpn_rows_compact_both_kernel<<<both ? 2 : 1, COMPACT_T, 0, st>>>(bm[l & 1], nwords, rows[l], caps[l], counts + l,
                                                                     both ? tiles[l] : nullptr, both ? tcaps[l] : 0,
                                                                     both ? tcounts + l : nullptr, flag);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}
