// mx_corrupt_ops.h — the per-element arithmetic of the corruption ops (scripts/augmentations.py:30-45),
// shared by the one-op-per-launch kernels of mx_elementwise.hip and the batched kernel of
// mx_corrupt.hip. Both files are built -ffp-contract=off, and both reach every value through these
// functions, so the two paths produce the same bits. The bodies take the source pixels through a
// caller-supplied fetch (global memory there, LDS here); everything that rounds is in this file.
#pragma once
#include "mx_common.h"

namespace mx {

// Philox4x32-10 counter RNG + Box-Muller: N(0, sigma) per element (the on-device replacement of
// np.random.normal, which cannot be matched bit for bit; parity tests pass the field explicitly).
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ float gauss(uint64_t seed, uint64_t idx) {
  uint4 r = philox(make_uint4((uint32_t)idx, (uint32_t)(idx >> 32), 0x5eedu, 0u), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  float u1 = ((float)(r.x >> 8) + 1.0f) * (1.0f / 16777217.0f);
  float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// apply_noise: clip(f32(img) + f32(noise), 0, 255).astype(uint8) (truncation). i is the element's flat
// index within its own image: the Philox counter, or the index into the explicit field; px() is its source value.
template <typename Px>
__device__ __forceinline__ uint8_t noise_px(Px px, const float* __restrict__ noise, float sigma, uint64_t seed, int64_t i) {
  float nz = noise ? noise[i] : sigma * gauss(seed, (uint64_t)i);
  float v = (float)px() + nz;
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (uint8_t)v;
}

__device__ __forceinline__ int64_t refl101(int64_t i, int64_t n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
  }
  return i;
}

// filter2D's per-element sum: sum_t coef_t * src in f32 from 0, taps in the given order, then
// saturate_cast<uchar> (round half to even). coef(k) is tap k's coefficient, px(k) the source value at
// tap k's offset from the element (the offsets and the border rule are the fetch's).
template <typename Coef, typename Px>
__device__ __forceinline__ uint8_t filter2d_px(int n, Coef coef, Px px) {
  float s = 0.f;
  for (int k = 0; k < n; ++k) s += coef(k) * (float)px(k);
  float r = rintf(s);
  r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
  return (uint8_t)r;
}

// INTER_AREA, exact x2: sum = the four source values of the element; vec = the element lies in the part
// of its row that ResizeAreaFastVec_SIMD_8u takes ((sum + 2) >> 2), else the scalar tail
// (saturate_cast<uchar>(sum * 0.25f), exact halves to even).
__device__ __forceinline__ uint8_t area_fast2_px(int sum, bool vec) {
  if (vec) return (uint8_t)((sum + 2) >> 2);
  const float r = rintf((float)sum * 0.25f);
  return (uint8_t)(r > 255.f ? 255.f : r);
}

// elements per destination row that ResizeAreaFastVec_SIMD_8u (scale 2, 128-bit vectors) handles:
// cn 1: 8 per step, cn 3: 48 per step, cn 4: 16 per step; other channel counts: none (scalar)
__host__ __device__ inline int64_t area_fast2_vec_elems(int64_t dw, int64_t C) {
  const int64_t w = dw * C;
  const int64_t step = C == 1 ? 8 : (C == 3 ? 48 : (C == 4 ? 16 : 0));
  return step ? (w / step) * step : 0;
}

// OpenCV computeResizeAreaTab for one destination index: up to 3 (src, alpha) entries
__device__ int area_entries(int64_t ssize, int64_t d, double scale, int64_t* si, float* al) {
  int k = 0;
  double fs1 = d * scale, fs2 = fs1 + scale;
  double cell = scale < (ssize - fs1) ? scale : (ssize - fs1);
  int64_t s1 = (int64_t)ceil(fs1), s2 = (int64_t)floor(fs2);
  if (s2 > ssize - 1) s2 = ssize - 1;
  if (s1 > s2) s1 = s2;
  if (s1 - fs1 > 1e-3) { si[k] = s1 - 1; al[k++] = (float)((s1 - fs1) / cell); }
  for (int64_t s = s1; s < s2 && k < 7; ++s) { si[k] = s; al[k++] = (float)(1.0 / cell); }
  if (fs2 - s2 > 1e-3 && k < 8) {
    double dd = fs2 - s2;
    if (dd > 1.) dd = 1.;
    if (dd > cell) dd = cell;
    si[k] = s2; al[k++] = (float)(dd / cell);
  }
  return k;
}

// INTER_AREA general path for one element: sat(sum_y beta_y * (sum_x alpha_x * S)) in f32, same order as
// OpenCV; (xs, xa, nx) and (ys, ya, ny) from area_entries, px(j, k) = the source value at (ys[j], xs[k])
template <typename Px>
__device__ __forceinline__ uint8_t area_px(int nx, const float* xa, int ny, const float* ya, Px px) {
  float sum = 0.f;
  for (int j = 0; j < ny; ++j) {
    float buf = 0.f;
    for (int k = 0; k < nx; ++k) buf = buf + (float)px(j, k) * xa[k];
    sum = j == 0 ? ya[j] * buf : sum + ya[j] * buf;
  }
  float r = rintf(sum);
  return (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

__device__ __forceinline__ void lin_coef(int64_t ssize, int64_t dsize, int64_t d, int64_t* s_out, int* a0, int* a1) {
  double scale = 1.0 / ((double)dsize / ssize);
  float f = (float)((d + 0.5) * scale - 0.5);
  int64_t s = (int64_t)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  *s_out = s;
  *a0 = (int)rintf((1.f - f) * 2048.f);
  *a1 = (int)rintf(f * 2048.f);
}

// INTER_LINEAR 8U for one element, 11-bit fixed point; vertical combine as OpenCV's SIMD path (see
// oracle): p00, p01 the two source values of the upper row, p10, p11 of the lower one
__device__ __forceinline__ uint8_t linear_px(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
  int S0 = p00 * a0 + p01 * a1;
  int S1 = p10 * a0 + p11 * a1;
  int v = ((((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16) + 2) >> 2;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace mx
