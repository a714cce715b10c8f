// mx_gate.hip — degradation statistics of a whole batch of u8 images in one launch, and the verdict of a
// rule list over them, for the blind restoration gate (gfx950). The launch scheme of mx_corrupt.hip and
// mx_weather.hip: one workgroup per tile of one image, descriptors and rules as the kernel argument in
// chunks of 16 images; no workspace, no upload, no allocation, no host synchronisation.
//   The sums run over the interior pixels (rows 1..H-2, columns 1..W-2), so the tiles cover the interior
//   and a tile's one-pixel halo always lies inside the image: no border rule.
//   stage 1: the byte rows of the tile and its halo go to LDS as aligned 16-B vectors (a row starts at any
//     byte: 3 * W is no multiple of 4), bytes outside the image never read;
//   stage 2: luma Y = (77 R + 150 G + 29 B + 128) >> 8 of every staged pixel, one byte each, to LDS;
//   stage 3: a lane walks down one column of the tile with a sliding 3 x 3 window of luma and sums
//     |Immerkaer|, dx^2, dy^2, dxx^2, dyy^2 in u32 (GT_ROWS / 2 pixels per lane, 1024 per wave: see the
//     static_assert), waves reduce by shuffles, the workgroup through LDS in u64;
//   stage 4: one lane adds the five sums to stats[b][1..5] (64-bit agent-scope atomics: integer addition,
//     so the result does not depend on arrival order), then adds the tile's pixel count to stats[b][0]
//     (release / acquire). The workgroup that completes N = (H-2)(W-2) arrived last: it reads the totals
//     back, writes G2 = DX2 + DY2 and H2 = DXX2 + DYY2, evaluates the rules and writes the verdict.
//   stats is zeroed by one memset in front of the launches, so N doubles as the arrival counter and every
//   call starts from the same state.
// mx_restore_finish_gated lives here too: mx_restore_finish's arithmetic under a per-image verdict.
#include "mx_common.h"

namespace mx {

static constexpr int GT_ROWS = 32, GT_COLS = 128, GT_THREADS = 256;
static constexpr int GT_IMGS = 16;       // per chunk (kernel argument)
static constexpr int GT_MAX_RULES = 8;
static constexpr int GT_SROWS = GT_ROWS + 2, GT_SCOLS = GT_COLS + 2;  // staged: the tile and its halo
// 16-B vectors that cover a staged row's bytes wherever its first byte falls in a vector
static constexpr int GT_VECS = (GT_SCOLS * 3 + 15 + 15) / 16;
static constexpr int GT_RAW_STRIDE = GT_VECS * 16;
static constexpr int GT_Y_STRIDE = (GT_SCOLS + 3) / 4 * 4;
static constexpr int GT_LANE_ROWS = GT_ROWS * GT_COLS / GT_THREADS;  // pixels per lane
static_assert(GT_COLS == 128 && GT_THREADS == 2 * GT_COLS && GT_ROWS % 2 == 0, "a lane owns half a column of the tile");
// |Immerkaer term| <= 2040 bounds every summand by 2040^2; a wave's u32 sums cover 64 * GT_LANE_ROWS pixels
static_assert(2040ull * 2040ull * 64ull * GT_LANE_ROWS < (1ull << 32), "u32 accumulators per wave");
static_assert(GT_SROWS * GT_RAW_STRIDE + GT_SROWS * GT_Y_STRIDE < 32768, "LDS budget");

struct GtImg {
  const uint8_t* src;
  unsigned long long* stats;  // this image's 8 sums
  int32_t* verdict;           // this image's verdict
  int32_t H, W, bgr;
  int32_t tile0;              // first workgroup of this image
  int32_t tiles_x;
};
struct GtChunk {
  GtImg im[GT_IMGS];
  mx_gate_rule rules[GT_MAX_RULES];
  int32_t n, nrules, default_verdict;
};
static_assert(sizeof(GtChunk) <= 3072, "the chunk travels as a kernel argument");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(GT_THREADS) gate_stats_kernel(GtChunk ck) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[GT_SROWS * GT_RAW_STRIDE];
  __shared__ __attribute__((aligned(4))) uint8_t lum[GT_SROWS * GT_Y_STRIDE];
  __shared__ unsigned long long part[GT_THREADS / 64][5];
  __shared__ unsigned long long tot[8];
  int b = 0;
  while (b + 1 < ck.n && (int)blockIdx.x >= ck.im[b + 1].tile0) ++b;
  const GtImg& m = ck.im[b];
  const int H = m.H, W = m.W;
  const int t = (int)blockIdx.x - m.tile0;
  const int ty = t / m.tiles_x, tx = t - ty * m.tiles_x;
  const int y0 = 1 + ty * GT_ROWS, x0 = 1 + tx * GT_COLS;  // first interior pixel of the tile
  const int rows = min(GT_ROWS, H - 1 - y0), cols = min(GT_COLS, W - 1 - x0);
  const int srows = rows + 2, scols = cols + 2, len = scols * 3;
  const int tid = threadIdx.x;
  const uintptr_t img = (uintptr_t)m.src, end = img + (uintptr_t)H * W * 3;

  // stage 1: image rows y0 - 1 .. y0 + rows, the bytes of columns x0 - 1 .. x0 + cols
  for (int i = tid; i < srows * GT_VECS; i += GT_THREADS) {
    const int r = i / GT_VECS, v = i - r * GT_VECS;
    const uintptr_t rowp = img + ((uintptr_t)(y0 - 1 + r) * W + (x0 - 1)) * 3;
    const uintptr_t p = (rowp & ~(uintptr_t)15) + (uintptr_t)v * 16;
    if (p >= rowp + len) continue;  // past the row's last byte
    uint4 q;
    if (p >= img && p + 16 <= end) {
      q = *(const uint4*)p;
    } else {  // the image's first or last vector: only its own bytes are read
      uint8_t* qb = (uint8_t*)&q;
#pragma unroll
      for (int j = 0; j < 16; ++j) qb[j] = (p + j >= img && p + j < end) ? *(const uint8_t*)(p + j) : (uint8_t)0;
    }
    *(uint4*)(raw + r * GT_RAW_STRIDE + v * 16) = q;
  }
  __syncthreads();

  // stage 2: luma of every staged pixel
  const int ir = m.bgr ? 2 : 0;
  for (int i = tid; i < srows * scols; i += GT_THREADS) {
    const int r = i / scols, x = i - r * scols;
    const uintptr_t rowp = img + ((uintptr_t)(y0 - 1 + r) * W + (x0 - 1)) * 3;
    const uint8_t* px = raw + r * GT_RAW_STRIDE + (int)(rowp & 15) + 3 * x;
    const uint32_t R = px[ir], G = px[1], B = px[2 - ir];
    lum[r * GT_Y_STRIDE + x] = (uint8_t)((77u * R + 150u * G + 29u * B + 128u) >> 8);
  }
  __syncthreads();

  // stage 3: lane (c, g) sums rows g * GT_LANE_ROWS .. of tile column c
  uint32_t imm = 0, dx2 = 0, dy2 = 0, dxx2 = 0, dyy2 = 0;
  {
    const int c = tid & (GT_COLS - 1), g = tid >> 7;
    const int r0 = g * GT_LANE_ROWS, r1 = min(r0 + GT_LANE_ROWS, rows);
    if (c < cols && r0 < r1) {
      const uint8_t* L = lum + r0 * GT_Y_STRIDE + c;  // staged row r0 is the row above tile row r0
      int a0 = L[0], a1 = L[1], a2 = L[2];
      int b0 = L[GT_Y_STRIDE], b1 = L[GT_Y_STRIDE + 1], b2 = L[GT_Y_STRIDE + 2];
      for (int r = r0; r < r1; ++r) {
        const uint8_t* D = lum + (r + 2) * GT_Y_STRIDE + c;
        const int c0 = D[0], c1 = D[1], c2 = D[2];
        const int e = a0 + a2 + c0 + c2 - 2 * (a1 + c1 + b0 + b2) + 4 * b1;
        const int dx = b2 - b0, dy = c1 - a1, dxx = b2 - 2 * b1 + b0, dyy = c1 - 2 * b1 + a1;
        imm += (uint32_t)(e < 0 ? -e : e);
        dx2 += (uint32_t)(dx * dx);
        dy2 += (uint32_t)(dy * dy);
        dxx2 += (uint32_t)(dxx * dxx);
        dyy2 += (uint32_t)(dyy * dyy);
        a0 = b0; a1 = b1; a2 = b2;
        b0 = c0; b1 = c1; b2 = c2;
      }
    }
  }
  imm = wave_sum(imm);
  dx2 = wave_sum(dx2);
  dy2 = wave_sum(dy2);
  dxx2 = wave_sum(dxx2);
  dyy2 = wave_sum(dyy2);
  if ((tid & 63) == 0) {
    unsigned long long* pw = part[tid >> 6];
    pw[0] = imm; pw[1] = dx2; pw[2] = dy2; pw[3] = dxx2; pw[4] = dyy2;
  }
  __syncthreads();

  // stage 4: one lane per workgroup
  if (tid == 0) {
    unsigned long long* st = m.stats;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      unsigned long long s = 0;
#pragma unroll
      for (int w = 0; w < GT_THREADS / 64; ++w) s += part[w][k];
      __hip_atomic_fetch_add(st + 1 + k, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long cnt = (unsigned long long)rows * cols, N = (unsigned long long)(H - 2) * (W - 2);
    // the release orders this workgroup's five adds in front of its count; the acquire of the workgroup
    // that completes N orders every other workgroup's adds in front of the reads below
    const unsigned long long prev = __hip_atomic_fetch_add(st, cnt, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + cnt == N) {
      tot[0] = N;
#pragma unroll
      for (int k = 1; k <= 5; ++k) tot[k] = __hip_atomic_load(st + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tot[6] = tot[2] + tot[3];
      tot[7] = tot[4] + tot[5];
      st[6] = tot[6];
      st[7] = tot[7];
      int verdict = ck.default_verdict;
      for (int r = 0; r < ck.nrules; ++r) {
        const mx_gate_rule& u = ck.rules[r];
        // a, b < 2^16 and every sum < 2^47: the products fit
        if ((unsigned long long)u.a * tot[u.i] > (unsigned long long)u.b * tot[u.j]) {
          verdict = u.verdict;
          break;
        }
      }
      *m.verdict = verdict;
    }
  }
}

// mx_restore_finish's arithmetic (restore_finish_kernel, mx_unet.hip), statement by statement, for the
// images whose verdict is 1; the others keep the input's bytes
__global__ void restore_finish_gated_kernel(const uint8_t* __restrict__ img, int64_t B, int64_t Hp, int64_t Wp,
                                            const float* __restrict__ res, int64_t H, int64_t W,
                                            const int32_t* __restrict__ verdict, uint8_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * H * W * 3) return;
  int64_t c = i % 3, x = (i / 3) % W, y = (i / (3 * W)) % H, b = i / (3 * W * H);
  int64_t pi = ((b * Hp + y) * Wp + x) * 3 + c;
  if (verdict[b] == 0) {
    out[i] = img[pi];
    return;
  }
  float v = (float)img[pi] / 255.0f + res[pi];
  v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
  v = v * 255.0f;
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  out[i] = (uint8_t)v;
}

}  // namespace mx

using namespace mx;

extern "C" int mx_degradation_stats_tile(int32_t out[2]) {
  MX_CHECK_ARG(out != nullptr, "mx_degradation_stats_tile: null output");
  out[0] = GT_ROWS;
  out[1] = GT_COLS;
  return MX_OK;
}

extern "C" int mx_degradation_stats_u8(const mx_gate_desc* descs_host, int64_t n, const mx_gate_rule* rules_host,
                                       int32_t nrules, int32_t default_verdict, int64_t* stats, int32_t* verdict,
                                       mx_stream_t stream) {
  // everything is checked before the first launch
  MX_CHECK_ARG(n >= 0 && (n == 0 || descs_host), "mx_degradation_stats_u8: bad descriptor array");
  MX_CHECK_ARG(n == 0 || (stats && verdict), "mx_degradation_stats_u8: null stats or verdict output");
  MX_CHECK_ARG(nrules >= 0 && nrules <= GT_MAX_RULES, "mx_degradation_stats_u8: %d rules, at most %d", nrules, GT_MAX_RULES);
  MX_CHECK_ARG(nrules == 0 || rules_host, "mx_degradation_stats_u8: null rule array");
  MX_CHECK_ARG(default_verdict == 0 || default_verdict == 1, "mx_degradation_stats_u8: default verdict %d is not 0 or 1",
               default_verdict);
  for (int32_t r = 0; r < nrules; ++r) {
    const mx_gate_rule& u = rules_host[r];
    MX_CHECK_ARG(u.i >= 0 && u.i < 8 && u.j >= 0 && u.j < 8, "mx_degradation_stats_u8: rule %d: sum index outside 0..7", r);
    MX_CHECK_ARG(u.a >= 0 && u.a <= 65535 && u.b >= 0 && u.b <= 65535,
                 "mx_degradation_stats_u8: rule %d: coefficient outside 0..65535", r);
    MX_CHECK_ARG(u.verdict == 0 || u.verdict == 1, "mx_degradation_stats_u8: rule %d: verdict %d is not 0 or 1", r, u.verdict);
  }
  for (int64_t b = 0; b < n; ++b) {
    const mx_gate_desc& d = descs_host[b];
    MX_CHECK_ARG(d.src != nullptr, "mx_degradation_stats_u8: image %lld: null image", (long long)b);
    MX_CHECK_ARG(d.H >= 3 && d.W >= 3 && (int64_t)d.H * d.W <= ((int64_t)1 << 24),
                 "mx_degradation_stats_u8: image %lld: bad size %d x %d (3 <= H, W and H * W <= 2^24)", (long long)b, d.H,
                 d.W);
  }
  if (n == 0) return MX_OK;

  hipStream_t s = (hipStream_t)stream;
  MX_HIP(hipMemsetAsync(stats, 0, (size_t)n * 8 * sizeof(int64_t), s));
  GtChunk ck{};
  ck.nrules = nrules;
  ck.default_verdict = default_verdict;
  for (int32_t r = 0; r < nrules; ++r) ck.rules[r] = rules_host[r];
  int64_t tiles = 0;
  auto flush = [&]() -> int {
    if (ck.n > 0 && tiles > 0) {
      gate_stats_kernel<<<(unsigned)tiles, GT_THREADS, 0, s>>>(ck);
      MX_LAUNCH_CHECK();
    }
    ck.n = 0;
    tiles = 0;
    return MX_OK;
  };
  for (int64_t b = 0; b < n; ++b) {
    const mx_gate_desc& d = descs_host[b];
    const int64_t tx = cdiv(d.W - 2, GT_COLS), tyn = cdiv(d.H - 2, GT_ROWS);
    if (ck.n == GT_IMGS) {
      const int rc = flush();
      if (rc) return rc;
    }
    GtImg& m = ck.im[ck.n];
    m.src = d.src;
    m.stats = (unsigned long long*)stats + b * 8;
    m.verdict = verdict + b;
    m.H = d.H; m.W = d.W; m.bgr = d.bgr != 0;
    m.tile0 = (int32_t)tiles;
    m.tiles_x = (int32_t)tx;
    tiles += tx * tyn;  // <= 16 images of <= 2^24 pixels: far below 2^31
    ++ck.n;
  }
  return flush();
}

extern "C" int mx_restore_finish_gated(const uint8_t* img_padded, int64_t B, int64_t Hp, int64_t Wp, const float* residual,
                                       int64_t H, int64_t W, const int32_t* verdict, uint8_t* out, mx_stream_t stream) {
  MX_CHECK_ARG(B >= 0 && H >= 0 && W >= 0 && Hp >= H && Wp >= W, "restore_finish_gated: bad sizes");
  int64_t n = B * H * W * 3;
  if (n == 0) return MX_OK;
  MX_CHECK_ARG(img_padded && residual && verdict && out, "restore_finish_gated: null pointer");
  restore_finish_gated_kernel<<<(unsigned)cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(img_padded, B, Hp, Wp, residual, H, W,
                                                                                        verdict, out);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
