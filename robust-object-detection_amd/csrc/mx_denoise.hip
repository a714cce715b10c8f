// mx_denoise.hip — blind non-local means over a whole batch of u8 images in one launch (gfx950): the pixel
// branch behind the restoration gate's noise verdict. include/mx_det.h (mx_denoise_nlm_u8) defines the
// arithmetic; all of it is unsigned integers, so the numpy restatement (tests/denoise_ref.py) gives the same
// bytes. The launch scheme of mx_gate.hip and mx_corrupt.hip: one workgroup per output tile of one image,
// descriptors as the kernel argument in chunks of 16 images; no workspace, no upload, no allocation, no host
// synchronisation.
//   stage 0: every workgroup reads stats[b] (and verdict[b]) from device memory and derives s8, T0, Q and the
//     apply decision itself: the call is blind without a read-back. A tile of an image that is not denoised
//     copies its bytes and leaves. The lane that owns the image's first tile writes applied[b].
//   stage 1: the byte rows of the tile and its 7-pixel halo, clipped to the image, go to LDS as aligned 16-B
//     vectors (a row starts at any byte), bytes outside the image never read;
//   stage 2: every staged position takes the pixel at its clamped coordinates: luma, one byte each, with the
//     7-pixel halo; the three channels packed in a dword with the 5-pixel halo. Clamping is done here, on
//     indices, so the hot loop below only adds offsets. The dwords of a row lie in four planes by column & 3,
//     so that lanes four columns apart read neighbouring banks.
//   stage 3: a lane owns 4 neighbouring columns x NL_R rows. Its own 8 luma bytes per patch row stay in
//     registers. Per candidate offset it walks down NL_R + 4 patch rows: 8 squared differences per row give
//     the four 5-wide row sums by sliding (h1 = h0 - e0 + e5), a ring of the last five row sums gives the
//     5 x 5 distance by sliding down. So a candidate costs 8 (NL_R + 4) / (4 NL_R) = 4 squared differences
//     per pixel instead of 25. The distance goes through T0, Q and the table to the weight; weight and
//     weighted channels accumulate in u32 registers over the 121 candidates.
//   stage 4: out = (sum + (Wsum >> 1)) / Wsum per channel, stored for the pixels inside the image.
#include "mx_common.h"
#include "mx_nlm_lut.h"

namespace mx {

static constexpr int NL_P = 2, NL_S = 5;              // patch and search radius
static constexpr int NL_HY = NL_P + NL_S;             // luma halo
static constexpr int NL_HX = NL_S;                    // channel halo
static constexpr int NL_TR = 32, NL_TC = 64;          // output tile
static constexpr int NL_R = 4;                        // rows per lane; a lane owns 4 columns
static constexpr int NL_THREADS = (NL_TR / NL_R) * (NL_TC / 4);
static constexpr int NL_IMGS = 16;                    // per chunk (kernel argument)
static constexpr int NL_YR = NL_TR + 2 * NL_HY, NL_YC = NL_TC + 2 * NL_HY;  // staged luma
static constexpr int NL_XR = NL_TR + 2 * NL_HX, NL_XC = NL_TC + 2 * NL_HX;  // staged channels
// 16-B vectors that cover a staged row's bytes wherever its first byte falls in a vector
static constexpr int NL_VECS = (NL_YC * 3 + 15 + 15) / 16;
static constexpr int NL_RAW_STRIDE = NL_VECS * 16;
// luma: staged column s lies at byte s + NL_YSHIFT of its row, so that the 8 bytes a lane owns (tile columns
// 4 lc - 2 .. 4 lc + 5) are two aligned dwords. The row pitch is 28 dwords: the four row groups of a wave lie
// 4 rows = 112 dwords = 16 banks (mod 32) apart.
static constexpr int NL_YSHIFT = 3;
static constexpr int NL_LSTR = 112;
// channels: plane (column & 3) of NL_XPL dwords, row pitch 84 dwords (4 rows = 16 banks mod 32)
static constexpr int NL_XPL = 20, NL_XSTR = 4 * NL_XPL + 4;
static_assert(NL_THREADS == 128 && NL_TC % 4 == 0 && NL_TR % NL_R == 0, "a lane owns 4 columns x NL_R rows");
static_assert((NL_HY - NL_P + NL_YSHIFT) % 4 == 0, "a lane's own luma bytes are aligned dwords");
// the candidate's 8 bytes start at byte 4 lc + 8 + dx of the row, |dx| <= 5: three dwords from dword
// lc + ((8 + dx) >> 2) cover them and stay inside the row
static_assert(NL_HY - NL_P + NL_YSHIFT - NL_S >= 0, "the candidate's first dword lies in the row");
static_assert((NL_TC / 4 - 1) + ((NL_HY - NL_P + NL_YSHIFT + NL_S) >> 2) + 2 < NL_LSTR / 4, "and its last");
static_assert(NL_YC + NL_YSHIFT <= NL_LSTR && (NL_XC + 3) / 4 <= NL_XPL, "row pitches");
static_assert(NL_YR * NL_RAW_STRIDE + NL_YR * NL_LSTR + NL_XR * NL_XSTR * 4 + (MX_NLM_LUT_SIZE + 1) * 4 < 49152, "LDS budget");
// the bounds of the definition (include/mx_det.h)
static_assert(25 * 255 * 255 < (1 << 21), "d < 2^21");
static_assert((1ull << 21) * (1ull << 24) <= (1ull << 45), "t * Q < 2^45: 64 bits by the definition");
static_assert((1ull << 27) + (1ull << 24) < (1ull << 32), "min(t, ceil(2^27 / Q)) * Q fits 32 bits (stage 0)");
static_assert(121ull * 4096ull * 255ull < (1ull << 27), "sum w * X < 2^27: u32 accumulators");
static_assert(121ull * 4096ull < (1ull << 19), "Wsum < 2^19");

__constant__ int32_t nlm_lut_dev[MX_NLM_LUT_SIZE] = {MX_NLM_LUT_VALUES};
static const int32_t nlm_lut_host[MX_NLM_LUT_SIZE] = {MX_NLM_LUT_VALUES};

struct NlImg {
  const uint8_t* src;
  uint8_t* dst;
  const unsigned long long* stats;  // this image's 8 sums, or null (explicit sigma)
  const int32_t* verdict;           // this image's verdict, or null
  int32_t* applied;                 // this image's flag, or null
  int32_t H, W, bgr, sigma_q8;
  int32_t tile0;                    // first workgroup of this image
  int32_t tiles_x;
};
struct NlChunk {
  NlImg im[NL_IMGS];
  int32_t n, rule_a, rule_b, k16;
};
static_assert(sizeof(NlChunk) <= 3072, "the chunk travels as a kernel argument");

__global__ void __launch_bounds__(NL_THREADS) nlm_kernel(NlChunk ck) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[NL_YR * NL_RAW_STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t lum[NL_YR * NL_LSTR];
  __shared__ uint32_t rgb[NL_XR * NL_XSTR];
  __shared__ uint32_t lut[MX_NLM_LUT_SIZE + 1];
  int b = 0;
  while (b + 1 < ck.n && (int)blockIdx.x >= ck.im[b + 1].tile0) ++b;
  const NlImg& m = ck.im[b];
  const int H = m.H, W = m.W;
  const int t = (int)blockIdx.x - m.tile0;
  const int ty = t / m.tiles_x, tx = t - ty * m.tiles_x;
  const int y0 = ty * NL_TR, x0 = tx * NL_TC;
  const int rows = min(NL_TR, H - y0), cols = min(NL_TC, W - x0);
  const int tid = threadIdx.x;

  // stage 0: the image's parameters, the same in every lane of every workgroup of the image
  unsigned long long s8 = (unsigned long long)m.sigma_q8;
  bool apply = true;
  if (m.sigma_q8 == 0) {
    const unsigned long long N = m.stats[0], IMM = m.stats[1];
    // IMM < 2^47, coefficients < 2^16: the products and IMM << 8 fit
    apply = N != 0 && (unsigned long long)ck.rule_a * IMM > (unsigned long long)ck.rule_b * N;
    const unsigned long long a = N != 0 ? (IMM << 8) / N : 0;  // <= 2040 * 256
    s8 = (a * 13689ull) >> 16;                                  // < 2^17
  }
  if (m.verdict != nullptr && *m.verdict != 0) apply = false;
  if (t == 0 && tid == 0 && m.applied != nullptr) *m.applied = apply ? 1 : 0;

  const uintptr_t img = (uintptr_t)m.src, end = img + (uintptr_t)H * W * 3;
  if (!apply) {  // the tile's bytes as they are
    const int len = cols * 3;
    for (int i = tid; i < rows * len; i += NL_THREADS) {
      const int r = i / len, o = i - r * len;
      const size_t at = ((size_t)(y0 + r) * W + x0) * 3 + o;
      m.dst[at] = m.src[at];
    }
    return;
  }
  // s8 < 2^17 and k16 <= 64: 50 s8^2 < 2^40, 25 k16^2 s8^2 < 2^51
  const unsigned long long T0w = (50ull * s8 * s8) >> 16;
  unsigned long long Dw = (25ull * (unsigned long long)(ck.k16 * ck.k16) * s8 * s8) >> 24;
  if (Dw < 1) Dw = 1;
  // d < 2^21, so a T0 of 2^21 and above gives t = 0 like 2^21 itself; D > 2^24 gives Q = 0
  const uint32_t T0 = (uint32_t)(T0w < (1ull << 21) ? T0w : (1ull << 21));
  const uint32_t Q = Dw > (1ull << 24) ? 0u : (uint32_t)((1ull << 24) / Dw);
  // idx = min((t * Q) >> 20, 128) with no 64-bit product in the hot loop: idx is 128 from t = tmax =
  // ceil(2^27 / Q) on, and tmax * Q < 2^27 + Q < 2^32, so min(t, tmax) * Q fits 32 bits and gives the same idx.
  // Q = 2^24 (D = 1) is halved together with the shift; then both factors fit the 24-bit multiplier
  // (t <= 2^21, Qa < 2^24). Q = 0 gives idx = 0 whatever tmax is.
  const uint32_t qhalf = Q >> 24, Qa = Q >> qhalf, qsh = 20u - qhalf;
  const uint32_t tmax = Q != 0 ? min(((1u << 27) + Q - 1u) / Q, 1u << 21) : (1u << 21);

  // stage 1: image rows ylo .. yhi, the bytes of columns xlo .. xhi
  const int ylo = max(y0 - NL_HY, 0), yhi = min(y0 + NL_TR + NL_HY - 1, H - 1);
  const int xlo = max(x0 - NL_HY, 0), xhi = min(x0 + NL_TC + NL_HY - 1, W - 1);
  const int srows = yhi - ylo + 1, len = (xhi - xlo + 1) * 3;
  for (int i = tid; i < srows * NL_VECS; i += NL_THREADS) {
    const int r = i / NL_VECS, v = i - r * NL_VECS;
    const uintptr_t rowp = img + ((uintptr_t)(ylo + r) * W + xlo) * 3;
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
    *(uint4*)(raw + r * NL_RAW_STRIDE + v * 16) = q;
  }
  for (int i = tid; i <= MX_NLM_LUT_SIZE; i += NL_THREADS) lut[i] = i < MX_NLM_LUT_SIZE ? (uint32_t)nlm_lut_dev[i] : 0u;
  __syncthreads();

  // stage 2: staged position (sy, sx) is image pixel clamp(y0 - 7 + sy), clamp(x0 - 7 + sx); an image
  // smaller than the halo clamps on both sides at once
  const int ir = m.bgr ? 2 : 0;
  for (int i = tid; i < NL_YR * NL_YC; i += NL_THREADS) {
    const int sy = i / NL_YC, sx = i - sy * NL_YC;
    const int iy = min(max(y0 - NL_HY + sy, 0), H - 1), ix = min(max(x0 - NL_HY + sx, 0), W - 1);  // in ylo..yhi, xlo..xhi
    const uintptr_t rowp = img + ((uintptr_t)iy * W + xlo) * 3;
    const uint8_t* px = raw + (iy - ylo) * NL_RAW_STRIDE + (int)(rowp & 15) + 3 * (ix - xlo);
    const uint32_t c0 = px[0], c1 = px[1], c2 = px[2];
    const uint32_t R = ir ? c2 : c0, B = ir ? c0 : c2;
    lum[sy * NL_LSTR + NL_YSHIFT + sx] = (uint8_t)((77u * R + 150u * c1 + 29u * B + 128u) >> 8);
    const int xr = sy - (NL_HY - NL_HX), xc = sx - (NL_HY - NL_HX);
    if (xr >= 0 && xr < NL_XR && xc >= 0 && xc < NL_XC) rgb[xr * NL_XSTR + (xc & 3) * NL_XPL + (xc >> 2)] = c0 | (c1 << 8) | (c2 << 16);
  }
  __syncthreads();

  // stage 3: lane (lc, rg) owns tile columns 4 lc .. 4 lc + 3 of rows NL_R rg .. NL_R rg + NL_R - 1
  const int lc = tid & (NL_TC / 4 - 1), rg = tid / (NL_TC / 4);
  const int c0 = 4 * lc, r0 = NL_R * rg;
  if (c0 >= cols || r0 >= rows) return;  // no barrier below
  // patch row j of the lane is tile row r0 - 2 + j = staged row r0 + 5 + j; its own bytes, tile columns
  // c0 - 2 .. c0 + 5, are dwords lc + 2 and lc + 3 of that row
  uint32_t own[NL_R + 4][2];
#pragma unroll
  for (int j = 0; j < NL_R + 4; ++j) {
    const uint32_t* row = (const uint32_t*)(lum + (r0 + NL_HY - NL_P + j) * NL_LSTR);
    own[j][0] = row[lc + 2];
    own[j][1] = row[lc + 3];
  }
  uint32_t wsum[NL_R][4], acc[NL_R][4][3];  // Wsum < 2^19, sum w * X < 2^27
#pragma unroll
  for (int r = 0; r < NL_R; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) wsum[r][k] = acc[r][k][0] = acc[r][k][1] = acc[r][k][2] = 0;

  for (int dy = -NL_S; dy <= NL_S; ++dy) {
    for (int dx = -NL_S; dx <= NL_S; ++dx) {
      const int first = NL_HY - NL_P + NL_YSHIFT + dx;  // byte of the candidate's first column, less 4 lc
      const int sh = first & 3, qd = lc + (first >> 2);
      uint32_t ring[5][4];  // the last five row sums of each column; h < 5 * 255^2 < 2^19
      uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < NL_R + 4; ++j) {
        const uint32_t* qrow = (const uint32_t*)(lum + (r0 + NL_HY - NL_P + j + dy) * NL_LSTR) + qd;
        const uint32_t w0 = qrow[0], w1 = qrow[1], w2 = qrow[2];
        const uint32_t q0 = __builtin_amdgcn_alignbyte(w1, w0, sh), q1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int u0 = (int)((own[j][0] >> (8 * k)) & 255u) - (int)((q0 >> (8 * k)) & 255u);
          const int u1 = (int)((own[j][1] >> (8 * k)) & 255u) - (int)((q1 >> (8 * k)) & 255u);
          e[k] = (uint32_t)(u0 * u0);
          e[4 + k] = (uint32_t)(u1 * u1);
        }
        uint32_t h[4];
        h[0] = e[0] + e[1] + e[2] + e[3] + e[4];
        h[1] = h[0] - e[0] + e[5];
        h[2] = h[1] - e[1] + e[6];
        h[3] = h[2] - e[2] + e[7];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          d[k] += h[k];
          if (j >= 5) d[k] -= ring[j % 5][k];
          ring[j % 5][k] = h[k];
        }
        if (j >= 4) {  // patch rows j - 4 .. j are in: the distance of lane row r = j - 4 is complete
          const int r = j - 4;
          const uint32_t* xrow = rgb + (r0 + r + NL_HX + dy) * NL_XSTR;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t tt = min(max(d[k], T0) - T0, tmax);
            const uint32_t idx = min((uint32_t)__umul24(tt, Qa) >> qsh, (uint32_t)MX_NLM_LUT_SIZE);
            const uint32_t w = lut[idx];  // <= 4096: w * X below goes through the 24-bit multiplier too
            const int xc = k + NL_HX + dx;  // the candidate's staged column, less c0
            const uint32_t x = xrow[(xc & 3) * NL_XPL + lc + (xc >> 2)];
            wsum[r][k] += w;
            acc[r][k][0] += __umul24(w, x & 255u);
            acc[r][k][1] += __umul24(w, (x >> 8) & 255u);
            acc[r][k][2] += __umul24(w, (x >> 16) & 255u);
          }
        }
      }
    }
  }

  // stage 4: Wsum >= 4096 (the centre has t = 0)
#pragma unroll
  for (int r = 0; r < NL_R; ++r) {
    if (r0 + r >= rows) break;
    uint8_t* o = m.dst + ((size_t)(y0 + r0 + r) * W + x0 + c0) * 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c0 + k >= cols) break;
      const uint32_t ws = wsum[r][k];
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * k + c] = (uint8_t)((acc[r][k][c] + (ws >> 1)) / ws);
    }
  }
}

}  // namespace mx

using namespace mx;

extern "C" int mx_denoise_nlm_tile(int32_t out[2]) {
  MX_CHECK_ARG(out != nullptr, "mx_denoise_nlm_tile: null output");
  out[0] = NL_TR;
  out[1] = NL_TC;
  return MX_OK;
}

extern "C" int mx_denoise_nlm_lut(int32_t out[128]) {
  MX_CHECK_ARG(out != nullptr, "mx_denoise_nlm_lut: null output");
  for (int i = 0; i < MX_NLM_LUT_SIZE; ++i) out[i] = nlm_lut_host[i];
  return MX_OK;
}

extern "C" int mx_denoise_nlm_u8(const mx_nlm_desc* descs_host, int64_t n, const int64_t* stats, const int32_t* verdict,
                                 int32_t rule_a, int32_t rule_b, int32_t k16, int32_t* applied, mx_stream_t stream) {
  // everything is checked before the first launch
  MX_CHECK_ARG(n >= 0 && (n == 0 || descs_host), "mx_denoise_nlm_u8: bad descriptor array");
  MX_CHECK_ARG(k16 >= 1 && k16 <= 64, "mx_denoise_nlm_u8: k16 %d outside 1..64", k16);
  MX_CHECK_ARG(rule_a >= 0 && rule_a <= 65535 && rule_b >= 0 && rule_b <= 65535,
               "mx_denoise_nlm_u8: rule coefficient outside 0..65535");
  for (int64_t b = 0; b < n; ++b) {
    const mx_nlm_desc& d = descs_host[b];
    MX_CHECK_ARG(d.src != nullptr && d.dst != nullptr, "mx_denoise_nlm_u8: image %lld: null image", (long long)b);
    MX_CHECK_ARG(d.H >= 1 && d.W >= 1 && (int64_t)d.H * d.W <= ((int64_t)1 << 24),
                 "mx_denoise_nlm_u8: image %lld: bad size %d x %d (1 <= H, W and H * W <= 2^24)", (long long)b, d.H, d.W);
    MX_CHECK_ARG(d.sigma_q8 >= 0 && d.sigma_q8 <= 65535, "mx_denoise_nlm_u8: image %lld: sigma_q8 %d outside 0..65535",
                 (long long)b, d.sigma_q8);
    if (d.sigma_q8 == 0) {
      MX_CHECK_ARG(stats != nullptr, "mx_denoise_nlm_u8: image %lld: a blind image without stats", (long long)b);
      MX_CHECK_ARG(d.H >= 3 && d.W >= 3, "mx_denoise_nlm_u8: image %lld: a blind image of %d x %d has no stats (3 <= H, W)",
                   (long long)b, d.H, d.W);
    }
  }
  // a tile reads pixels that another tile writes: no output may overlap any input of the call
  for (int64_t i = 0; i < n; ++i) {
    const uintptr_t d0 = (uintptr_t)descs_host[i].dst, d1 = d0 + (uintptr_t)descs_host[i].H * descs_host[i].W * 3;
    for (int64_t j = 0; j < n; ++j) {
      const uintptr_t s0 = (uintptr_t)descs_host[j].src, s1 = s0 + (uintptr_t)descs_host[j].H * descs_host[j].W * 3;
      MX_CHECK_ARG(d1 <= s0 || s1 <= d0, "mx_denoise_nlm_u8: image %lld: dst overlaps the src of image %lld", (long long)i,
                   (long long)j);
    }
  }
  if (n == 0) return MX_OK;

  hipStream_t s = (hipStream_t)stream;
  NlChunk ck{};
  ck.rule_a = rule_a;
  ck.rule_b = rule_b;
  ck.k16 = k16;
  int64_t tiles = 0;
  auto flush = [&]() -> int {
    if (ck.n > 0 && tiles > 0) {
      nlm_kernel<<<(unsigned)tiles, NL_THREADS, 0, s>>>(ck);
      MX_LAUNCH_CHECK();
    }
    ck.n = 0;
    tiles = 0;
    return MX_OK;
  };
  for (int64_t b = 0; b < n; ++b) {
    const mx_nlm_desc& d = descs_host[b];
    const int64_t tx = cdiv(d.W, NL_TC), tyn = cdiv(d.H, NL_TR);
    if (ck.n == NL_IMGS) {
      const int rc = flush();
      if (rc) return rc;
    }
    NlImg& m = ck.im[ck.n];
    m.src = d.src;
    m.dst = d.dst;
    m.stats = d.sigma_q8 == 0 ? (const unsigned long long*)stats + b * 8 : nullptr;
    m.verdict = verdict ? verdict + b : nullptr;
    m.applied = applied ? applied + b : nullptr;
    m.H = d.H; m.W = d.W; m.bgr = d.bgr != 0; m.sigma_q8 = d.sigma_q8;
    m.tile0 = (int32_t)tiles;
    m.tiles_x = (int32_t)tx;
    tiles += tx * tyn;  // <= 16 images of <= 2^24 pixels, a tile per 32 pixels at the least: far below 2^31
    ++ck.n;
  }
  return flush();
}
