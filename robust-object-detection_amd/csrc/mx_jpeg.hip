// mx_jpeg.hip — device half of the hybrid baseline-JPEG decoder (host half: mx_jpeg.cpp), and below it
// the device JPEG encoder (pixel stage + entropy coder).
//
// Reproduces libjpeg-turbo's default decompression (the decoder behind PIL and cv2.imread,
// coco_detection_dataset.py:23, restore_testsets.py:99) bit for bit:
//   idct_kernel      dequantisation + jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2, 64-bit
//                    intermediates like JLONG, the post-IDCT range-limit table of jdmaster.c
//                    prepare_range_limit_table indexed by x & 1023), one thread per 8x8 block, written
//                    into MCU-padded component planes;
//   colour_kernel    per output pixel: chroma "fancy" upsampling (jdsample.c h2v1_fancy_upsample /
//                    h2v2_fancy_upsample: triangle filter, rows beyond the image replicated like
//                    jdmainct.c's context rows; plain replication when downsampled_width <= 2) and
//                    ycc_rgb_convert (jdcolor.c tables, SCALEBITS 16), grey replicated to RGB.
//   window_kernel    both stages for a window of the frame in one launch, through LDS instead of the
//                    component planes (mx_jpeg_reconstruct_window, below the full path).
// All are integer kernels (no float anywhere); the first two are HBM-bound streaming work.
#include "mx_common.h"
#include "mx_jpeg_walk.h"

namespace mx {

struct JpegDev {
  int32_t width, height, ncomp;
  int32_t h[3], v[3], tq[3];
  int32_t hmax, vmax;
  int32_t bw[3], bh[3], dw[3], dh[3];
  int64_t coef_off[3], plane_off[3];
  int64_t nblocks[3];
  uint16_t qt[4][64];
};

// post-IDCT range limit (jdmaster.c prepare_range_limit_table, idct table = sample_range_limit +
// CENTERJSAMPLE): x & 1023 -> [0,128): x+128, [128,512): 255, [512,896): 0, [896,1024): x-896
__device__ __forceinline__ uint8_t idct_limit(int64_t x) {
  const int i = (int)(x & 1023);
  return i < 128 ? (uint8_t)(i + 128) : (i < 512 ? 255 : (i < 896 ? 0 : (uint8_t)(i - 896)));
}

#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

__device__ __forceinline__ int64_t descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }

// one 1-D islow pass over in[0..7] (stride-free), CONST_BITS 13; returns the 8 outputs before the
// final descale (shared by both passes)
__device__ __forceinline__ void idct8(const int64_t* in, int64_t* o) {
  int64_t z2 = in[2], z3 = in[6];
  int64_t z1 = (z2 + z3) * FIX_0_541196100;
  const int64_t tmp2e = z1 + z3 * (-FIX_1_847759065);
  const int64_t tmp3e = z1 + z2 * FIX_0_765366865;
  const int64_t tmp0e = (in[0] + in[4]) * 8192;
  const int64_t tmp1e = (in[0] - in[4]) * 8192;
  const int64_t tmp10 = tmp0e + tmp3e, tmp13 = tmp0e - tmp3e, tmp11 = tmp1e + tmp2e, tmp12 = tmp1e - tmp2e;
  int64_t tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int64_t z4 = tmp1 + tmp3;
  const int64_t z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 = tmp0 * FIX_0_298631336;
  tmp1 = tmp1 * FIX_2_053119869;
  tmp2 = tmp2 * FIX_3_072711026;
  tmp3 = tmp3 * FIX_1_501321110;
  z1 = z1 * (-FIX_0_899976223);
  z2 = z2 * (-FIX_2_562915447);
  z3 = z3 * (-FIX_1_961570560);
  z4 = z4 * (-FIX_0_390180644);
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  o[0] = tmp10 + tmp3;
  o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2;
  o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1;
  o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0;
  o[4] = tmp13 - tmp0;
}

__global__ void __launch_bounds__(256) jpeg_idct_kernel(const int16_t* __restrict__ coefs, JpegDev j,
                                                        uint8_t* __restrict__ planes) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int c = 0;
  while (c < j.ncomp && b >= j.nblocks[c]) b -= j.nblocks[c++];
  if (c >= j.ncomp) return;
  const int16_t* src = coefs + j.coef_off[c] + b * 64;
  const uint16_t* q = j.qt[j.tq[c]];
  int16_t cf[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) *(uint4*)&cf[8 * i] = ((const uint4*)src)[i];
  int64_t ws[64];
  // pass 1: columns (DEQUANTIZE = coef * q), outputs descaled by CONST_BITS - PASS1_BITS
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int64_t in[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = (int64_t)cf[r * 8 + col] * q[r * 8 + col];
    idct8(in, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r * 8 + col] = (int64_t)(int32_t)descale(o[r], 11);
  }
  const int64_t by = b / j.bw[c], bx = b % j.bw[c];
  const int64_t stride = (int64_t)j.bw[c] * 8;
  uint8_t* dst = planes + j.plane_off[c] + by * 8 * stride + bx * 8;
  // pass 2: rows, descaled by CONST_BITS + PASS1_BITS + 3, range-limited
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int64_t o[8];
    idct8(&ws[r * 8], o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      lo |= (uint32_t)idct_limit(descale(o[t], 18)) << (8 * t);
      hi |= (uint32_t)idct_limit(descale(o[t + 4], 18)) << (8 * t);
    }
    *(uint2*)(dst + r * stride) = make_uint2(lo, hi);
  }
}

__device__ __forceinline__ int clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }
__device__ __forceinline__ int sel3(const int32_t* a, int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// upsampled chroma sample at output (x, y) of a component whose plane sample (row, col) is at(row, col)
// (jdsample.c). The dw > 2 switch and the clamps are those of the image: dw, dh are the component's
// downsampled size, whatever part of the plane `at` can reach.
template <typename P>
__device__ __forceinline__ int chroma_at(P at, int hs, int vs, int dw, int dh, int x, int y) {
  if (hs == 1 && vs == 1) return at(y, x);
  const bool fancy = dw > 2;
  if (!fancy) return at(y / vs, x / hs);  // h2v1_upsample / h2v2_upsample: replicate
  const int cx = x >> 1;
  if (vs == 1) {  // h2v1 fancy
    const int v0 = at(y, cx);
    if ((x & 1) == 0) return cx == 0 ? v0 : (v0 * 3 + at(y, cx - 1) + 1) >> 2;
    return cx == dw - 1 ? v0 : (v0 * 3 + at(y, cx + 1) + 2) >> 2;
  }
  // h2v2 fancy: the nearer sample row (3/4) and the other row (1/4), rows clamped to the image
  const int r0 = y >> 1;
  int r1 = (y & 1) ? r0 + 1 : r0 - 1;
  r1 = r1 < 0 ? 0 : (r1 > dh - 1 ? dh - 1 : r1);
  const int cs = at(r0, cx) * 3 + at(r1, cx);
  if ((x & 1) == 0) {
    if (cx == 0) return (cs * 4 + 8) >> 4;
    return (cs * 3 + at(r0, cx - 1) * 3 + at(r1, cx - 1) + 8) >> 4;
  }
  if (cx == dw - 1) return (cs * 4 + 7) >> 4;
  return (cs * 3 + at(r0, cx + 1) * 3 + at(r1, cx + 1) + 7) >> 4;
}

// the same over a whole component plane in memory
__device__ __forceinline__ int chroma(const uint8_t* pl, int64_t stride, int hs, int vs, int dw, int dh, int x, int y) {
  return chroma_at([=](int r, int c) -> int { return pl[(int64_t)r * stride + c]; }, hs, vs, dw, dh, x, y);
}

// jdcolor.c build_ycc_rgb_table (FIX(x) = (int)(x * 65536 + 0.5), ONE_HALF = 1 << 15)
__device__ __forceinline__ void ycc_rgb(int Y, int cb, int cr, int& R, int& G, int& B) {
  const int xcr = cr - 128, xcb = cb - 128;
  const int crr = (91881 * xcr + 32768) >> 16;
  const int cbb = (116130 * xcb + 32768) >> 16;
  const int g = (-46802 * xcr + (-22554 * xcb + 32768)) >> 16;
  R = clamp255(Y + crr);
  G = clamp255(Y + g);
  B = clamp255(Y + cbb);
}

__global__ void __launch_bounds__(256) jpeg_colour_kernel(const uint8_t* __restrict__ planes, JpegDev j, int bgr,
                                                          uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)j.width * j.height) return;
  const int x = (int)(i % j.width), y = (int)(i / j.width);
  const int Y = planes[j.plane_off[0] + (int64_t)y * j.bw[0] * 8 + x];
  int R, G, B;
  if (j.ncomp == 1) {
    R = G = B = Y;
  } else {
    const int hs = j.hmax / j.h[1], vs = j.vmax / j.v[1];  // chroma components share one sampling
    const int cb = chroma(planes + j.plane_off[1], (int64_t)j.bw[1] * 8, hs, vs, j.dw[1], j.dh[1], x, y);
    const int cr = chroma(planes + j.plane_off[2], (int64_t)j.bw[2] * 8, hs, vs, j.dw[2], j.dh[2], x, y);
    ycc_rgb(Y, cb, cr, R, G, B);
  }
  uint8_t* o = out + i * 3;
  o[0] = (uint8_t)(bgr ? B : R);
  o[1] = (uint8_t)G;
  o[2] = (uint8_t)(bgr ? R : B);
}

static void to_dev(const mx_jpeg_info* in, JpegDev* j, int64_t* plane_bytes) {
  j->width = in->width;
  j->height = in->height;
  j->ncomp = in->ncomp;
  j->hmax = in->hmax;
  j->vmax = in->vmax;
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < in->ncomp;
    j->h[c] = on ? in->h[c] : 1;
    j->v[c] = on ? in->v[c] : 1;
    j->tq[c] = on ? in->tq[c] : 0;
    j->bw[c] = on ? in->bw[c] : 0;
    j->bh[c] = on ? in->bh[c] : 0;
    j->dw[c] = on ? in->dw[c] : 0;
    j->dh[c] = on ? in->dh[c] : 0;
    j->coef_off[c] = on ? in->coef_off[c] : 0;
    j->nblocks[c] = on ? (int64_t)in->bw[c] * in->bh[c] : 0;
    j->plane_off[c] = off;
    off += j->nblocks[c] * 64;
  }
  for (int t = 0; t < 4; ++t)
    for (int k = 0; k < 64; ++k) j->qt[t][k] = in->qt[t][k];
  *plane_bytes = off;
}

}  // namespace mx

using namespace mx;

extern "C" size_t mx_jpeg_workspace(const mx_jpeg_info* info) {
  if (!info) return 0;
  JpegDev j;
  int64_t bytes = 0;
  to_dev(info, &j, &bytes);
  return (size_t)bytes;
}

extern "C" int mx_jpeg_reconstruct(const int16_t* coefs, const mx_jpeg_info* info, void* ws, size_t ws_bytes,
                                   uint8_t* out, int bgr, mx_stream_t stream) {
  MX_CHECK_ARG(coefs && info && out, "jpeg_reconstruct: null argument");
  MX_CHECK_ARG(info->ncomp == 1 || info->ncomp == 3, "jpeg_reconstruct: 1 or 3 components");
  MX_CHECK_ARG(info->width > 0 && info->height > 0 && info->coef_total > 0, "jpeg_reconstruct: parse the image first");
  JpegDev j;
  int64_t need = 0;
  to_dev(info, &j, &need);
  MX_CHECK_ARG(ws && (int64_t)ws_bytes >= need, "jpeg_reconstruct: workspace of %lld bytes required", (long long)need);
  const int64_t nb = j.nblocks[0] + j.nblocks[1] + j.nblocks[2];
  hipStream_t st = (hipStream_t)stream;
  jpeg_idct_kernel<<<(unsigned)cdiv(nb, 256), 256, 0, st>>>(coefs, j, (uint8_t*)ws);
  MX_LAUNCH_CHECK();
  const int64_t np = (int64_t)j.width * j.height;
  jpeg_colour_kernel<<<(unsigned)cdiv(np, 256), 256, 0, st>>>((const uint8_t*)ws, j, bgr, out);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

// ================================================================================================
// Windowed reconstruct: the pixels of a window of the frame straight from the coefficients, without
// the full-frame component planes (mx_jpeg_reconstruct_window; the U-Net patch loader keeps a 256x256
// crop of a 1920x1080 frame). One workgroup per 32x32-pixel tile of the IMAGE grid (a multiple of
// every accepted MCU, so a tile's luma blocks are whole blocks); the part of the tile inside the
// window is its rectangle. jpeg_window_cover() names the blocks of each component that rectangle
// reads: its luma blocks, and the chroma blocks under it plus the one-sample halo of the fancy
// upsampling (at most 4 x 4 blocks per component). The workgroup loads those blocks (16 B per lane),
// runs the islow IDCT with 8 lanes per block (column pass, then row pass, through LDS) into LDS
// planes, and after a barrier every lane upsamples, converts and stores its pixels with the
// arithmetic of the full path (idct8, descale, idct_limit, chroma_at, ycc_rgb). The fancy / replicate
// switch and the edge clamps are the image's (dw, dh), never the tile's: at a tile or window edge
// inside the image the neighbour sample is real data from the halo block.
// ================================================================================================
namespace mx {

constexpr int kWinTile = 32;    // pixels a side
constexpr int kWinPitch = 40;   // bytes per row of an LDS plane: 4 blocks across + 8 (8-B aligned rows)
constexpr int kWinSlots = 32;   // blocks per IDCT round: 256 lanes / 8
constexpr int kWinWsPitch = 65; // words per block of the IDCT workspace: the 8 blocks of a wave on 8 banks

struct JpegWinGeom {
  int32_t ncomp, hs, vs, dw, dh;  // chroma upsampling factors and downsampled size (both chroma components)
};

// Blocks (bx0, by0, bx1, by1; high end exclusive) of every component that hold a sample the pixels
// [x0, x1] x [y0, y1] (inclusive, inside the image) read: chroma_at()'s taps restated as ranges.
__host__ __device__ inline void jpeg_window_cover(const JpegWinGeom& g, int x0, int y0, int x1, int y1,
                                                  int32_t cover[3][4]) {
  cover[0][0] = x0 >> 3;
  cover[0][1] = y0 >> 3;
  cover[0][2] = (x1 >> 3) + 1;
  cover[0][3] = (y1 >> 3) + 1;
  int cl = x0, cr = x1, rt = y0, rb = y1;  // chroma sample columns / rows, inclusive
  if (g.hs == 1 && g.vs == 1) {
  } else if (g.dw <= 2) {  // replicate
    cl = x0 / g.hs;
    cr = x1 / g.hs;
    rt = y0 / g.vs;
    rb = y1 / g.vs;
  } else {
    cl = x0 >> 1;
    if ((x0 & 1) == 0 && cl > 0) --cl;  // an even column reads its left neighbour
    cr = x1 >> 1;
    if ((x1 & 1) == 1 && cr < g.dw - 1) ++cr;  // an odd column its right one
    if (g.vs == 2) {
      rt = y0 >> 1;
      if ((y0 & 1) == 0 && rt > 0) --rt;
      rb = y1 >> 1;
      if ((y1 & 1) == 1 && rb < g.dh - 1) ++rb;
    }
  }
  for (int c = 1; c < 3; ++c) {
    const bool on = g.ncomp == 3;
    cover[c][0] = on ? cl >> 3 : 0;
    cover[c][1] = on ? rt >> 3 : 0;
    cover[c][2] = on ? (cr >> 3) + 1 : 0;
    cover[c][3] = on ? (rb >> 3) + 1 : 0;
  }
}

__global__ void __launch_bounds__(256) jpeg_window_kernel(const int16_t* __restrict__ coefs, JpegDev j, int x0, int y0,
                                                          int w, int h, int hflip, int bgr, uint8_t* __restrict__ out,
                                                          int64_t out_row_bytes) {
  __shared__ __attribute__((aligned(16))) uint8_t pl[3][kWinTile * kWinPitch];
  __shared__ int ws[kWinSlots * kWinWsPitch];
  __shared__ uint16_t qd[3][64];
  const int t = threadIdx.x;
  const int X = ((x0 >> 5) + (int)blockIdx.x) * kWinTile, Y = ((y0 >> 5) + (int)blockIdx.y) * kWinTile;
  // the tile's rectangle: its pixels inside the window
  const int rx0 = max(X, x0), ry0 = max(Y, y0);
  const int rx1 = min(X + kWinTile - 1, x0 + w - 1), ry1 = min(Y + kWinTile - 1, y0 + h - 1);
  JpegWinGeom g;
  g.ncomp = j.ncomp;
  g.hs = j.hmax / j.h[1];  // chroma components share one sampling
  g.vs = j.vmax / j.v[1];
  g.dw = j.dw[1];
  g.dh = j.dh[1];
  int32_t cov[3][4];
  jpeg_window_cover(g, rx0, ry0, rx1, ry1, cov);
  const int lbx0 = cov[0][0], lby0 = cov[0][1], lnx = cov[0][2] - cov[0][0];
  const int cbx0 = cov[1][0], cby0 = cov[1][1], cnx = cov[1][2] - cov[1][0];
  const int nb0 = lnx * (cov[0][3] - cov[0][1]);
  const int nb1 = cnx * (cov[1][3] - cov[1][1]);  // 0 for a grey frame; the two chroma covers are equal
  const int nblk = nb0 + 2 * nb1;
  if (t < 192) qd[t >> 6][t & 63] = j.qt[sel3(j.tq, t >> 6)][t & 63];
  __syncthreads();
  // ---- dequantisation + jpeg_idct_islow, 8 lanes per block, 32 blocks per round
  const int l = t & 7, slot = t >> 3;
  int* wsb = &ws[slot * kWinWsPitch];
  for (int base = 0; base < nblk; base += kWinSlots) {
    int k = base + slot;
    const bool on = k < nblk;
    int c = 0;
    if (k >= nb0) {
      k -= nb0;
      c = 1;
      if (k >= nb1) {
        k -= nb1;
        c = 2;
      }
    }
    const int nx = c == 0 ? lnx : cnx;
    const int by = on ? k / nx : 0, bx = on ? k - by * nx : 0;  // inside the component's cover
    if (on) {
      const int64_t gb = (int64_t)((c == 0 ? lby0 : cby0) + by) * sel3(j.bw, c) + (c == 0 ? lbx0 : cbx0) + bx;
      const int64_t off = c == 0 ? j.coef_off[0] : (c == 1 ? j.coef_off[1] : j.coef_off[2]);
      const uint4 u = *(const uint4*)(coefs + off + gb * 64 + l * 8);  // row l of the block
      const uint32_t uw[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) wsb[l * 8 + e] = (int)(int16_t)((uw[e >> 1] >> ((e & 1) * 16)) & 0xffff);
    }
    __syncthreads();
    if (on) {  // pass 1: column l (DEQUANTIZE = coef * q), outputs descaled by CONST_BITS - PASS1_BITS
      int64_t in[8], o[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) in[r] = (int64_t)wsb[r * 8 + l] * qd[c][r * 8 + l];
      idct8(in, o);
#pragma unroll
      for (int r = 0; r < 8; ++r) wsb[r * 8 + l] = (int32_t)descale(o[r], 11);
    }
    __syncthreads();
    if (on) {  // pass 2: row l, descaled by CONST_BITS + PASS1_BITS + 3, range-limited
      int64_t in[8], o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) in[e] = (int64_t)wsb[l * 8 + e];
      idct8(in, o);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo |= (uint32_t)idct_limit(descale(o[e], 18)) << (8 * e);
        hi |= (uint32_t)idct_limit(descale(o[e + 4], 18)) << (8 * e);
      }
      *(uint2*)&pl[c][(by * 8 + l) * kWinPitch + bx * 8] = make_uint2(lo, hi);
    }
    __syncthreads();
  }
  // ---- upsampling + colour conversion from the LDS planes; lanes outside the rectangle store nothing
  const int hs = g.hs, vs = g.vs, dw = g.dw, dh = g.dh;
  const int x = X + (t & 31);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int y = Y + (t >> 5) + 8 * q;
    if (x < rx0 || x > rx1 || y < ry0 || y > ry1) continue;
    const int Yv = pl[0][(y - lby0 * 8) * kWinPitch + (x - lbx0 * 8)];
    int R, G, B;
    if (j.ncomp == 1) {
      R = G = B = Yv;
    } else {
      const uint8_t* p1 = pl[1];
      const uint8_t* p2 = pl[2];
      const int cb = chroma_at([=](int r, int cc) -> int { return p1[(r - cby0 * 8) * kWinPitch + (cc - cbx0 * 8)]; },
                               hs, vs, dw, dh, x, y);
      const int cr = chroma_at([=](int r, int cc) -> int { return p2[(r - cby0 * 8) * kWinPitch + (cc - cbx0 * 8)]; },
                               hs, vs, dw, dh, x, y);
      ycc_rgb(Yv, cb, cr, R, G, B);
    }
    const int col = hflip ? w - 1 - (x - x0) : x - x0;
    uint8_t* o = out + (int64_t)(y - y0) * out_row_bytes + (int64_t)col * 3;
    o[0] = (uint8_t)(bgr ? B : R);
    o[1] = (uint8_t)G;
    o[2] = (uint8_t)(bgr ? R : B);
  }
}

// what both window entry points require of (info, window); nullptr when fine
static const char* win_check(const mx_jpeg_info* info, int x0, int y0, int w, int h, JpegWinGeom* g) {
  if (!info) return "null argument";
  if (info->ncomp != 1 && info->ncomp != 3) return "1 or 3 components";
  if (info->width <= 0 || info->height <= 0 || info->coef_total <= 0) return "parse the image first";
  if (w <= 0 || h <= 0) return "empty window";
  if (x0 < 0 || y0 < 0 || (int64_t)x0 + w > info->width || (int64_t)y0 + h > info->height)
    return "window outside the image";
  g->ncomp = info->ncomp;
  g->hs = g->vs = 1;
  g->dw = g->dh = 0;
  if (info->ncomp == 3) {
    const int h0 = info->h[0], v0 = info->v[0];
    const bool ok = info->h[1] == 1 && info->v[1] == 1 && info->h[2] == 1 && info->v[2] == 1 && info->hmax == h0 &&
                    info->vmax == v0 && ((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2));
    if (!ok) return "chroma subsampling 4:4:4, 4:2:2 or 4:2:0 only";
    g->hs = h0;
    g->vs = v0;
    g->dw = info->dw[1];
    g->dh = info->dh[1];
    if (info->dw[2] != g->dw || info->dh[2] != g->dh || g->dw != (info->width + h0 - 1) / h0 ||
        g->dh != (info->height + v0 - 1) / v0)
      return "inconsistent downsampled size";
  }
  // every block the window can name lies inside the coefficient layout
  int32_t cov[3][4];
  jpeg_window_cover(*g, 0, 0, info->width - 1, info->height - 1, cov);
  int64_t off = 0;
  for (int c = 0; c < info->ncomp; ++c) {
    if (cov[c][2] > info->bw[c] || cov[c][3] > info->bh[c] || info->coef_off[c] != off || info->tq[c] < 0 ||
        info->tq[c] > 3)
      return "inconsistent block layout";
    off += (int64_t)info->bw[c] * info->bh[c] * 64;
  }
  if (off != info->coef_total) return "inconsistent coefficient total";
  return nullptr;
}

}  // namespace mx

extern "C" int mx_jpeg_window_cover(const mx_jpeg_info* info, int x0, int y0, int w, int h, int32_t cover[3][4]) {
  MX_CHECK_ARG(cover, "jpeg_window_cover: null argument");
  JpegWinGeom g;
  const char* bad = win_check(info, x0, y0, w, h, &g);
  MX_CHECK_ARG(!bad, "jpeg_window_cover: %s", bad);
  jpeg_window_cover(g, x0, y0, x0 + w - 1, y0 + h - 1, cover);
  return MX_OK;
}

extern "C" int mx_jpeg_reconstruct_window(const int16_t* coefs, const mx_jpeg_info* info, int x0, int y0, int w, int h,
                                          int hflip, int bgr, uint8_t* out, int64_t out_row_bytes, mx_stream_t stream) {
  MX_CHECK_ARG(coefs && info && out, "jpeg_reconstruct_window: null argument");
  JpegWinGeom g;
  const char* bad = win_check(info, x0, y0, w, h, &g);
  MX_CHECK_ARG(!bad, "jpeg_reconstruct_window: %s", bad);
  MX_CHECK_ARG(out_row_bytes >= (int64_t)3 * w, "jpeg_reconstruct_window: out_row_bytes below 3 * w = %lld",
               (long long)3 * w);
  MX_CHECK_ARG(((uintptr_t)coefs & 15) == 0, "jpeg_reconstruct_window: coefficients must be 16-byte aligned");
  JpegDev j;
  int64_t unused = 0;
  to_dev(info, &j, &unused);
  const dim3 grid((unsigned)(((x0 + w - 1) >> 5) - (x0 >> 5) + 1), (unsigned)(((y0 + h - 1) >> 5) - (y0 >> 5) + 1));
  jpeg_window_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(coefs, j, x0, y0, w, h, hflip ? 1 : 0, bgr ? 1 : 0, out,
                                                          out_row_bytes);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

// ================================================================================================
// Encoder, device half. Reproduces libjpeg-turbo's default compression (PIL Image.save(format="JPEG",
// quality, subsampling), cv2.imwrite) byte for byte:
//   jpeg_forward_kernel   one workgroup per 64-pixel-wide strip of one MCU row (4 MCUs at 4:2:0, 8 at
//                         4:4:4; 24 blocks either way), everything through LDS: 16-B pixel loads,
//                         rgb_ycc_convert (jccolor.c, SCALEBITS 16), edge replication at full
//                         resolution (jcprepct.c: columns to the block grid, rows only to an even
//                         count), h2v2_downsample (jcsample.c, alternating 1/2 bias) with the
//                         DOWNSAMPLED rows replicated to the iMCU height, jpeg_fdct_islow (jfdctint.c)
//                         as a row pass and a column pass of 8 lanes per block, the quantiser of
//                         jcdctmgr.c, the dummy blocks of jccoefct.c, 16-B coefficient stores.
//   entropy passes        (a) jpeg_count_kernel: exact bit count of every block in scan order + scan
//                         inside the workgroup; (b) jpeg_scan_bits_kernel: one workgroup scans the
//                         workgroup sums; jpeg_zero_kernel clears the words the stream will occupy;
//                         (c) jpeg_emit_kernel: every block writes its bits MSB first (atomicOr on the
//                         words it shares with neighbours, 1-padding of the tail); (d) jpeg_ff_count /
//                         jpeg_scan_ff / jpeg_stuff kernels: 0xFF bytes per 4-KiB chunk, scan, scatter
//                         with the stuffed 0x00. No pass waits on another workgroup; every launch is
//                         sized on the host from the worst case and exits early on the device total.
// ================================================================================================
namespace mx {

bool jpeg_enc_table(const uint8_t* bits, const uint8_t* vals, uint32_t* tab);  // mx_jpeg.cpp

struct JpegFwd {
  int32_t width, height, mcux, bgr;
  int32_t bw[3];
  int32_t wib0, hib0;  // luma blocks that hold image samples, across / down
  int64_t coef_off[3];
  uint16_t qt[3][64];  // per component
};

template <int PASS>
__device__ __forceinline__ void fdct8(const int* d, int* o) {
  const int s = PASS == 0 ? 11 : 15;  // CONST_BITS -/+ PASS1_BITS
  int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (PASS == 0) {
    o[0] = (tmp10 + tmp11) << 2;
    o[4] = (tmp10 - tmp11) << 2;
  } else {
    o[0] = (tmp10 + tmp11 + 2) >> 2;
    o[4] = (tmp10 - tmp11 + 2) >> 2;
  }
  int z1 = (tmp12 + tmp13) * FIX_0_541196100;
  o[2] = (z1 + tmp13 * FIX_0_765366865 + (1 << (s - 1))) >> s;
  o[6] = (z1 + tmp12 * (-FIX_1_847759065) + (1 << (s - 1))) >> s;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  tmp4 *= FIX_0_298631336;
  tmp5 *= FIX_2_053119869;
  tmp6 *= FIX_3_072711026;
  tmp7 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 = z3 * (-FIX_1_961570560) + z5;
  z4 = z4 * (-FIX_0_390180644) + z5;
  o[7] = (tmp4 + z1 + z3 + (1 << (s - 1))) >> s;
  o[5] = (tmp5 + z2 + z4 + (1 << (s - 1))) >> s;
  o[3] = (tmp6 + z2 + z3 + (1 << (s - 1))) >> s;
  o[1] = (tmp7 + z1 + z4 + (1 << (s - 1))) >> s;
}

constexpr int kFwdBlocks = 24;  // blocks per workgroup: 16 + 4 + 4 (4:2:0) or 8 + 8 + 8 (4:4:4)
constexpr int kRawPitch = 224;  // 64 pixels * 3 + up to 15 bytes of misalignment, in 16-B chunks

// block b of the workgroup's tile -> component, plane row of its first sample, plane column
template <int SUB>
__device__ __forceinline__ void fwd_block(int b, int& c, int& row0, int& col0) {
  if (SUB == 2) {
    if (b < 16) {
      c = 0;
      row0 = (b >> 3) * 8;
      col0 = (b & 7) * 8;
    } else {
      c = 1 + ((b - 16) >> 2);
      row0 = 0;
      col0 = ((b - 16) & 3) * 8;
    }
  } else {
    c = b >> 3;
    row0 = 0;
    col0 = (b & 7) * 8;
  }
}

// The front of the pixel stage, shared by jpeg_forward_kernel and jpeg_roundtrip_kernel: the tile at
// (x0, y0) of the [height][width][3] image `img` -> raw (16-B chunks) -> component planes pl (colour
// conversion, edge replication, h2v2 downsampling) -> pass 1 of jpeg_fdct_islow into ws (block pitch
// 72 words: the 8 blocks of a wave hit 8 bank groups). Lane t works on row l = t & 7 of block
// b = t >> 3 (component c, first plane sample (row0, col0)); ws holds every block when it returns.
// SUB 2: 4:2:0 (luma 2x2 blocks per MCU), SUB 1: 4:4:4
template <int SUB>
__device__ __forceinline__ void fwd_tile_pass1(const uint8_t* __restrict__ img, int width, int height, int bgr, int x0,
                                               int y0, uint8_t* raw, uint8_t (*pl)[16][64], int* ws, int& c, int& row0,
                                               int& col0) {
  constexpr int ROWS = 8 * SUB;  // pixel rows of the tile
  const int t = threadIdx.x;
  const int xmax = min(63, width - 1 - x0), rmax = min(ROWS - 1, height - 1 - y0);
  // ---- pixels -> LDS in 16-B chunks aligned in memory; chunks that straddle the tensor go by bytes
  const uintptr_t base = (uintptr_t)img, end = base + (uintptr_t)width * height * 3;
  {
    const int r = t / 14, ch = t % 14;
    if (r <= rmax) {
      const uintptr_t a = base + ((uintptr_t)(y0 + r) * width + x0) * 3;
      const uintptr_t stop = a + (uintptr_t)(xmax + 1) * 3;
      const uintptr_t p = (a & ~(uintptr_t)15) + 16 * ch;
      if (p < stop) {
        uint4 v;
        if (p >= base && p + 16 <= end) {
          v = *(const uint4*)p;
        } else {
          uint8_t* vb = (uint8_t*)&v;
#pragma unroll
          for (int k = 0; k < 16; ++k) vb[k] = (p + k >= base && p + k < end) ? *(const uint8_t*)(p + k) : 0;
        }
        *(uint4*)&raw[r * kRawPitch + 16 * ch] = v;
      }
    }
  }
  __syncthreads();
  // ---- colour conversion (+ chroma downsampling) into the component planes
  auto px = [&](int r, int x, int& R, int& Gc, int& B) {
    const int off = (int)((base + ((uintptr_t)(y0 + r) * width + x0) * 3) & 15);
    const uint8_t* p = &raw[r * kRawPitch + off + 3 * x];
    R = p[bgr ? 2 : 0];
    Gc = p[1];
    B = p[bgr ? 0 : 2];
  };
  if (SUB == 2) {
    const int qy = t >> 5, qx = t & 31;
    // luma: rows and columns beyond the image replicate the last one
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int R, Gc, B;
        px(min(2 * qy + dy, rmax), min(2 * qx + dx, xmax), R, Gc, B);
        pl[0][2 * qy + dy][2 * qx + dx] = (uint8_t)((19595 * R + 38470 * Gc + 7471 * B + 32768) >> 16);
      }
    // chroma: the last DOWNSAMPLED row is the one replicated; inside it an odd image height repeats
    // the last pixel row
    const int cy = min(y0 / 2 + qy, (height + 1) / 2 - 1);
    const int ra = 2 * cy - y0;
    int cb = 0, cr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int R, Gc, B;
        px(min(ra + dy, rmax), min(2 * qx + dx, xmax), R, Gc, B);
        cb += (-11059 * R - 21709 * Gc + 32768 * B + (128 << 16) + 32767) >> 16;
        cr += (32768 * R - 27439 * Gc - 5329 * B + (128 << 16) + 32767) >> 16;
      }
    const int bias = 1 + (qx & 1);
    pl[1][qy][qx] = (uint8_t)((cb + bias) >> 2);
    pl[2][qy][qx] = (uint8_t)((cr + bias) >> 2);
  } else {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int p = t + 256 * k, r = p >> 6, x = p & 63;
      int R, Gc, B;
      px(min(r, rmax), min(x, xmax), R, Gc, B);
      pl[0][r][x] = (uint8_t)((19595 * R + 38470 * Gc + 7471 * B + 32768) >> 16);
      pl[1][r][x] = (uint8_t)((-11059 * R - 21709 * Gc + 32768 * B + (128 << 16) + 32767) >> 16);
      pl[2][r][x] = (uint8_t)((32768 * R - 27439 * Gc - 5329 * B + (128 << 16) + 32767) >> 16);
    }
  }
  __syncthreads();
  // ---- jpeg_fdct_islow pass 1: one block row per lane
  const int b = t >> 3, l = t & 7;
  if (b < kFwdBlocks) {
    fwd_block<SUB>(b, c, row0, col0);
    const uint2 s = *(const uint2*)&pl[c][row0 + l][col0];
    int d[8], o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = (int)((s.x >> (8 * k)) & 255) - 128;
      d[k + 4] = (int)((s.y >> (8 * k)) & 255) - 128;
    }
    fdct8<0>(d, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) ws[b * 72 + l * 8 + k] = o[k];
  }
  __syncthreads();
}

// pass 2 of jpeg_fdct_islow on column l of block b of ws, then the quantiser of jcdctmgr.c (divisor
// 8 * q, q = column l of the component's table): qv[k] = the quantised coefficient of row k
__device__ __forceinline__ void fwd_pass2_quant(const int* ws, int b, int l, const uint16_t* q, int* qv) {
  int d[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = ws[b * 72 + k * 8 + l];
  fdct8<1>(d, o);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dv = 8 * (int)q[k * 8 + l];
    const int a = (o[k] < 0 ? -o[k] : o[k]) + (dv >> 1);
    const int qq = a >= dv ? a / dv : 0;
    qv[k] = o[k] < 0 ? -qq : qq;
  }
}

template <int SUB>
__global__ void __launch_bounds__(256) jpeg_forward_kernel(const uint8_t* __restrict__ img, JpegFwd j,
                                                           int16_t* __restrict__ coefs) {
  constexpr int ROWS = 8 * SUB;  // pixel rows of the tile
  constexpr int G = SUB == 2 ? 4 : 8;  // MCUs of the tile
  __shared__ __attribute__((aligned(16))) uint8_t raw[16 * kRawPitch];
  __shared__ __attribute__((aligned(16))) uint8_t pl[3][16][64];
  __shared__ int ws[kFwdBlocks * 72];  // pass-1 output
  __shared__ __attribute__((aligned(16))) int16_t outc[kFwdBlocks * 64];
  __shared__ uint16_t qd[3][64];
  const int t = threadIdx.x;
  const int tx = blockIdx.x, my = blockIdx.y;
  if (t < 192) qd[t >> 6][t & 63] = j.qt[t >> 6][t & 63];
  const int b = t >> 3, l = t & 7;
  int c = 0, row0 = 0, col0 = 0;
  fwd_tile_pass1<SUB>(img, j.width, j.height, j.bgr, tx * 64, my * ROWS, raw, pl, ws, c, row0, col0);
  // ---- pass 2: one block column per lane, then quantisation
  if (b < kFwdBlocks) {
    int qv[8];
    fwd_pass2_quant(ws, b, l, qd[c], qv);
#pragma unroll
    for (int k = 0; k < 8; ++k) outc[b * 64 + k * 8 + l] = (int16_t)qv[k];
  }
  __syncthreads();
  // ---- dummy luma blocks of an edge MCU (jccoefct.c compress_data): AC zero, DC of the block
  // before it in the MCU
  if (SUB == 2 && t < G && tx * G + t < j.mcux) {
    for (int k = 1; k < 4; ++k) {
      const int vv = k >> 1, hh = k & 1;
      if (2 * (tx * G + t) + hh >= j.wib0 || 2 * my + vv >= j.hib0) {
        const int pv = k - 1;
        int16_t* blk = &outc[(vv * 8 + 2 * t + hh) * 64];
        const int16_t dc = outc[((pv >> 1) * 8 + 2 * t + (pv & 1)) * 64];
        for (int e = 0; e < 64; ++e) blk[e] = 0;
        blk[0] = dc;
      }
    }
  }
  __syncthreads();
  // ---- 16-B stores; the blocks of one component row are contiguous in [comp][by][bx][64]
  if (b < kFwdBlocks) {
    const int by = SUB == 2 && c == 0 ? 2 * my + (row0 >> 3) : my;
    const int bx = (SUB == 2 && c != 0 ? tx * 4 : tx * 8) + (col0 >> 3);
    if (bx < j.bw[c])
      *(uint4*)(coefs + j.coef_off[c] + ((int64_t)by * j.bw[c] + bx) * 64 + l * 8) = *(const uint4*)&outc[b * 64 + l * 8];
  }
}

// ---------------------------------------------------------------- compress + decompress round trip
// JPEG compression as a corruption (mx_corrupt_jpeg_u8): the pixels a decoder gives back for the file
// the encoder above would write, for a batch of images of one size, without the file and without the
// coefficients ever leaving the workgroup.
//   jpeg_roundtrip_kernel  the forward kernel's tile (64 pixels x one MCU row; blockIdx.z = slot of
//                          the launch's image table) through fwd_tile_pass1 and fwd_pass2_quant; the
//                          lane that quantised column l of a block dequantises it (coef * q) and runs
//                          pass 1 of jpeg_idct_islow on that same column in registers, pass 2 goes by
//                          rows through the LDS words the forward DCT used, and the range-limited
//                          samples are stored to the image's component planes (JpegDev's layout: the
//                          MCU-padded planes jpeg_idct_kernel writes). The dummy blocks of an edge MCU
//                          get whatever the replicated tile gives: no decoder output reads them.
//   jpeg_planes_rgb_kernel jpeg_colour_kernel over the planes of every image of the table.
// The quantisation tables are scaled in the kernel from the image's quality exactly as
// mx_jpeg_encode_info scales them (jpeg_quality_scaling, force_baseline).
constexpr int kRtBatch = 64;  // images per launch: one table of (image, quality) pairs in the arguments

struct JpegRt {
  int32_t width, height, bgr;
  int32_t bw[3];
  int64_t plane_off[3];
  int64_t plane_bytes;  // component planes of one image
  uint8_t base[2][64];  // Annex K tables, natural order
  int32_t image[kRtBatch], quality[kRtBatch];
};

struct JpegRtColour {
  int32_t width, height, bgr, hs, vs;
  int32_t bw[3], dw[3], dh[3];
  int64_t plane_off[3];
  int64_t plane_bytes;
  int32_t image[kRtBatch];
};

template <int SUB>
__global__ void __launch_bounds__(256) jpeg_roundtrip_kernel(const uint8_t* __restrict__ img, JpegRt j,
                                                             uint8_t* __restrict__ planes) {
  constexpr int ROWS = 8 * SUB;
  __shared__ __attribute__((aligned(16))) uint8_t raw[16 * kRawPitch];
  __shared__ __attribute__((aligned(16))) uint8_t pl[3][16][64];
  __shared__ __attribute__((aligned(16))) int ws[kFwdBlocks * 72];
  __shared__ uint16_t qd[2][64];  // luma, chroma
  const int t = threadIdx.x;
  const int tx = blockIdx.x, my = blockIdx.y;
  const int64_t image = j.image[blockIdx.z];
  if (t < 128) {
    const int quality = j.quality[blockIdx.z];
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = ((int)j.base[t >> 6][t & 63] * scale + 50) / 100;
    qd[t >> 6][t & 63] = (uint16_t)(q < 1 ? 1 : (q > 255 ? 255 : q));
  }
  const int b = t >> 3, l = t & 7;
  int c = 0, row0 = 0, col0 = 0;
  fwd_tile_pass1<SUB>(img + image * ((int64_t)j.width * j.height * 3), j.width, j.height, j.bgr, tx * 64, my * ROWS, raw,
                      pl, ws, c, row0, col0);
  int* wsb = &ws[b * 72];
  if (b < kFwdBlocks) {
    // forward pass 2 + quantiser, then DEQUANTIZE and pass 1 of jpeg_idct_islow, all on column l
    const uint16_t* q = qd[c != 0];
    int qv[8];
    fwd_pass2_quant(ws, b, l, q, qv);
    int64_t in[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = (int64_t)qv[r] * q[r * 8 + l];
    idct8(in, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) wsb[r * 8 + l] = (int32_t)descale(o[r], 11);
  }
  __syncthreads();
  if (b < kFwdBlocks) {  // pass 2: row l, descaled by CONST_BITS + PASS1_BITS + 3, range-limited
    int64_t in[8], o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) in[e] = (int64_t)wsb[l * 8 + e];
    idct8(in, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo |= (uint32_t)idct_limit(descale(o[e], 18)) << (8 * e);
      hi |= (uint32_t)idct_limit(descale(o[e + 4], 18)) << (8 * e);
    }
    const int by = SUB == 2 && c == 0 ? 2 * my + (row0 >> 3) : my;
    const int bx = (SUB == 2 && c != 0 ? tx * 4 : tx * 8) + (col0 >> 3);
    const int bwc = sel3(j.bw, c);
    if (bx < bwc) {
      const int64_t off = c == 0 ? j.plane_off[0] : (c == 1 ? j.plane_off[1] : j.plane_off[2]);
      *(uint2*)(planes + image * j.plane_bytes + off + ((int64_t)by * 8 + l) * bwc * 8 + bx * 8) = make_uint2(lo, hi);
    }
  }
}

__global__ void __launch_bounds__(256) jpeg_planes_rgb_kernel(const uint8_t* __restrict__ planes, JpegRtColour j,
                                                              uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t np = (int64_t)j.width * j.height;
  if (i >= np) return;
  const int64_t image = j.image[blockIdx.y];
  const uint8_t* p = planes + image * j.plane_bytes;
  const int x = (int)(i % j.width), y = (int)(i / j.width);
  const int Y = p[j.plane_off[0] + (int64_t)y * j.bw[0] * 8 + x];
  const int cb = chroma(p + j.plane_off[1], (int64_t)j.bw[1] * 8, j.hs, j.vs, j.dw[1], j.dh[1], x, y);
  const int cr = chroma(p + j.plane_off[2], (int64_t)j.bw[2] * 8, j.hs, j.vs, j.dw[2], j.dh[2], x, y);
  int R, G, B;
  ycc_rgb(Y, cb, cr, R, G, B);
  uint8_t* o = out + (image * np + i) * 3;
  o[0] = (uint8_t)(j.bgr ? B : R);
  o[1] = (uint8_t)G;
  o[2] = (uint8_t)(j.bgr ? R : B);
}

// ---------------------------------------------------------------- entropy coder
struct JpegScan {
  int32_t ncomp, mcux, bpm;
  int32_t h[3], v[3], bw[3], first[3];  // first: index of the component's first block inside an MCU
  int64_t coef_off[3];
  int64_t nblk;  // blocks of the scan
};
struct JpegHuff {
  uint32_t dc[3][16], ac[3][256];  // per component: code << 8 | length (0: no code)
};
constexpr int kHuffWords = 3 * 16 + 3 * 256;
constexpr int kMaxBlockBits = 64 * 26 + 27;
constexpr int kChunk = 4096;  // bytes per workgroup of the stuffing passes (16 per lane)

__device__ constexpr int kZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                     12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                     58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// scan-order block s -> component, coefficient offset of the block and of the block whose DC is its
// predictor (-1: none, the first block of the component)
__device__ __forceinline__ void scan_locate(const JpegScan& j, int64_t s, int& c, int64_t& off, int64_t& poff) {
  int64_t m = s / j.bpm;
  const int k = (int)(s - m * j.bpm);
  c = (j.ncomp == 3 && k >= j.first[1]) ? (k >= j.first[2] ? 2 : 1) : 0;
  const int h = sel3(j.h, c), v = sel3(j.v, c), bw = sel3(j.bw, c);
  const int64_t co = c == 0 ? j.coef_off[0] : (c == 1 ? j.coef_off[1] : j.coef_off[2]);
  int kk = k - sel3(j.first, c);
  off = co + (((m / j.mcux) * v + kk / h) * bw + (m % j.mcux) * h + kk % h) * 64;
  if (kk > 0) {
    --kk;
  } else if (m > 0) {
    --m;
    kk = h * v - 1;
  } else {
    poff = -1;
    return;
  }
  poff = co + (((m / j.mcux) * v + kk / h) * bw + (m % j.mcux) * h + kk % h) * 64;
}

struct BitCount {
  uint32_t bits = 0;
  __device__ __forceinline__ void put(uint32_t, int n) { bits += n; }
};

// MSB-first writer into 32-bit words (byte i of the stream is bits 31-8*(i%4).. of word i/4). The
// first and the last word of a block may be shared with its neighbours: atomicOr into the zeroed
// buffer; the words between belong to this block alone.
struct BitEmit {
  uint32_t* words;
  int64_t w, cap;
  uint64_t acc = 0;
  int nacc;
  bool first = true;
  __device__ __forceinline__ void put(uint32_t v, int n) {  // 0 <= n <= 27, nacc < 32
    if (n == 0) return;
    acc |= (uint64_t)v << (64 - nacc - n);
    nacc += n;
    if (nacc >= 32) {
      const uint32_t x = (uint32_t)(acc >> 32);
      if (w < cap) {
        if (first) atomicOr(&words[w], x);
        else words[w] = x;
      }
      first = false;
      ++w;
      acc <<= 32;
      nacc -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nacc > 0 && w < cap) atomicOr(&words[w], (uint32_t)(acc >> 32));
  }
};

// jchuff.c encode_one_block on one block (natural order, 8 x 16 B); false when a value has no code
// (the bits then written stay inside the kMaxBlockBits bound: sizes are clamped to 11 / 10)
template <typename S>
__device__ __forceinline__ bool encode_block(const int16_t* blk, int pred, const uint32_t* dct, const uint32_t* act,
                                             S& s) {
  uint32_t w[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 u = ((const uint4*)blk)[i];
    w[4 * i] = u.x;
    w[4 * i + 1] = u.y;
    w[4 * i + 2] = u.z;
    w[4 * i + 3] = u.w;
  }
  bool ok = true;
  {
    const int d = (int)(int16_t)(w[0] & 0xffff) - pred;
    int nb = 32 - __clz(d < 0 ? -d : d);
    if (nb > 11) {
      ok = false;
      nb = 11;
    }
    const uint32_t e = dct[nb];
    ok = ok && e != 0;
    s.put(((e >> 8) << nb) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << nb) - 1)), (int)(e & 255) + nb);
  }
  int r = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int n = kZig[k];
    const int v = (int)(int16_t)((w[n >> 1] >> ((n & 1) * 16)) & 0xffff);
    if (v == 0) {
      ++r;
    } else {
      if (r > 15) {
        const uint32_t z = act[0xF0];
        ok = ok && z != 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (i < (r >> 4)) s.put(z >> 8, (int)(z & 255));
        r &= 15;
      }
      int nb = 32 - __clz(v < 0 ? -v : v);
      if (nb > 10) {
        ok = false;
        nb = 10;
      }
      const uint32_t e = act[(r << 4) | nb];
      ok = ok && e != 0;
      s.put(((e >> 8) << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1)), (int)(e & 255) + nb);
      r = 0;
    }
  }
  if (r > 0) {
    const uint32_t e = act[0];
    ok = ok && e != 0;
    s.put(e >> 8, (int)(e & 255));
  }
  return ok;
}

// exclusive scan over the N lanes of a workgroup (sh: N words); *total = the sum
template <int N>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < N; o <<= 1) {
    const uint32_t a = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const uint32_t inc = sh[t];
  *total = sh[N - 1];
  __syncthreads();
  return inc - v;
}

__device__ __forceinline__ void load_huff(const JpegHuff& hd, uint32_t* sh) {
  const uint32_t* src = (const uint32_t*)&hd;
  for (int i = threadIdx.x; i < kHuffWords; i += blockDim.x) sh[i] = src[i];
  __syncthreads();
}

// (a) bits of every block + exclusive scan inside the workgroup of 256 blocks
__global__ void __launch_bounds__(256) jpeg_count_kernel(const int16_t* __restrict__ coefs, JpegScan j, JpegHuff hd,
                                                         uint32_t* __restrict__ local, uint32_t* __restrict__ wg_sum,
                                                         int64_t* __restrict__ scal) {
  __shared__ uint32_t huff[kHuffWords];
  __shared__ uint32_t sh[256];
  load_huff(hd, huff);
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bits = 0;
  if (s < j.nblk) {
    int c;
    int64_t off, poff;
    scan_locate(j, s, c, off, poff);
    BitCount bc;
    if (!encode_block(coefs + off, poff < 0 ? 0 : (int)coefs[poff], huff + 16 * c, huff + 48 + 256 * c, bc))
      atomicOr((unsigned long long*)&scal[1], 1ull);
    bits = bc.bits;
  }
  uint32_t total;
  const uint32_t ex = block_excl_scan<256>(bits, sh, &total);
  if (s < j.nblk) local[s] = ex;
  if (threadIdx.x == 0) wg_sum[blockIdx.x] = total;
}

// one workgroup: out[i] = sum of in[0..i), *total = sum of all n
__device__ __forceinline__ int64_t scan_partials(const uint32_t* in, int64_t n, int64_t* out, uint32_t* sh) {
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_excl_scan<1024>(i < n ? in[i] : 0, sh, &total);
    if (i < n) out[i] = carry + ex;
    carry += total;
  }
  return carry;
}

// (b) scal[0] = bits of the scan
__global__ void __launch_bounds__(1024) jpeg_scan_bits_kernel(const uint32_t* __restrict__ wg_sum, int64_t n,
                                                              int64_t* __restrict__ wg_off, int64_t* __restrict__ scal) {
  __shared__ uint32_t sh[1024];
  const int64_t total = scan_partials(wg_sum, n, wg_off, sh);
  if (threadIdx.x == 0) scal[0] = total;
}

// bytes of the unstuffed stream (the last one padded)
__device__ __forceinline__ int64_t stream_bytes(const int64_t* scal) { return (scal[0] + 7) >> 3; }

__global__ void __launch_bounds__(256) jpeg_zero_kernel(uint32_t* __restrict__ words, int64_t cap,
                                                        const int64_t* __restrict__ scal) {
  int64_t n = ((stream_bytes(scal) + 15) >> 4) << 2;  // whole 16-B groups: what the stuffing lanes read
  n = n < cap ? n : cap;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) words[i] = 0;
}

// (c) every block writes its bits at its offset
__global__ void __launch_bounds__(256) jpeg_emit_kernel(const int16_t* __restrict__ coefs, JpegScan j, JpegHuff hd,
                                                        const uint32_t* __restrict__ local,
                                                        const int64_t* __restrict__ wg_off, uint32_t* __restrict__ words,
                                                        int64_t cap) {
  __shared__ uint32_t huff[kHuffWords];
  load_huff(hd, huff);
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= j.nblk) return;
  int c;
  int64_t off, poff;
  scan_locate(j, s, c, off, poff);
  const int64_t pos = wg_off[blockIdx.x] + local[s];
  BitEmit be;
  be.words = words;
  be.cap = cap;
  be.w = pos >> 5;
  be.nacc = (int)(pos & 31);
  encode_block(coefs + off, poff < 0 ? 0 : (int)coefs[poff], huff + 16 * c, huff + 48 + 256 * c, be);
  if (s == j.nblk - 1) {  // flush_bits: ones up to the byte boundary
    const int pad = (8 - (be.nacc & 7)) & 7;
    be.put((1u << pad) - 1, pad);
  }
  be.finish();
}

// the 16 stream bytes of lane `g` (g-th group of 16) and how many are 0xFF; bytes at or past nb are not counted
__device__ __forceinline__ int ff_group(const uint32_t* words, int64_t g, int64_t nb, uint32_t (&w)[4]) {
  int n = 0;
  if (g * 16 < nb) {
    const uint4 u = ((const uint4*)words)[g];
    w[0] = u.x, w[1] = u.y, w[2] = u.z, w[3] = u.w;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      n += (g * 16 + k < nb) && ((w[k >> 2] >> (24 - 8 * (k & 3))) & 255) == 255;
  }
  return n;
}

// (d1) 0xFF bytes per chunk
__global__ void __launch_bounds__(256) jpeg_ff_count_kernel(const uint32_t* __restrict__ words,
                                                            const int64_t* __restrict__ scal,
                                                            uint32_t* __restrict__ wg_ff) {
  __shared__ uint32_t sh[256];
  const int64_t nb = stream_bytes(scal);
  if ((int64_t)blockIdx.x * kChunk >= nb) return;
  uint32_t w[4];
  const int n = ff_group(words, (int64_t)blockIdx.x * 256 + threadIdx.x, nb, w);
  uint32_t total;
  block_excl_scan<256>(n, sh, &total);
  if (threadIdx.x == 0) wg_ff[blockIdx.x] = total;
}

// (d2) chunk offsets; *nbytes = stuffed length, or -1 when a coefficient had no code
__global__ void __launch_bounds__(1024) jpeg_scan_ff_kernel(const uint32_t* __restrict__ wg_ff,
                                                            const int64_t* __restrict__ scal,
                                                            int64_t* __restrict__ wg_ffoff, int64_t* __restrict__ nbytes) {
  __shared__ uint32_t sh[1024];
  const int64_t nb = stream_bytes(scal);
  const int64_t ff = scan_partials(wg_ff, (nb + kChunk - 1) / kChunk, wg_ffoff, sh);
  if (threadIdx.x == 0) *nbytes = scal[1] ? -1 : nb + ff;
}

// (d3) scatter with the stuffed zeros
__global__ void __launch_bounds__(256) jpeg_stuff_kernel(const uint32_t* __restrict__ words,
                                                         const int64_t* __restrict__ scal,
                                                         const int64_t* __restrict__ wg_ffoff, uint8_t* __restrict__ out,
                                                         int64_t out_cap) {
  __shared__ uint32_t sh[256];
  const int64_t nb = stream_bytes(scal);
  if ((int64_t)blockIdx.x * kChunk >= nb) return;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t w[4];
  const int n = ff_group(words, g, nb, w);
  uint32_t total;
  const uint32_t ex = block_excl_scan<256>(n, sh, &total);
  if (g * 16 >= nb) return;
  int64_t pos = g * 16 + wg_ffoff[blockIdx.x] + ex;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (g * 16 + k < nb) {
      const uint32_t b = (w[k >> 2] >> (24 - 8 * (k & 3))) & 255;
      if (pos < out_cap) out[pos] = (uint8_t)b;
      ++pos;
      if (b == 255) {
        if (pos < out_cap) out[pos] = 0;
        ++pos;
      }
    }
  }
}

struct EntropyWs {
  uint32_t *local, *wg_sum, *words, *wg_ff;
  int64_t *wg_off, *scal, *wg_ffoff;
  int64_t nblk, nwg, wcap, nchunk;
  size_t bytes;
};

static EntropyWs entropy_ws(const mx_jpeg_info* info, void* ws, size_t cap) {
  EntropyWs e;
  e.nblk = info->coef_total / 64;
  e.nwg = cdiv(e.nblk, 256);
  e.wcap = cdiv(cdiv(e.nblk * kMaxBlockBits, 8), 16) * 4 + 4;  // whole 16-B groups
  e.nchunk = cdiv(e.wcap * 4, kChunk);
  Carver cv(ws, cap);
  e.local = cv.take<uint32_t>(e.nblk);
  e.wg_sum = cv.take<uint32_t>(e.nwg);
  e.wg_off = cv.take<int64_t>(e.nwg);
  e.scal = cv.take<int64_t>(4);
  e.words = cv.take<uint32_t>(e.wcap);
  e.wg_ff = cv.take<uint32_t>(e.nchunk);
  e.wg_ffoff = cv.take<int64_t>(e.nchunk);
  e.bytes = align_up(cv.off);
  return e;
}

const char* jpeg_enc_check(const mx_jpeg_info* info);  // mx_jpeg.cpp: geometry both coders rely on

}  // namespace mx

extern "C" int mx_jpeg_forward(const uint8_t* img, int bgr, const mx_jpeg_info* info, int16_t* coefs,
                               mx_stream_t stream) {
  MX_CHECK_ARG(img && info && coefs, "jpeg_forward: null argument");
  const char* bad = jpeg_enc_check(info);
  MX_CHECK_ARG(!bad, "jpeg_forward: %s", bad);
  MX_CHECK_ARG(((uintptr_t)coefs & 15) == 0, "jpeg_forward: coefficients must be 16-byte aligned");
  const bool c11 = info->ncomp == 3 && info->h[1] == 1 && info->v[1] == 1 && info->h[2] == 1 && info->v[2] == 1;
  const int sub = c11 && info->h[0] == 2 && info->v[0] == 2 ? 2 : (c11 && info->h[0] == 1 && info->v[0] == 1 ? 1 : 0);
  if (!sub) {
    set_error("jpeg_forward: 3-component 4:4:4 or 4:2:0 only");
    return MX_EUNSUPPORTED;
  }
  MX_CHECK_ARG(info->mcux == cdiv(info->width, 8 * sub) && info->mcuy == cdiv(info->height, 8 * sub),
               "jpeg_forward: MCU counts do not match the image size");
  JpegFwd j;
  j.width = info->width;
  j.height = info->height;
  j.mcux = info->mcux;
  j.bgr = bgr ? 1 : 0;
  j.wib0 = (int)cdiv(info->width, 8);
  j.hib0 = (int)cdiv(info->height, 8);
  for (int c = 0; c < 3; ++c) {
    j.bw[c] = info->bw[c];
    j.coef_off[c] = info->coef_off[c];
    for (int k = 0; k < 64; ++k) {
      MX_CHECK_ARG(info->qt[info->tq[c]][k] >= 1, "jpeg_forward: zero quantiser");
      j.qt[c][k] = info->qt[info->tq[c]][k];
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(info->mcux, sub == 2 ? 4 : 8), (unsigned)info->mcuy);
  if (sub == 2) jpeg_forward_kernel<2><<<grid, 256, 0, st>>>(img, j, coefs);
  else jpeg_forward_kernel<1><<<grid, 256, 0, st>>>(img, j, coefs);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

namespace mx {
const uint8_t* jpeg_base_quant(int t);  // mx_jpeg.cpp

// geometry of a B x H x W round trip (the layout mx_jpeg_encode_info gives one image); nullptr when fine
static const char* roundtrip_geom(int64_t B, int64_t H, int64_t W, int subsampling, mx_jpeg_info* info, JpegDev* j,
                                  int64_t* plane_bytes) {
  if (B < 0 || B > INT32_MAX || H < 1 || W < 1) return "bad shape";
  if (subsampling != 0 && subsampling != 2) return "subsampling 0 (4:4:4) or 2 (4:2:0) only";
  if (H > 65535 || W > 65535 || H * W > ((int64_t)1 << 28)) return "image larger than 65535 a side or 2^28 pixels";
  if (mx_jpeg_encode_info((int)W, (int)H, 50, subsampling, info) != MX_OK) return "no encoder geometry for this size";
  to_dev(info, j, plane_bytes);
  return nullptr;
}
}  // namespace mx

extern "C" size_t mx_corrupt_jpeg_workspace(int64_t B, int64_t H, int64_t W, int subsampling) {
  mx_jpeg_info info;
  JpegDev j;
  int64_t per = 0;
  if (roundtrip_geom(B, H, W, subsampling, &info, &j, &per)) return 0;
  return (size_t)(per * B);
}

extern "C" int mx_corrupt_jpeg_u8(const uint8_t* img, int64_t B, int64_t H, int64_t W, const int32_t* quality_host,
                                  int subsampling, int bgr, void* ws, size_t ws_bytes, uint8_t* out, mx_stream_t stream) {
  MX_CHECK_ARG(img && quality_host && out, "corrupt_jpeg_u8: null argument");
  mx_jpeg_info info;
  JpegDev d;
  int64_t per = 0;
  const char* bad = roundtrip_geom(B, H, W, subsampling, &info, &d, &per);
  MX_CHECK_ARG(!bad, "corrupt_jpeg_u8: %s", bad);
  const int64_t img_bytes = H * W * 3;
  MX_CHECK_ARG(out != img, "corrupt_jpeg_u8: out must not be img");
  MX_CHECK_ARG((uintptr_t)out + B * img_bytes <= (uintptr_t)img || (uintptr_t)img + B * img_bytes <= (uintptr_t)out,
               "corrupt_jpeg_u8: out must not overlap img");
  int64_t active = 0;
  for (int64_t b = 0; b < B; ++b) {
    MX_CHECK_ARG(quality_host[b] >= 0 && quality_host[b] <= 100,
                 "corrupt_jpeg_u8: quality %d of image %lld is not 1..100 (or 0: leave the image alone)",
                 (int)quality_host[b], (long long)b);
    active += quality_host[b] != 0;
  }
  if (active == 0) return MX_OK;
  MX_CHECK_ARG(ws && (int64_t)ws_bytes >= per * B, "corrupt_jpeg_u8: workspace of %lld bytes required",
               (long long)(per * B));
  MX_CHECK_ARG(((uintptr_t)ws & 7) == 0, "corrupt_jpeg_u8: workspace must be 8-byte aligned");
  const int sub = subsampling == 2 ? 2 : 1;
  JpegRt j = {};
  JpegRtColour k = {};
  j.width = k.width = (int32_t)W;
  j.height = k.height = (int32_t)H;
  j.bgr = k.bgr = bgr ? 1 : 0;
  j.plane_bytes = k.plane_bytes = per;
  k.hs = d.hmax / d.h[1];
  k.vs = d.vmax / d.v[1];
  for (int c = 0; c < 3; ++c) {
    j.bw[c] = k.bw[c] = d.bw[c];
    j.plane_off[c] = k.plane_off[c] = d.plane_off[c];
    k.dw[c] = d.dw[c];
    k.dh[c] = d.dh[c];
  }
  for (int t = 0; t < 2; ++t)
    for (int e = 0; e < 64; ++e) j.base[t][e] = jpeg_base_quant(t)[e];
  hipStream_t st = (hipStream_t)stream;
  int64_t b = 0;
  while (b < B) {
    int n = 0;
    for (; b < B && n < kRtBatch; ++b)
      if (quality_host[b] != 0) {
        j.image[n] = k.image[n] = (int32_t)b;
        j.quality[n] = quality_host[b];
        ++n;
      }
    if (n == 0) break;
    const dim3 grid((unsigned)cdiv(info.mcux, sub == 2 ? 4 : 8), (unsigned)info.mcuy, (unsigned)n);
    if (sub == 2) jpeg_roundtrip_kernel<2><<<grid, 256, 0, st>>>(img, j, (uint8_t*)ws);
    else jpeg_roundtrip_kernel<1><<<grid, 256, 0, st>>>(img, j, (uint8_t*)ws);
    MX_LAUNCH_CHECK();
    jpeg_planes_rgb_kernel<<<dim3((unsigned)cdiv(W * H, 256), (unsigned)n), 256, 0, st>>>((const uint8_t*)ws, k, out);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

extern "C" size_t mx_jpeg_entropy_workspace(const mx_jpeg_info* info) {
  if (jpeg_enc_check(info)) return 0;
  return entropy_ws(info, nullptr, 0).bytes;
}

extern "C" int mx_jpeg_entropy(const int16_t* coefs, const mx_jpeg_info* info, void* ws, size_t ws_bytes, uint8_t* out,
                               int64_t out_cap, int64_t* nbytes, mx_stream_t stream) {
  MX_CHECK_ARG(coefs && info && ws && out && nbytes && out_cap >= 0, "jpeg_entropy: null argument");
  const char* bad = jpeg_enc_check(info);
  MX_CHECK_ARG(!bad, "jpeg_entropy: %s", bad);
  MX_CHECK_ARG(((uintptr_t)coefs & 15) == 0 && ((uintptr_t)ws & 255) == 0,
               "jpeg_entropy: coefficients must be 16-byte and the workspace 256-byte aligned");
  if (info->restart_interval != 0) {
    set_error("jpeg_entropy: restart intervals are not supported");
    return MX_EUNSUPPORTED;
  }
  const EntropyWs e = entropy_ws(info, ws, ws_bytes);
  MX_CHECK_ARG(e.bytes <= ws_bytes, "jpeg_entropy: workspace of %lld bytes required", (long long)e.bytes);
  JpegScan j;
  JpegHuff hd;
  j.ncomp = info->ncomp;
  j.mcux = info->mcux;
  j.nblk = e.nblk;
  j.bpm = 0;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < info->ncomp;
    j.h[c] = on ? info->h[c] : 1;
    j.v[c] = on ? info->v[c] : 1;
    j.bw[c] = on ? info->bw[c] : 0;
    j.coef_off[c] = on ? info->coef_off[c] : 0;
    j.first[c] = j.bpm;
    if (on) j.bpm += info->h[c] * info->v[c];
    uint32_t tab[256];
    const int cc = on ? c : 0;
    MX_CHECK_ARG(jpeg_enc_table(info->hbits[info->td[cc]], info->hval[info->td[cc]], tab), "jpeg_entropy: bad DC Huffman table");
    for (int k = 0; k < 16; ++k) hd.dc[c][k] = tab[k];
    MX_CHECK_ARG(jpeg_enc_table(info->hbits[4 + info->ta[cc]], info->hval[4 + info->ta[cc]], hd.ac[c]),
                 "jpeg_entropy: bad AC Huffman table");
  }
  hipStream_t st = (hipStream_t)stream;
  MX_HIP(hipMemsetAsync(e.scal, 0, 4 * sizeof(int64_t), st));
  jpeg_count_kernel<<<(unsigned)e.nwg, 256, 0, st>>>(coefs, j, hd, e.local, e.wg_sum, e.scal);
  MX_LAUNCH_CHECK();
  jpeg_scan_bits_kernel<<<1, 1024, 0, st>>>(e.wg_sum, e.nwg, e.wg_off, e.scal);
  MX_LAUNCH_CHECK();
  jpeg_zero_kernel<<<(unsigned)(e.wcap / 256 < 2048 ? e.wcap / 256 + 1 : 2048), 256, 0, st>>>(e.words, e.wcap, e.scal);
  MX_LAUNCH_CHECK();
  jpeg_emit_kernel<<<(unsigned)e.nwg, 256, 0, st>>>(coefs, j, hd, e.local, e.wg_off, e.words, e.wcap);
  MX_LAUNCH_CHECK();
  jpeg_ff_count_kernel<<<(unsigned)e.nchunk, 256, 0, st>>>(e.words, e.scal, e.wg_ff);
  MX_LAUNCH_CHECK();
  jpeg_scan_ff_kernel<<<1, 1024, 0, st>>>(e.wg_ff, e.scal, e.wg_ffoff, nbytes);
  MX_LAUNCH_CHECK();
  jpeg_stuff_kernel<<<(unsigned)e.nchunk, 256, 0, st>>>(e.words, e.scal, e.wg_ffoff, out, out_cap);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

// ================================================================================================
// Entropy decoder, device half (mx_jpeg_entropy_decode; the walk itself is mx_jpeg_walk.h, shared with
// the serial host restatement mx_jpeg_decode_coefs_chunked in mx_jpeg.cpp). A Huffman stream
// re-synchronises, so fixed-size subsequences are decoded speculatively and a fix-up iteration gives
// every lane its true start state: the result is the sequential decoder's, bit for bit.
//   jd_mark / jd_scan_chunks / jd_compact   markers and FF 00 pairs per 4-KiB chunk (16 B per lane, the
//                         neighbours of a lane's bytes read across lane and chunk boundaries), scans,
//                         compaction to the unstuffed stream + the restart segments' first bytes;
//   jd_seg                subsequences per segment, scan;
//   jd_sync (pass 0)      every lane walks its subsequence from the assumed state, then the workgroup
//                         iterates with barriers: lane i + 1 re-walks from lane i's exit state until no
//                         input changes;
//   jd_sync (pass p > 0)  the same from the previous workgroup's last exit state; exits at once when
//                         pass p - 1 changed no workgroup's last exit state (a device flag). After pass
//                         p the first p + 1 workgroups are final. No workgroup waits on another;
//   jd_place              scan of the blocks completed per lane;
//   jd_write              every lane walks from its true state: AC values, DC differences, status bits;
//   jd_dc<0> / jd_dc_carry / jd_dc<1>   per-component DC prefix sums (32-bit, reset at restart segments).
// Integer only. Every launch is sized on the host from the worst case and exits on the device totals.
// ================================================================================================
namespace mx {

int jpeg_dec_subseq();  // mx_jpeg.cpp: the process setting (mx_jpeg_entropy_decode_set_subseq)

struct JdWs {
  int64_t *scal;  // [0] clean bytes, [1] restart markers found, [2] subsequences
  JdHuff* tabs;
  uint32_t *chunk_last, *chunk_rst, *chunk_pre, *chunk_post, *chunk_live, *chunk_rstoff;
  int64_t* chunk_off;
  uint32_t* clean;
  int64_t *seg_start, *sub_base, *P;
  uint32_t *gexit, *glastin, *gcnt, *flags;
  int32_t *tile_f, *tile_v, *carry;
  int64_t nchunk, maxsubs, nwg, ntile[3], ntiles;
  size_t bytes;
};

static JdWs jd_ws(const mx_jpeg_info* info, const JdGeom& g, int64_t nbytes, void* ws, size_t cap) {
  JdWs e;
  e.nchunk = cdiv(nbytes + 15, kJdChunk);  // chunks are cut at 16-B aligned addresses: up to 15 bytes of lead-in
  e.maxsubs = nbytes * 8 / g.subseq + g.nseg + 1;
  e.nwg = cdiv(e.maxsubs, kJdLanes);
  e.ntiles = 0;
  for (int c = 0; c < 3; ++c) {
    e.ntile[c] = c < g.ncomp ? cdiv((int64_t)info->bw[c] * info->bh[c], 256) : 0;
    e.ntiles += e.ntile[c];
  }
  Carver cv(ws, cap);
  e.scal = cv.take<int64_t>(8);
  e.tabs = cv.take<JdHuff>(kJdTables);
  e.chunk_last = cv.take<uint32_t>(e.nchunk);
  e.chunk_rst = cv.take<uint32_t>(e.nchunk);
  e.chunk_pre = cv.take<uint32_t>(e.nchunk);
  e.chunk_post = cv.take<uint32_t>(e.nchunk);
  e.chunk_live = cv.take<uint32_t>(e.nchunk);
  e.chunk_rstoff = cv.take<uint32_t>(e.nchunk);
  e.chunk_off = cv.take<int64_t>(e.nchunk);
  e.clean = cv.take<uint32_t>((nbytes + 16) / 4 + 1);  // + the word a peek reads past the last bit
  e.seg_start = cv.take<int64_t>((int64_t)g.nseg + 1);
  e.sub_base = cv.take<int64_t>((int64_t)g.nseg + 1);
  e.P = cv.take<int64_t>(e.maxsubs + 1);
  e.gexit = cv.take<uint32_t>(e.maxsubs);
  e.glastin = cv.take<uint32_t>(e.maxsubs);
  e.gcnt = cv.take<uint32_t>(e.maxsubs);
  e.flags = cv.take<uint32_t>(e.nwg + 1);
  e.tile_f = cv.take<int32_t>(e.ntiles);
  e.tile_v = cv.take<int32_t>(e.ntiles);
  e.carry = cv.take<int32_t>(e.ntiles);
  e.bytes = align_up(cv.off);
  return e;
}

// exclusive scan over the N lanes of a workgroup with an associative op (sh: N elements); *total = all
template <int N, typename T, typename Op>
__device__ __forceinline__ T block_excl_scan_op(T v, T identity, T* sh, T* total, Op op) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < N; o <<= 1) {
    const T a = t >= o ? sh[t - o] : identity;
    __syncthreads();
    sh[t] = op(a, sh[t]);
    __syncthreads();
  }
  const T ex = t > 0 ? sh[t - 1] : identity;
  *total = sh[N - 1];
  __syncthreads();
  return ex;
}
struct OpAdd64 {
  __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return a + b; }
};
struct OpMax32 {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
struct OpMax64 {
  __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};

// The 16 scan bytes of lane `lane` of chunk `chunk` with their classes. Chunks and lanes are cut at
// 16-B aligned addresses (the scan starts `mis` bytes into the first group). cls[k] < 0: byte outside
// the scan. Returns the scan index of byte 0 of the group.
__device__ __forceinline__ int64_t jd_group(const uint8_t* scan, int64_t n, int mis, int64_t chunk, int lane,
                                            uint8_t (&b)[16], int (&cls)[16]) {
  const int64_t i0 = chunk * kJdChunk + (int64_t)lane * 16 - mis;
  if (i0 >= 0 && i0 + 16 <= n) {
    *(uint4*)b = *(const uint4*)(scan + i0);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = (i0 + k >= 0 && i0 + k < n) ? scan[i0 + k] : 0;
  }
  const int prev = (i0 - 1 >= 0 && i0 - 1 < n) ? (int)scan[i0 - 1] : -1;
  const int next = (i0 + 16 >= 0 && i0 + 16 < n) ? (int)scan[i0 + 16] : -1;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t i = i0 + k;
    const int p = k > 0 ? (i - 1 >= 0 ? (int)b[k - 1] : -1) : prev;
    const int x = k < 15 ? (i + 1 < n ? (int)b[k + 1] : -1) : next;
    cls[k] = (i >= 0 && i < n) ? jd_classify(p, b[k], x) : -1;
  }
  return i0;
}

// last marker of the lane's bytes: (index in the chunk + 1) * 2 + (it is an RSTn), 0 for none
__device__ __forceinline__ uint32_t jd_last_marker(const int (&cls)[16], int lane) {
  uint32_t last = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (cls[k] >= 0 && (cls[k] & kJdMarker)) last = (uint32_t)(lane * 16 + k + 1) * 2 + ((cls[k] & kJdRst) ? 1 : 0);
  return last;
}

// (1a) per chunk: its last marker, its RSTn count, the data bytes before its first marker (kept only if
// the chunk starts inside live data) and the data bytes kept whatever came before
__global__ void __launch_bounds__(256) jd_mark_kernel(const uint8_t* __restrict__ scan, int64_t n, int mis, JdWs e) {
  __shared__ uint32_t sh[256];
  __attribute__((aligned(16))) uint8_t b[16];
  int cls[16];
  jd_group(scan, n, mis, blockIdx.x, threadIdx.x, b, cls);
  const uint32_t mine = jd_last_marker(cls, threadIdx.x);
  uint32_t last;
  const uint32_t before = block_excl_scan_op<256>(mine, 0u, sh, &last, OpMax32());
  int state = before == 0 ? -1 : (int)(before & 1);  // -1: no marker yet in this chunk
  uint32_t pre = 0, post = 0, rst = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (cls[k] < 0) continue;
    if (cls[k] & kJdMarker) {
      state = (cls[k] & kJdRst) ? 1 : 0;
      rst += state;
    } else if (!(cls[k] & kJdDrop)) {
      pre += state < 0;
      post += state > 0;
    }
  }
  uint32_t tpre, tpost, trst;
  block_excl_scan<256>(pre, sh, &tpre);
  block_excl_scan<256>(post, sh, &tpost);
  block_excl_scan<256>(rst, sh, &trst);
  if (threadIdx.x == 0) {
    e.chunk_last[blockIdx.x] = last;
    e.chunk_pre[blockIdx.x] = tpre;
    e.chunk_post[blockIdx.x] = tpost;
    e.chunk_rst[blockIdx.x] = trst;
  }
}

// (1b) one workgroup: whether each chunk starts in live data, its first clean byte, its first RSTn's
// number; the totals; the starts of the segments no marker opens
__global__ void __launch_bounds__(1024) jd_scan_chunks_kernel(JdWs e, int64_t nchunk, int nseg, int32_t* status) {
  __shared__ int64_t sh[1024];
  int64_t c_last = 0, c_off = 0, c_rst = 0;  // carries: last marker (chunk * 2^14 + in-chunk code), sums
  for (int64_t base = 0; base < nchunk; base += 1024) {
    const int64_t c = base + threadIdx.x;
    const bool on = c < nchunk;
    const uint32_t lm = on ? e.chunk_last[c] : 0;
    int64_t tot;
    int64_t before = block_excl_scan_op<1024>(lm ? (c << 14) + lm : (int64_t)0, (int64_t)0, sh, &tot, OpMax64());
    before = before > c_last ? before : c_last;
    c_last = tot > c_last ? tot : c_last;
    const bool live = before == 0 || (before & 1);
    const int64_t keep = on ? (int64_t)e.chunk_post[c] + (live ? e.chunk_pre[c] : 0) : 0;
    const int64_t off = block_excl_scan_op<1024>(keep, (int64_t)0, sh, &tot, OpAdd64());
    if (on) {
      e.chunk_live[c] = live;
      e.chunk_off[c] = c_off + off;
    }
    c_off += tot;
    const int64_t ro = block_excl_scan_op<1024>(on ? (int64_t)e.chunk_rst[c] : 0, (int64_t)0, sh, &tot, OpAdd64());
    if (on) e.chunk_rstoff[c] = (uint32_t)(c_rst + ro);
    c_rst += tot;
  }
  if (threadIdx.x == 0) {
    e.scal[0] = c_off;
    e.scal[1] = c_rst;
    e.seg_start[0] = 0;
    if (c_rst != nseg - 1) atomicOr(status, MX_JPEG_ST_RESTART);
  }
  const int64_t first = (c_rst < nseg - 1 ? c_rst : nseg - 1) + 1;
  for (int64_t j = first + threadIdx.x; j <= nseg; j += 1024) e.seg_start[j] = c_off;
}

// (1c) the clean stream and the segment starts
__global__ void __launch_bounds__(256) jd_compact_kernel(const uint8_t* __restrict__ scan, int64_t n, int mis, JdWs e,
                                                         int nseg) {
  __shared__ uint32_t sh[256];
  __attribute__((aligned(16))) uint8_t b[16];
  int cls[16];
  jd_group(scan, n, mis, blockIdx.x, threadIdx.x, b, cls);
  const uint32_t mine = jd_last_marker(cls, threadIdx.x);
  uint32_t last;
  const uint32_t before = block_excl_scan_op<256>(mine, 0u, sh, &last, OpMax32());
  const int state0 = before == 0 ? (int)e.chunk_live[blockIdx.x] : (int)(before & 1);
  int state = state0;
  uint32_t keep = 0, rst = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (cls[k] < 0) continue;
    if (cls[k] & kJdMarker) {
      state = (cls[k] & kJdRst) ? 1 : 0;
      rst += state;
    } else if (!(cls[k] & kJdDrop)) {
      keep += state;
    }
  }
  uint32_t tot;
  const uint32_t kex = block_excl_scan<256>(keep, sh, &tot);
  const uint32_t rex = block_excl_scan<256>(rst, sh, &tot);
  int64_t pos = e.chunk_off[blockIdx.x] + kex;
  int64_t r = (int64_t)e.chunk_rstoff[blockIdx.x] + rex;
  const int64_t nclean = e.scal[0];
  uint8_t* clean = (uint8_t*)e.clean;
  state = state0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (cls[k] < 0) continue;
    if (cls[k] & kJdMarker) {
      state = (cls[k] & kJdRst) ? 1 : 0;
      if (state) {
        ++r;  // this marker opens segment r
        if (r < nseg) e.seg_start[r] = pos;
      }
    } else if (!(cls[k] & kJdDrop) && state) {
      if (pos < nclean) clean[pos] = b[k];
      ++pos;
    }
  }
}

// (1d) one workgroup: subsequences of every segment, their scan; an empty segment is a short one
__global__ void __launch_bounds__(1024) jd_seg_kernel(JdWs e, int nseg, int subseq, int32_t* status) {
  __shared__ int64_t sh[1024];
  int64_t carry = 0;
  for (int64_t base = 0; base < nseg; base += 1024) {
    const int64_t j = base + threadIdx.x;
    int64_t ns = 0;
    if (j < nseg) {
      const int64_t bits = (e.seg_start[j + 1] - e.seg_start[j]) * 8;
      if (bits <= 0) atomicOr(status, MX_JPEG_ST_SHORT);
      ns = bits > 0 ? (bits + subseq - 1) / subseq : 0;
    }
    int64_t tot;
    const int64_t ex = block_excl_scan_op<1024>(ns, (int64_t)0, sh, &tot, OpAdd64());
    if (j < nseg) e.sub_base[j] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    e.sub_base[nseg] = carry;
    e.scal[2] = carry;
  }
}

__device__ __forceinline__ void jd_load_tabs(const JdHuff* tabs, uint32_t* sh) {
  const uint32_t* src = (const uint32_t*)tabs;
  for (int i = threadIdx.x; i < kJdHuffWords; i += blockDim.x) sh[i] = src[i];
  __syncthreads();
}

// one component's two tables per launch: a kernel argument holds at most 4 KiB
struct JdHuffPair {
  JdHuff t[2];
};
__global__ void __launch_bounds__(256) jd_tables_kernel(JdHuffPair p, JdHuff* __restrict__ dst) {
  const uint32_t* src = (const uint32_t*)&p;
  uint32_t* d = (uint32_t*)dst;
  for (int i = threadIdx.x; i < (int)(sizeof(JdHuffPair) / 4); i += 256) d[i] = src[i];
}

// (2) + (3) speculative walk (pass 0) and synchronisation
__global__ void __launch_bounds__(kJdLanes) jd_sync_kernel(JdWs e, JdGeom g, int pass) {
  __shared__ uint32_t huff[kJdHuffWords];
  __shared__ uint32_t sh_exit[kJdLanes];
  const int64_t total = e.scal[2];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kJdLanes + t;
  if ((int64_t)blockIdx.x * kJdLanes >= total) return;
  if (pass > 0 && ((int)blockIdx.x < pass || e.flags[pass - 1] == 0)) return;
  jd_load_tabs(e.tabs, huff);
  const JdHuff* tabs = (const JdHuff*)huff;
  const uint32_t* words = e.clean;
  const bool valid = i < total;
  JdLane l;
  uint32_t ex = 0, cnt = 0, lastin = 0;
  if (valid) {
    l = jd_lane(g, e.seg_start, e.sub_base, i);
    if (pass == 0) {
      ex = jd_walk(words, tabs, g, jd_unpack(0, l.boundary), l.limit, l.end, &cnt);
    } else {
      ex = e.gexit[i];
      cnt = e.gcnt[i];
      lastin = e.glastin[i];
    }
  }
  const uint32_t ex0 = ex;
  // the previous workgroup's last exit state: unknown in pass 0 (the assumed state stays), and read
  // once in later passes (a value of this pass or of the one before; flags[] sends a further pass
  // whenever one changed)
  const uint32_t head = (pass == 0 || i == 0 || !valid) ? lastin : e.gexit[i - 1];
  sh_exit[t] = ex;
  __syncthreads();
  bool dirty = pass == 0;
  for (int round = 0; round <= kJdLanes; ++round) {
    uint32_t in = lastin;
    if (valid) in = l.q == 0 ? 0u : (t == 0 ? head : sh_exit[t - 1]);
    const bool changed = valid && in != lastin;
    __syncthreads();
    if (changed) {
      lastin = in;
      if (in == kJdEnd) {
        ex = kJdEnd;
        cnt = 0;
      } else {
        ex = jd_walk(words, tabs, g, jd_unpack(in, l.boundary), l.limit, l.end, &cnt);
      }
      sh_exit[t] = ex;
      dirty = true;
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (valid && dirty) {
    e.gexit[i] = ex;
    e.gcnt[i] = cnt;
    e.glastin[i] = lastin;
  }
  if (pass == 0) {
    if (blockIdx.x == 0 && t == 0) e.flags[0] = total > kJdLanes;
  } else if (t == kJdLanes - 1 && valid && ex != ex0) {
    e.flags[pass] = 1;
  }
}

// (4) one workgroup: P[i] = blocks completed by the lanes before lane i
__global__ void __launch_bounds__(1024) jd_place_kernel(JdWs e) {
  __shared__ int64_t sh[1024];
  const int64_t total = e.scal[2];
  int64_t carry = 0;
  for (int64_t base = 0; base < total; base += 1024) {
    const int64_t i = base + threadIdx.x;
    int64_t tot;
    const int64_t ex = block_excl_scan_op<1024>(i < total ? (int64_t)e.gcnt[i] : 0, (int64_t)0, sh, &tot, OpAdd64());
    if (i < total) e.P[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) e.P[total] = carry;
}

// (5) the true walk of every lane, storing
__global__ void __launch_bounds__(kJdLanes) jd_write_kernel(JdWs e, JdGeom g, int16_t* __restrict__ coefs, int32_t* status) {
  __shared__ uint32_t huff[kJdHuffWords];
  const int64_t total = e.scal[2];
  if ((int64_t)blockIdx.x * kJdLanes >= total) return;
  jd_load_tabs(e.tabs, huff);
  const int64_t i = (int64_t)blockIdx.x * kJdLanes + threadIdx.x;
  if (i >= total) return;
  const JdLane l = jd_lane(g, e.seg_start, e.sub_base, i);
  const uint32_t in = l.q == 0 ? 0u : e.gexit[i - 1];
  const int err = jd_walk_store(e.clean, (const JdHuff*)huff, g, jd_unpack(in, l.boundary), in == kJdEnd, l.limit, l.end,
                                e.P[i] - e.P[e.sub_base[l.seg]], l.quota, l.seg_first, l.last, coefs);
  if (err) atomicOr(status, err);
}

// (6) DC prediction. Tiles of 256 scan-order blocks of one component; MODE 0: the tile's (reset seen,
// sum since it) pair; MODE 1: the running sums with the carry of the tiles before, truncated to int16
template <int MODE>
__global__ void __launch_bounds__(256) jd_dc_kernel(JdWs e, JdGeom g, int16_t* __restrict__ coefs) {
  __shared__ JdSeg sh[256];
  int64_t tile = blockIdx.x;
  int c = 0;
  while (c < 2 && tile >= e.ntile[c]) tile -= e.ntile[c++];
  const int64_t ne = (int64_t)g.bw[c] * (g.nblk / g.bpm / g.mcux) * g.v[c];
  const int64_t el = tile * 256 + threadIdx.x;
  JdSeg x{0, 0};
  int64_t off = 0;
  if (el < ne) {
    int reset;
    off = jd_dc_off(g, c, el, &reset);
    x.f = reset;
    x.v = coefs[off];
  }
  const int t = threadIdx.x;
  sh[t] = x;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < 256; o <<= 1) {
    JdSeg a{0, 0};
    if (t >= o) a = sh[t - o];
    __syncthreads();
    if (t >= o) sh[t] = jd_seg_combine(a, sh[t]);
    __syncthreads();
  }
  const JdSeg inc = sh[t];
  if (MODE == 0) {
    if (t == 255) {
      e.tile_f[blockIdx.x] = inc.f;
      e.tile_v[blockIdx.x] = inc.v;
    }
  } else if (el < ne) {
    const JdSeg r = jd_seg_combine(JdSeg{0, e.carry[blockIdx.x]}, inc);
    coefs[off] = (int16_t)r.v;
  }
}

// one workgroup: carry[t] = the running sum entering tile t
__global__ void __launch_bounds__(1024) jd_dc_carry_kernel(JdWs e, int64_t ntiles) {
  __shared__ JdSeg sh[1024];
  const int t = threadIdx.x;
  JdSeg run{0, 0};
  for (int64_t base = 0; base < ntiles; base += 1024) {
    const int64_t i = base + t;
    JdSeg x{0, 0};
    if (i < ntiles) x = JdSeg{e.tile_f[i], e.tile_v[i]};
    sh[t] = x;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < 1024; o <<= 1) {
      JdSeg a{0, 0};
      if (t >= o) a = sh[t - o];
      __syncthreads();
      if (t >= o) sh[t] = jd_seg_combine(a, sh[t]);
      __syncthreads();
    }
    JdSeg before = run;
    if (t > 0) before = jd_seg_combine(run, sh[t - 1]);
    if (i < ntiles) e.carry[i] = before.v;
    run = jd_seg_combine(run, sh[1023]);
    __syncthreads();
  }
}

static const char* jd_prepare(const mx_jpeg_info* info, int64_t nbytes, JdGeom* g) {
  if (!info) return "null info";
  if (nbytes <= 0 || nbytes >= ((int64_t)1 << 31)) return "nbytes must be 1 .. 2^31 - 1";
  return jpeg_dec_geom(info, jpeg_dec_subseq(), g);
}

}  // namespace mx

extern "C" size_t mx_jpeg_entropy_decode_workspace(const mx_jpeg_info* info, int64_t nbytes) {
  JdGeom g;
  if (jd_prepare(info, nbytes, &g)) return 0;
  return jd_ws(info, g, nbytes, nullptr, 0).bytes;
}

extern "C" int mx_jpeg_entropy_decode(const uint8_t* scan, int64_t nbytes, const mx_jpeg_info* info, void* ws,
                                      size_t ws_bytes, int16_t* coefs, int32_t* status, mx_stream_t stream) {
  MX_CHECK_ARG(scan && info && ws && coefs && status, "jpeg_entropy_decode: null argument");
  JdGeom g;
  const char* bad = jd_prepare(info, nbytes, &g);
  MX_CHECK_ARG(!bad, "jpeg_entropy_decode: %s", bad);
  MX_CHECK_ARG(((uintptr_t)coefs & 15) == 0 && ((uintptr_t)ws & 255) == 0 && ((uintptr_t)status & 3) == 0,
               "jpeg_entropy_decode: coefficients must be 16-byte, the workspace 256-byte and the status 4-byte aligned");
  const JdWs e = jd_ws(info, g, nbytes, ws, ws_bytes);
  MX_CHECK_ARG(e.bytes <= ws_bytes, "jpeg_entropy_decode: workspace of %lld bytes required", (long long)e.bytes);
  JdHuff tabs[kJdTables];
  MX_CHECK_ARG(jpeg_dec_tables(info, tabs), "jpeg_entropy_decode: bad Huffman table");
  hipStream_t st = (hipStream_t)stream;
  const int mis = (int)((uintptr_t)scan & 15);
  const int64_t nchunk = cdiv(nbytes + mis, kJdChunk);
  MX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  MX_HIP(hipMemsetAsync(e.flags, 0, sizeof(uint32_t) * (size_t)(e.nwg + 1), st));
  MX_HIP(hipMemsetAsync(coefs, 0, sizeof(int16_t) * (size_t)info->coef_total, st));
  for (int c = 0; c < 3; ++c) {
    JdHuffPair p;
    p.t[0] = tabs[2 * c];
    p.t[1] = tabs[2 * c + 1];
    jd_tables_kernel<<<1, 256, 0, st>>>(p, e.tabs + 2 * c);
    MX_LAUNCH_CHECK();
  }
  jd_mark_kernel<<<(unsigned)nchunk, 256, 0, st>>>(scan, nbytes, mis, e);
  MX_LAUNCH_CHECK();
  jd_scan_chunks_kernel<<<1, 1024, 0, st>>>(e, nchunk, g.nseg, status);
  MX_LAUNCH_CHECK();
  jd_compact_kernel<<<(unsigned)nchunk, 256, 0, st>>>(scan, nbytes, mis, e, g.nseg);
  MX_LAUNCH_CHECK();
  jd_seg_kernel<<<1, 1024, 0, st>>>(e, g.nseg, g.subseq, status);
  MX_LAUNCH_CHECK();
  for (int64_t pass = 0; pass < e.nwg; ++pass) {
    jd_sync_kernel<<<(unsigned)e.nwg, kJdLanes, 0, st>>>(e, g, (int)pass);
    MX_LAUNCH_CHECK();
  }
  jd_place_kernel<<<1, 1024, 0, st>>>(e);
  MX_LAUNCH_CHECK();
  jd_write_kernel<<<(unsigned)e.nwg, kJdLanes, 0, st>>>(e, g, coefs, status);
  MX_LAUNCH_CHECK();
  jd_dc_kernel<0><<<(unsigned)e.ntiles, 256, 0, st>>>(e, g, coefs);
  MX_LAUNCH_CHECK();
  jd_dc_carry_kernel<<<1, 1024, 0, st>>>(e, e.ntiles);
  MX_LAUNCH_CHECK();
  jd_dc_kernel<1><<<(unsigned)e.ntiles, 256, 0, st>>>(e, g, coefs);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
