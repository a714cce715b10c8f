// mx_corrupt.hip — the corruption ops for a whole batch in one launch (gfx950): per-image op, strength,
// tap set and size, one workgroup per output tile of one image. Built -ffp-contract=off; every value
// comes out of mx_corrupt_ops.h, the arithmetic mx_elementwise.hip's one-op kernels use, so image b of a
// batch is bit-identical to mx_corrupt_u8 / mx_filter2d_u8 called for that image alone.
//
// Tile scheme. A workgroup (256 threads, 4 waves) owns CB_ROWS x CB_COLS output pixels of one image; the
// image and the tile follow from blockIdx.x by a scan over the chunk's <= CB_IMGS descriptors, which
// travel with the tap table as the kernel argument (no upload, no synchronisation, graph-capturable).
//   noise / identity: no LDS; each lane reads the source bytes of the dword it writes.
//   blur: the source tile plus the image's own halo (max |dy|, |dx| of its taps, <= CB_HALO) is staged in
//     LDS with BORDER_REFLECT_101 applied while staging, so the tap loop reads LDS without a border rule.
//   low-res: the INTER_AREA pixels the tile's INTER_LINEAR reads (the rows and columns lin_coef names for
//     the tile's first and last row and column, plus one) are computed from the source into LDS -- the
//     exact-x2 fast path or the general table, per image, as mx_corrupt_u8 chooses (the general path
//     first builds OpenCV's (source, alpha) table of every staged column and row in LDS, once each, not
//     once per pixel) -- then, after one barrier, the 11-bit up-scale runs out of LDS. No intermediate
//     image in HBM, no second launch.
// Stores (cb_store_tile, mx_corrupt_tile.h, shared with mx_weather.hip). A wave owns a tile row at a time; lane g owns the g-th aligned dword of that row's byte span
// (<= 61 dwords of 240 bytes plus misalignment), computes its 4 bytes and writes one dword; the first
// and last dword of a row, where they are partial, are written byte by byte.
#include <algorithm>
#include <cstdlib>

#include "mx_common.h"
#include "mx_corrupt_ops.h"
#include "mx_corrupt_tile.h"

namespace mx {

static constexpr int CB_HALO = 15;                      // largest tap reach
static constexpr int CB_IMGS = 16, CB_TAPS = 192;       // per chunk (kernel argument)
static constexpr int CB_BLUR_COLS = CB_COLS + 2 * CB_HALO, CB_BLUR_ROWS = CB_ROWS + 2 * CB_HALO;
static constexpr int CB_BLUR_STRIDE = CB_BLUR_COLS * 3 + 2;  // bytes per staged row (a multiple of 4)
// the up-scale reads s(d) = floor((d + .5) * scale - .5) and s + 1, scale <= 1: a tile's first and last
// row are < CB_ROWS source rows apart (one more for the f32 rounding of the coordinate), plus one
static constexpr int CB_LR_ROWS = CB_ROWS + 2, CB_LR_COLS = CB_COLS + 2;
static constexpr int CB_LR_STRIDE = CB_LR_COLS * 3 + 2;
// OpenCV's INTER_AREA table of one staged low-res column or row (area_entries): n (source index, alpha)
struct CbAreaTab {
  int32_t n;
  int32_t s[8];
  float al[8];
};
static constexpr int CB_LR_TABS = CB_LR_ROWS * CB_LR_STRIDE;  // the tables follow the staged pixels
static constexpr int CB_LR_LDS = CB_LR_TABS + (CB_LR_COLS + CB_LR_ROWS) * (int)sizeof(CbAreaTab);
static constexpr int CB_LDS = CB_BLUR_ROWS * CB_BLUR_STRIDE > CB_LR_LDS ? CB_BLUR_ROWS * CB_BLUR_STRIDE : CB_LR_LDS;
static_assert(CB_LR_TABS % 4 == 0, "the tables are word-aligned");
static_assert(CB_BLUR_STRIDE % 4 == 0 && CB_LR_STRIDE % 4 == 0, "LDS rows start on a bank boundary");

struct CbImg {
  const uint8_t* src;
  uint8_t* dst;
  const float* noise;  // this image's slice of the call's field, or NULL
  uint64_t seed;
  int32_t H, W, nh, nw;
  float sigma;
  int32_t op;
  int32_t tap0, ntaps;  // into CbChunk::tap*
  int32_t hy, hx;       // the tap set's reach
  int32_t tile0;        // first workgroup of this image
  int32_t tiles_x;
};
struct CbChunk {
  CbImg im[CB_IMGS];
  int8_t tdy[CB_TAPS], tdx[CB_TAPS];
  float tc[CB_TAPS];
  int32_t n;
};
static_assert(sizeof(CbChunk) <= 3072, "the chunk travels as a kernel argument");

__global__ void __launch_bounds__(CB_THREADS) corrupt_batch_kernel(CbChunk ck) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[CB_LDS];
  int b = 0;
  while (b + 1 < ck.n && (int)blockIdx.x >= ck.im[b + 1].tile0) ++b;
  const CbImg& m = ck.im[b];
  const int H = m.H, W = m.W;
  const int t = (int)blockIdx.x - m.tile0;
  const int ty = t / m.tiles_x, tx = t - ty * m.tiles_x;
  const int y0 = ty * CB_ROWS, x0 = tx * CB_COLS;
  const int rows = min(CB_ROWS, H - y0), cols = min(CB_COLS, W - x0);
  const uint8_t* src = m.src;  // may be dst (noise in place): no restrict
  const int tid = threadIdx.x;

  if (m.op == 0) {  // identity: copy
    cb_store_tile(m.dst, W, y0, x0, rows, cols,
                  [&](int r, int e) { return src[((int64_t)(y0 + r) * W + x0) * 3 + e]; });
  } else if (m.op == 1) {  // noise; in place is safe: a thread reads exactly the bytes it writes, first
    const float* __restrict__ noise = m.noise;
    const float sigma = m.sigma;
    const uint64_t seed = m.seed;
    cb_store_tile(m.dst, W, y0, x0, rows, cols, [&](int r, int e) {
      const int64_t i = ((int64_t)(y0 + r) * W + x0) * 3 + e;  // flat index within this image
      return noise_px([&] { return src[i]; }, noise, sigma, seed, i);
    });
  } else if (m.op == 2) {  // blur: stage tile + halo, reflected
    const int hy = m.hy, hx = m.hx;
    const int srows = rows + 2 * hy, scols = cols + 2 * hx;
    for (int i = tid; i < srows * scols; i += CB_THREADS) {
      const int ly = i / scols, lx = i - ly * scols;
      const int64_t gy = refl101((int64_t)y0 - hy + ly, H), gx = refl101((int64_t)x0 - hx + lx, W);
      const uint8_t* p = src + (gy * W + gx) * 3;
      uint8_t* q = lds + ly * CB_BLUR_STRIDE + lx * 3;
      q[0] = p[0];
      q[1] = p[1];
      q[2] = p[2];
    }
    __syncthreads();
    const int tap0 = m.tap0, ntaps = m.ntaps;
    cb_store_tile(m.dst, W, y0, x0, rows, cols, [&](int r, int e) {
      const uint8_t* q = lds + (r + hy) * CB_BLUR_STRIDE + hx * 3 + e;
      return filter2d_px(
          ntaps, [&](int k) { return ck.tc[tap0 + k]; },
          [&](int k) { return q[(int)ck.tdy[tap0 + k] * CB_BLUR_STRIDE + (int)ck.tdx[tap0 + k] * 3]; });
    });
  } else {  // low-res: INTER_AREA into LDS, INTER_LINEAR out of it
    const int nh = m.nh, nw = m.nw;
    int64_t ra, rb, ca, cb;
    int u0, u1;
    lin_coef(nh, H, y0, &ra, &u0, &u1);
    lin_coef(nh, H, y0 + rows - 1, &rb, &u0, &u1);
    lin_coef(nw, W, x0, &ca, &u0, &u1);
    lin_coef(nw, W, x0 + cols - 1, &cb, &u0, &u1);
    const int lr_rows = min((int)min<int64_t>(rb + 1, nh - 1) - (int)ra + 1, CB_LR_ROWS);
    const int lr_cols = min((int)min<int64_t>(cb + 1, nw - 1) - (int)ca + 1, CB_LR_COLS);
    const bool fast2 = W == 2 * nw && H == 2 * nh;  // OpenCV's exact-x2 INTER_AREA path
    const int64_t vec_elems = area_fast2_vec_elems(nw, 3);
    if (fast2) {
      for (int i = tid; i < lr_rows * lr_cols; i += CB_THREADS) {
        const int ly = i / lr_cols, lx = i - ly * lr_cols;
        const int64_t dy = ra + ly, dx = ca + lx;
        uint8_t* q = lds + ly * CB_LR_STRIDE + lx * 3;
        const uint8_t* s0 = src + ((2 * dy) * W + 2 * dx) * 3;
        const uint8_t* s1 = s0 + (int64_t)W * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int sum = (int)s0[c] + (int)s0[3 + c] + (int)s1[c] + (int)s1[3 + c];
          q[c] = area_fast2_px(sum, dx * 3 + c < vec_elems);
        }
      }
    } else {
      // the (source, alpha) tables once per staged column and row, in LDS, not once per pixel
      CbAreaTab* xt = (CbAreaTab*)(lds + CB_LR_TABS);
      CbAreaTab* yt = xt + CB_LR_COLS;
      for (int i = tid; i < lr_cols + lr_rows; i += CB_THREADS) {
        const bool isx = i < lr_cols;
        int64_t si[8];
        float al[8];
        const int n = area_entries(isx ? W : H, isx ? ca + i : ra + (i - lr_cols), isx ? (double)W / nw : (double)H / nh,
                                   si, al);
        CbAreaTab* tb = isx ? xt + i : yt + (i - lr_cols);
        tb->n = n;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < n) {
            tb->s[k] = (int)si[k];
            tb->al[k] = al[k];
          }
      }
      __syncthreads();
      for (int i = tid; i < lr_rows * lr_cols; i += CB_THREADS) {
        const int ly = i / lr_cols, lx = i - ly * lr_cols;
        uint8_t* q = lds + ly * CB_LR_STRIDE + lx * 3;
        const CbAreaTab* tx = xt + lx;
        const CbAreaTab* tyy = yt + ly;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          q[c] = area_px(tx->n, tx->al, tyy->n, tyy->al,
                         [&](int j, int k) { return src[(int64_t)tyy->s[j] * W * 3 + tx->s[k] * 3 + c]; });
      }
    }
    __syncthreads();
    cb_store_tile(m.dst, W, y0, x0, rows, cols, [&](int r, int e) {
      const int xl = e / 3, c = e - xl * 3;
      int64_t r0, c0;
      int b0, b1, a0, a1;
      lin_coef(nh, H, y0 + r, &r0, &b0, &b1);
      lin_coef(nw, W, x0 + xl, &c0, &a0, &a1);
      const int64_t r1 = r0 + 1 < nh ? r0 + 1 : nh - 1, c1 = c0 + 1 < nw ? c0 + 1 : nw - 1;
      // staged coordinates; the clamps never bind (see CB_LR_ROWS) and keep every read inside the array
      const int l0 = min((int)(r0 - ra), CB_LR_ROWS - 1), l1 = min((int)(r1 - ra), CB_LR_ROWS - 1);
      const int k0 = min((int)(c0 - ca), CB_LR_COLS - 1), k1 = min((int)(c1 - ca), CB_LR_COLS - 1);
      const uint8_t* q0 = lds + l0 * CB_LR_STRIDE + c;
      const uint8_t* q1 = lds + l1 * CB_LR_STRIDE + c;
      return linear_px(q0[k0 * 3], q0[k1 * 3], q1[k0 * 3], q1[k1 * 3], a0, a1, b0, b1);
    });
  }
}

static bool overlap(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace mx

using namespace mx;

extern "C" int mx_corrupt_batch_tile(int32_t out[2]) {
  MX_CHECK_ARG(out != nullptr, "mx_corrupt_batch_tile: null output");
  out[0] = CB_ROWS;
  out[1] = CB_COLS;
  return MX_OK;
}

extern "C" int mx_corrupt_batch_u8(const mx_corrupt_desc* descs_host, int64_t n, const float* taps_host, int64_t ntaps_total,
                                   const float* noise, mx_stream_t stream) {
  MX_CHECK_ARG(n >= 0 && (n == 0 || descs_host) && ntaps_total >= 0 && (ntaps_total == 0 || taps_host),
               "mx_corrupt_batch_u8: bad descriptor or tap table");
  // every descriptor is checked before the first launch
  for (int64_t b = 0; b < n; ++b) {
    const mx_corrupt_desc& d = descs_host[b];
    MX_CHECK_ARG(d.op >= 0 && d.op <= 3, "mx_corrupt_batch_u8: image %lld: bad op %d", (long long)b, d.op);
    MX_CHECK_ARG(d.src && d.dst && d.H >= 1 && d.W >= 1 && d.H <= 32768 && d.W <= 32768,
                 "mx_corrupt_batch_u8: image %lld: null image or bad size %d x %d", (long long)b, d.H, d.W);
    const int64_t per = (int64_t)d.H * d.W * 3;
    if (d.src == d.dst)
      MX_CHECK_ARG(d.op <= 1, "mx_corrupt_batch_u8: image %lld: blur and low-res cannot run in place", (long long)b);
    else
      MX_CHECK_ARG(!overlap(d.src, per, d.dst, per), "mx_corrupt_batch_u8: image %lld: src and dst overlap", (long long)b);
    if (d.op == 2) {
      MX_CHECK_ARG(d.ntaps >= 0 && d.ntaps <= 128, "mx_corrupt_batch_u8: image %lld: at most 128 non-zero taps",
                   (long long)b);
      MX_CHECK_ARG(d.tap_off >= 0 && (int64_t)d.tap_off + d.ntaps <= ntaps_total,
                   "mx_corrupt_batch_u8: image %lld: taps outside the table", (long long)b);
      for (int k = 0; k < d.ntaps; ++k) {
        const float* t = taps_host + 3 * ((int64_t)d.tap_off + k);
        MX_CHECK_ARG(t[0] >= -CB_HALO && t[0] <= CB_HALO && t[1] >= -CB_HALO && t[1] <= CB_HALO,
                     "mx_corrupt_batch_u8: image %lld: tap reach over %d", (long long)b, CB_HALO);
      }
    }
    if (d.op == 3)
      MX_CHECK_ARG(d.nh >= 1 && d.nh <= d.H && d.nw >= 1 && d.nw <= d.W,
                   "mx_corrupt_batch_u8: image %lld: low-res size %d x %d outside 1..%d x 1..%d", (long long)b, d.nh,
                   d.nw, d.H, d.W);
  }
  // no image's output may meet another image's input or output (an in-place identity writes nothing)
  for (int64_t i = 0; i < n; ++i) {
    const mx_corrupt_desc& a = descs_host[i];
    if (a.op == 0 && a.src == a.dst) continue;
    const int64_t na = (int64_t)a.H * a.W * 3;
    for (int64_t j = 0; j < n; ++j) {
      if (j == i) continue;
      const mx_corrupt_desc& c = descs_host[j];
      const int64_t nc = (int64_t)c.H * c.W * 3;
      MX_CHECK_ARG(!overlap(a.dst, na, c.src, nc), "mx_corrupt_batch_u8: output %lld overlaps input %lld", (long long)i,
                   (long long)j);
      if (j > i && !(c.op == 0 && c.src == c.dst))
        MX_CHECK_ARG(!overlap(a.dst, na, c.dst, nc), "mx_corrupt_batch_u8: outputs %lld and %lld overlap", (long long)i,
                     (long long)j);
    }
  }

  hipStream_t s = (hipStream_t)stream;
  CbChunk ck{};
  int ntap = 0;
  int64_t tiles = 0;
  int set_off[CB_IMGS], set_n[CB_IMGS], set_at[CB_IMGS], nsets = 0;  // tap sets already in the chunk
  auto flush = [&]() -> int {
    if (ck.n > 0 && tiles > 0) {
      corrupt_batch_kernel<<<(unsigned)tiles, CB_THREADS, 0, s>>>(ck);
      MX_LAUNCH_CHECK();
    }
    ck.n = 0;
    ntap = nsets = 0;
    tiles = 0;
    return MX_OK;
  };
  int64_t noise_off = 0;
  for (int64_t b = 0; b < n; ++b) {
    const mx_corrupt_desc& d = descs_host[b];
    const int64_t per = (int64_t)d.H * d.W * 3;
    const int64_t my_noise = noise_off;
    noise_off += per;
    if (d.op == 0 && d.src == d.dst) continue;
    int set = -1;
    if (d.op == 2) {
      for (int q = 0; q < nsets; ++q)
        if (set_off[q] == d.tap_off && set_n[q] == d.ntaps) set = q;
      if (set < 0 && ntap + d.ntaps > CB_TAPS) {
        const int rc = flush();
        if (rc) return rc;
      }
    }
    const int64_t tx = cdiv(d.W, CB_COLS), tyn = cdiv(d.H, CB_ROWS);
    if (ck.n == CB_IMGS || tiles + tx * tyn > 0x7fffffff) {
      const int rc = flush();
      if (rc) return rc;
      set = -1;
    }
    CbImg& m = ck.im[ck.n];
    m = CbImg{};
    m.src = d.src;
    m.dst = d.dst;
    m.noise = noise ? noise + my_noise : nullptr;
    m.seed = d.seed;
    m.H = d.H; m.W = d.W; m.nh = d.nh; m.nw = d.nw;
    m.sigma = d.sigma;
    m.op = d.op;
    if (d.op == 2) {
      if (set < 0) {
        set = nsets++;
        set_off[set] = d.tap_off;
        set_n[set] = d.ntaps;
        set_at[set] = ntap;
        for (int k = 0; k < d.ntaps; ++k) {
          const float* t = taps_host + 3 * ((int64_t)d.tap_off + k);
          ck.tdy[ntap] = (int8_t)(int)t[0];
          ck.tdx[ntap] = (int8_t)(int)t[1];
          ck.tc[ntap] = t[2];
          ++ntap;
        }
      }
      m.tap0 = set_at[set];
      m.ntaps = d.ntaps;
      for (int k = 0; k < d.ntaps; ++k) {
        m.hy = std::max<int>(m.hy, std::abs((int)ck.tdy[m.tap0 + k]));
        m.hx = std::max<int>(m.hx, std::abs((int)ck.tdx[m.tap0 + k]));
      }
    }
    m.tile0 = (int32_t)tiles;
    m.tiles_x = (int32_t)tx;
    tiles += tx * tyn;
    ++ck.n;
  }
  return flush();
}
