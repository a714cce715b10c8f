// mx_draw.hip — detection overlays and side-by-side panels on the device (gfx950): what the reference's
// demo_inference.py does with cv2 on the host (draw_boxes, add_title, resize + hstack), reading the fused
// detection tail's padded outputs where they lie. The pixel semantics are stated in include/mx_det.h
// (mx_draw_batch_u8, mx_panels_compose_u8); this comment is about how the kernels get there.
//
// Overlay: a gather, not a sequence of painting passes, so the result cannot depend on the launch
// geometry or on which workgroup runs first. A workgroup (256 threads, 4 waves) owns one CB_ROWS x
// CB_COLS tile of one image's output (the tile of mx_corrupt_tile.h; the image follows from blockIdx.x
// by a scan over the chunk's <= DR_IMGS descriptors, which travel with the names and colours as the
// kernel argument). It walks the image's candidate rows in chunks of DR_CAP = one row per thread, last
// chunk first:
//   bin      thread t decides whether row c*DR_CAP + t is drawn (count, threshold, finite and bounded
//            coordinates) and whether its extent, the bounding box of frame and plate, meets the tile;
//            the hits are compacted in row order with one wave64 ballot per wave and a four-entry
//            prefix in LDS, and each hit's thread writes the row's integer corners, colour and label
//            text (name or cls<label>, then the score) into the LDS list;
//   gather   a thread owns five fixed pixels of the tile and keeps them in registers; each one not yet
//            resolved walks the list from the last row to the first and stops at the first row whose
//            text, plate or frame covers it (text lies inside the plate, and both top the frame).
// A chunk with no hit costs one ballot; a tile none of whose chunks has a hit and which lies below the
// title bar is copied straight from the source. The title bar's pixels are resolved when loaded.
// The finished pixels go through LDS to cb_store_tile: aligned dword vector stores, bytes at a row's
// partial ends. The first tile of an image also counts the drawn rows (hit or not) and writes drawn[b].
//
// Panels: one workgroup per canvas tile; a byte finds its panel among <= 8, then takes OpenCV's
// INTER_LINEAR u8 taps (lin_coef / linear_px of mx_corrupt_ops.h) from the panel's source, or the
// separator's grey.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mx_common.h"
#include "mx_corrupt_ops.h"
#include "mx_corrupt_tile.h"
#include "mx_font5x7.h"

namespace mx {

static constexpr int DR_IMGS = 16;               // images per launch (kernel argument)
static constexpr int DR_CAP = CB_THREADS;        // rows binned per chunk = list capacity
static constexpr int DR_PER = CB_ROWS * CB_COLS / CB_THREADS;  // pixels a thread owns
static constexpr int DR_STRIDE = CB_COLS * 3;
static constexpr int DR_NAMES = 32, DR_NAME = 16, DR_TITLE = 64, DR_TEXT = 28;
static constexpr int DR_LIM = 1 << 20;           // |coordinate| bound
static constexpr int DR_MAX_SCALE = 8;
static_assert(CB_ROWS * CB_COLS % CB_THREADS == 0, "every thread owns the same number of pixels");
static_assert(DR_STRIDE % 4 == 0, "tile rows are word-aligned in LDS");
// the longest label text: 15 name bytes or "cls" + 20 digits / sign, then " d.dd"
static_assert(DR_TEXT >= 15 + 5 && DR_TEXT >= 3 + 20 + 5, "label text fits");

struct DrImg {
  const uint8_t* src;
  uint8_t* dst;
  const float* boxes;
  const int64_t* labels;
  const float* scores;
  const int32_t* count;
  int32_t H, W, D, bar, tlen;
  int32_t tile0, tiles_x;  // first workgroup of this image; tiles per tile row
  char title[DR_TITLE];
};
struct DrChunk {
  DrImg im[DR_IMGS];
  char names[DR_NAMES][DR_NAME];
  uint8_t nlen[DR_NAMES];
  uint8_t col[DR_NAMES][3];
  int32_t* drawn;  // this chunk's slice
  float thr;
  int32_t nnames, ncol, ls, ts, n;
};
static_assert(sizeof(DrChunk) <= 3072, "the chunk travels as a kernel argument");

// one listed row
struct DrEnt {
  int32_t x1, y1, x2, y2;
  int32_t len;
  uint8_t col[3], pad;
  char text[DR_TEXT];
};

// "%.2f" of the exact f32 value for 0 <= s < 9.995 (see mx_draw_format_score); 4 bytes
__host__ __device__ inline void format_score(float s, char* out) {
  const double v = rint((double)s * 100.0);  // the product is exact: 24 + 7 significant bits
  const int n = !(v > 0.0) ? 0 : (v > 999.0 ? 999 : (int)v);
  out[0] = (char)('0' + n / 100);
  out[1] = '.';
  out[2] = (char)('0' + n / 10 % 10);
  out[3] = (char)('0' + n % 10);
}

// font pixel under (gx, gy) of a text's glyph block at scale s: 0 <= gx < 6*s*len, 0 <= gy < 7*s
template <typename Txt>
__device__ __forceinline__ bool text_on(Txt txt, int gx, int gy, int s) {
  const int adv = FONT_ADV * s;
  const int k = gx / adv;
  const int cx = (gx - k * adv) / s;
  if (cx >= FONT_COLS) return false;
  const int ch = (uint8_t)txt(k);
  const int g = (ch < FONT_FIRST || ch >= FONT_FIRST + FONT_GLYPHS) ? '?' - FONT_FIRST : ch - FONT_FIRST;
  return (FONT5X7[g][gy / s] >> (FONT_COLS - 1 - cx)) & 1;
}

__global__ void __launch_bounds__(CB_THREADS) draw_batch_kernel(DrChunk ck) {
  __shared__ DrEnt list[DR_CAP];
  __shared__ __attribute__((aligned(16))) uint8_t tile[CB_ROWS * DR_STRIDE];
  __shared__ int wcnt[CB_THREADS / 64];
  __shared__ int s_drawn;
  int b = 0;
  while (b + 1 < ck.n && (int)blockIdx.x >= ck.im[b + 1].tile0) ++b;
  const DrImg& m = ck.im[b];
  const int W = m.W, bar = m.bar, OH = m.bar + m.H;
  const int t = (int)blockIdx.x - m.tile0;
  const int ty = t / m.tiles_x, tx = t - ty * m.tiles_x;
  const int oy0 = ty * CB_ROWS, x0 = tx * CB_COLS;  // output coordinates
  const int rows = min(CB_ROWS, OH - oy0), cols = min(CB_COLS, W - x0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* __restrict__ src = m.src;
  const float* __restrict__ boxes = m.boxes;
  const int64_t* __restrict__ labels = m.labels;
  const float* __restrict__ scores = m.scores;
  const int ls = ck.ls, th = FONT_ROWS * ls;
  const float thr = ck.thr;

  int cnt = *m.count;
  const bool failed = cnt < 0;
  cnt = cnt < 0 ? 0 : (cnt > m.D ? m.D : cnt);
  // the tile in image coordinates (rows above the image: negative), inclusive
  const int iy0 = oy0 - bar, iy1 = iy0 + rows - 1, ix0 = x0, ix1 = x0 + cols - 1;
  const bool first = t == 0;
  if (tid == 0) s_drawn = 0;

  uint8_t px[DR_PER][3];
  unsigned done = 0;
  bool loaded = false;
  auto load = [&]() {
#pragma unroll
    for (int k = 0; k < DR_PER; ++k) {
      const int p = tid + k * CB_THREADS;
      const int r = p / CB_COLS, c = p - r * CB_COLS;
      px[k][0] = px[k][1] = px[k][2] = 0;
      if (r >= rows || c >= cols) {
        done |= 1u << k;
        continue;
      }
      const int oy = oy0 + r, x = x0 + c;
      if (oy < bar) {  // title bar
        const int ts = ck.ts, tw = FONT_ADV * ts * m.tlen, tth = FONT_ROWS * ts;
        const int gx = x - ((W - tw) >> 1), gy = oy - (((bar + tth) >> 1) - tth);  // >> floors
        const bool on = gx >= 0 && gx < tw && gy >= 0 && gy < tth && text_on([&](int q) { return m.title[q]; }, gx, gy, ts);
        px[k][0] = px[k][1] = px[k][2] = on ? 255 : 40;
        done |= 1u << k;
      } else {
        const uint8_t* s = src + ((int64_t)(oy - bar) * W + x) * 3;
        px[k][0] = s[0];
        px[k][1] = s[1];
        px[k][2] = s[2];
      }
    }
  };

  const int nch = (cnt + DR_CAP - 1) / DR_CAP;
  for (int ch = nch - 1; ch >= 0; --ch) {
    __syncthreads();  // the previous chunk's walk is over: the list and wcnt may be rewritten
    const int i = ch * DR_CAP + tid;
    bool live = false, hit = false;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0, len = 0;
    int64_t lab = 0;
    bool named = false;
    if (i < cnt && (!scores || scores[i] >= thr)) {
      const float c0 = boxes[4 * (int64_t)i], c1 = boxes[4 * (int64_t)i + 1], c2 = boxes[4 * (int64_t)i + 2],
                  c3 = boxes[4 * (int64_t)i + 3];
      const float lim = (float)DR_LIM;
      // false on NaN; an infinity fails the bound
      live = fabsf(c0) < lim && fabsf(c1) < lim && fabsf(c2) < lim && fabsf(c3) < lim;
      if (live) {
        x1 = (int)c0; y1 = (int)c1; x2 = (int)c2; y2 = (int)c3;
        lab = labels[i];
        named = lab >= 1 && lab <= ck.nnames && ck.nlen[lab - 1] > 0;
        if (named) {
          len = ck.nlen[lab - 1];
        } else {
          uint64_t mag = lab < 0 ? 0ull - (uint64_t)lab : (uint64_t)lab;
          len = 3 + (lab < 0 ? 1 : 0) + 1;
          while (mag >= 10) { mag /= 10; ++len; }
        }
        if (scores) len += 5;
        const int tw = FONT_ADV * ls * len;
        // bounding box of frame and plate
        const int ex0 = x1 - 1, ex1 = max(x2 + 1, x1 + tw + 4), ey0 = y1 - th - 6, ey1 = max(y2 + 1, y1);
        hit = ex0 <= ix1 && ex1 >= ix0 && ey0 <= iy1 && ey1 >= iy0;
      }
    }
    const unsigned long long bh = __ballot(hit), bl = __ballot(live);
    const int off = __popcll(bh & ((1ull << lane) - 1ull));
    if (lane == 0) {
      wcnt[wave] = __popcll(bh);
      if (first) atomicAdd(&s_drawn, __popcll(bl));
    }
    __syncthreads();
    int base = 0, nhit = 0;
#pragma unroll
    for (int w = 0; w < CB_THREADS / 64; ++w) {
      if (w < wave) base += wcnt[w];
      nhit += wcnt[w];
    }
    if (nhit == 0) continue;  // uniform
    if (hit) {
      DrEnt& e = list[base + off];
      e.x1 = x1; e.y1 = y1; e.x2 = x2; e.y2 = y2;
      e.len = len;
      const bool has = lab >= 1 && lab <= ck.ncol;
#pragma unroll
      for (int c = 0; c < 3; ++c) e.col[c] = has ? ck.col[lab - 1][c] : (uint8_t)200;
      int q = 0;
      if (named) {
        const int nl = ck.nlen[lab - 1];
        for (; q < nl; ++q) e.text[q] = ck.names[lab - 1][q];
      } else {
        e.text[q++] = 'c'; e.text[q++] = 'l'; e.text[q++] = 's';
        if (lab < 0) e.text[q++] = '-';
        uint64_t mag = lab < 0 ? 0ull - (uint64_t)lab : (uint64_t)lab;
        const int end = len - (scores ? 5 : 0);
        for (int d = end - 1; d >= q; --d) { e.text[d] = (char)('0' + (int)(mag % 10)); mag /= 10; }
        q = end;
      }
      if (scores) {
        char sc[4];
        format_score(scores[i], sc);
        e.text[q] = ' ';
        e.text[q + 1] = sc[0]; e.text[q + 2] = sc[1]; e.text[q + 3] = sc[2]; e.text[q + 4] = sc[3];
      }
    }
    if (!loaded) {
      load();
      loaded = true;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DR_PER; ++k) {
      if (done >> k & 1u) continue;
      const int p = tid + k * CB_THREADS;
      const int r = p / CB_COLS, c = p - r * CB_COLS;
      const int x = x0 + c, y = iy0 + r;
      for (int j = nhit - 1; j >= 0; --j) {
        const DrEnt& e = list[j];
        const int tw = FONT_ADV * ls * e.len;
        bool cover = false, white = false;
        if (x >= e.x1 && x <= e.x1 + tw + 4 && y >= e.y1 - th - 6 && y <= e.y1) {  // plate, text on it
          cover = true;
          const int gx = x - (e.x1 + 2), gy = y - (e.y1 - 3 - th);
          white = gx >= 0 && gx < tw && gy >= 0 && gy < th && text_on([&](int q) { return e.text[q]; }, gx, gy, ls);
        } else if (x >= e.x1 - 1 && x <= e.x2 + 1 && y >= e.y1 - 1 && y <= e.y2 + 1 &&
                   !(x >= e.x1 + 1 && x <= e.x2 - 1 && y >= e.y1 + 1 && y <= e.y2 - 1)) {  // frame
          cover = true;
        }
        if (cover) {
#pragma unroll
          for (int q = 0; q < 3; ++q) px[k][q] = white ? (uint8_t)255 : e.col[q];
          done |= 1u << k;
          break;
        }
      }
    }
  }

  if (!loaded && oy0 >= bar) {  // no row of the image meets the tile: a straight copy
    cb_store_tile(m.dst, W, oy0, x0, rows, cols,
                  [&](int r, int e) { return src[((int64_t)(iy0 + r) * W + x0) * 3 + e]; });
  } else {
    if (!loaded) load();
#pragma unroll
    for (int k = 0; k < DR_PER; ++k) {
      const int p = tid + k * CB_THREADS;
      const int r = p / CB_COLS, c = p - r * CB_COLS;
      if (r < rows && c < cols) {
        uint8_t* q = tile + r * DR_STRIDE + c * 3;
        q[0] = px[k][0];
        q[1] = px[k][1];
        q[2] = px[k][2];
      }
    }
    __syncthreads();
    cb_store_tile(m.dst, W, oy0, x0, rows, cols, [&](int r, int e) { return tile[r * DR_STRIDE + e]; });
  }
  if (first && tid == 0) ck.drawn[b] = failed ? -1 : s_drawn;
}

static constexpr int PN_MAX = 8, PN_SEP = 3;
struct PnArgs {
  const uint8_t* src[PN_MAX];
  int32_t h[PN_MAX], w[PN_MAX], dw[PN_MAX], x0[PN_MAX];  // x0: the panel's first canvas column
  uint8_t* dst;
  int32_t P, TH, CW, tiles_x;
};

__global__ void __launch_bounds__(CB_THREADS) panels_compose_kernel(PnArgs pa) {
  const int t = (int)blockIdx.x;
  const int ty = t / pa.tiles_x, tx = t - ty * pa.tiles_x;
  const int y0 = ty * CB_ROWS, x0 = tx * CB_COLS;
  const int rows = min(CB_ROWS, pa.TH - y0), cols = min(CB_COLS, pa.CW - x0);
  cb_store_tile(pa.dst, pa.CW, y0, x0, rows, cols, [&](int r, int e) -> uint8_t {
    const int xl = e / 3, c = e - xl * 3;
    const int x = x0 + xl, y = y0 + r;
    // the last panel that starts at or before x (unrolled: the arrays stay in scalar registers)
    const uint8_t* src = pa.src[0];
    int h = pa.h[0], w = pa.w[0], dw = pa.dw[0], px0 = 0;
#pragma unroll
    for (int p = 1; p < PN_MAX; ++p)
      if (p < pa.P && x >= pa.x0[p]) {
        src = pa.src[p]; h = pa.h[p]; w = pa.w[p]; dw = pa.dw[p]; px0 = pa.x0[p];
      }
    const int lx = x - px0;
    if (lx >= dw) return 200;  // separator
    int64_t r0, c0;
    int b0, b1, a0, a1;
    lin_coef(h, pa.TH, y, &r0, &b0, &b1);
    lin_coef(w, dw, lx, &c0, &a0, &a1);
    const int64_t r1 = r0 + 1 < h ? r0 + 1 : h - 1, c1 = c0 + 1 < w ? c0 + 1 : w - 1;
    const uint8_t* q0 = src + r0 * w * 3 + c;
    const uint8_t* q1 = src + r1 * w * 3 + c;
    return linear_px(q0[c0 * 3], q0[c1 * 3], q1[c0 * 3], q1[c1 * 3], a0, a1, b0, b1);
  });
}

static bool draw_overlap(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace mx

using namespace mx;

extern "C" int mx_draw_batch_tile(int32_t out[3]) {
  MX_CHECK_ARG(out != nullptr, "mx_draw_batch_tile: null output");
  out[0] = CB_ROWS;
  out[1] = CB_COLS;
  out[2] = DR_CAP;
  return MX_OK;
}

extern "C" int mx_draw_font(uint8_t* out) {
  MX_CHECK_ARG(out != nullptr, "mx_draw_font: null output");
  memcpy(out, FONT5X7, sizeof(FONT5X7));
  return MX_OK;
}

extern "C" int mx_draw_format_score(float s, char out[5]) {
  MX_CHECK_ARG(out != nullptr, "mx_draw_format_score: null output");
  format_score(s, out);
  out[4] = 0;
  return MX_OK;
}

extern "C" int mx_draw_batch_u8(const mx_draw_desc* descs_host, int64_t n, const char* const* names_host, int32_t nnames,
                                const uint8_t* colors_host, int32_t ncolors, float conf_thr, int32_t label_scale,
                                int32_t title_scale, int32_t* drawn, mx_stream_t stream) {
  MX_CHECK_ARG(nnames >= 0 && nnames <= DR_NAMES && (nnames == 0 || names_host),
               "mx_draw_batch_u8: at most %d class names, got %d", DR_NAMES, nnames);
  for (int k = 0; k < nnames; ++k)
    MX_CHECK_ARG(names_host[k] && strlen(names_host[k]) < (size_t)DR_NAME,
                 "mx_draw_batch_u8: class name %d is null or longer than %d bytes", k, DR_NAME - 1);
  MX_CHECK_ARG(ncolors >= 0 && ncolors <= DR_NAMES && (ncolors == 0 || colors_host),
               "mx_draw_batch_u8: at most %d colours, got %d", DR_NAMES, ncolors);
  MX_CHECK_ARG(label_scale >= 1 && label_scale <= DR_MAX_SCALE && title_scale >= 1 && title_scale <= DR_MAX_SCALE,
               "mx_draw_batch_u8: font scales must be 1..%d, got %d and %d", DR_MAX_SCALE, label_scale, title_scale);
  MX_CHECK_ARG(n >= 0 && (n == 0 || (descs_host && drawn)), "mx_draw_batch_u8: bad descriptor array or null drawn");
  // every descriptor is checked before the first launch
  for (int64_t b = 0; b < n; ++b) {
    const mx_draw_desc& d = descs_host[b];
    MX_CHECK_ARG(d.title_len >= 0 && d.title_len <= DR_TITLE, "mx_draw_batch_u8: image %lld: title of %d bytes (at most %d)",
                 (long long)b, d.title_len, DR_TITLE);
    MX_CHECK_ARG(d.src && d.dst && d.H >= 1 && d.W >= 1 && d.H <= 32768 && d.W <= 32768,
                 "mx_draw_batch_u8: image %lld: null image or bad size %d x %d", (long long)b, d.H, d.W);
    MX_CHECK_ARG(d.bar >= 0 && d.bar <= 1024, "mx_draw_batch_u8: image %lld: bar %d outside 0..1024", (long long)b, d.bar);
    MX_CHECK_ARG(d.D >= 0 && d.D <= DR_LIM && (d.D == 0 || (d.boxes && d.labels)) && d.count,
                 "mx_draw_batch_u8: image %lld: bad D %d or null boxes / labels / count", (long long)b, d.D);
  }
  for (int64_t i = 0; i < n; ++i) {
    const mx_draw_desc& a = descs_host[i];
    const int64_t na = (int64_t)(a.bar + a.H) * a.W * 3;
    for (int64_t j = 0; j < n; ++j) {
      const mx_draw_desc& c = descs_host[j];
      MX_CHECK_ARG(!draw_overlap(a.dst, na, c.src, (int64_t)c.H * c.W * 3), "mx_draw_batch_u8: output %lld overlaps input %lld",
                   (long long)i, (long long)j);
      if (j > i)
        MX_CHECK_ARG(!draw_overlap(a.dst, na, c.dst, (int64_t)(c.bar + c.H) * c.W * 3),
                     "mx_draw_batch_u8: outputs %lld and %lld overlap", (long long)i, (long long)j);
    }
  }

  hipStream_t s = (hipStream_t)stream;
  DrChunk ck{};
  ck.nnames = nnames;
  ck.ncol = ncolors;
  ck.thr = conf_thr;
  ck.ls = label_scale;
  ck.ts = title_scale;
  for (int k = 0; k < nnames; ++k) {
    ck.nlen[k] = (uint8_t)strlen(names_host[k]);
    memcpy(ck.names[k], names_host[k], ck.nlen[k]);
  }
  for (int k = 0; k < ncolors; ++k)
    for (int c = 0; c < 3; ++c) ck.col[k][c] = colors_host[3 * k + c];
  for (int64_t b0 = 0; b0 < n; b0 += DR_IMGS) {
    const int nb = (int)std::min<int64_t>(DR_IMGS, n - b0);
    int64_t tiles = 0;
    for (int q = 0; q < nb; ++q) {
      const mx_draw_desc& d = descs_host[b0 + q];
      DrImg& m = ck.im[q];
      m = DrImg{};
      m.src = d.src; m.dst = d.dst; m.boxes = d.boxes; m.labels = d.labels; m.scores = d.scores; m.count = d.count;
      m.H = d.H; m.W = d.W; m.D = d.D; m.bar = d.bar; m.tlen = d.title_len;
      memcpy(m.title, d.title, (size_t)d.title_len);
      const int64_t tx = cdiv(d.W, CB_COLS), tyn = cdiv((int64_t)d.bar + d.H, CB_ROWS);
      m.tile0 = (int32_t)tiles;
      m.tiles_x = (int32_t)tx;
      tiles += tx * tyn;  // <= 16 images of <= 410 x 2112 tiles: below 2^31
    }
    ck.n = nb;
    ck.drawn = drawn + b0;
    draw_batch_kernel<<<(unsigned)tiles, CB_THREADS, 0, s>>>(ck);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

extern "C" int mx_panels_compose_u8(const mx_panel_desc* panels_host, int32_t P, int32_t target_h, uint8_t* canvas,
                                    mx_stream_t stream) {
  MX_CHECK_ARG(P >= 1 && P <= PN_MAX, "mx_panels_compose_u8: 1..%d panels, got %d", PN_MAX, P);
  MX_CHECK_ARG(panels_host && canvas && target_h >= 1 && target_h <= 32768,
               "mx_panels_compose_u8: null panels / canvas or bad target height %d", target_h);
  PnArgs pa{};
  int64_t cw = 0;
  for (int p = 0; p < P; ++p) {
    const mx_panel_desc& d = panels_host[p];
    MX_CHECK_ARG(d.src && d.h >= 1 && d.w >= 1 && d.h <= 32768 && d.w <= 32768 && d.dw >= 1 && d.dw <= 32768,
                 "mx_panels_compose_u8: panel %d: null source or bad size %d x %d -> width %d", p, d.h, d.w, d.dw);
    pa.src[p] = d.src; pa.h[p] = d.h; pa.w[p] = d.w; pa.dw[p] = d.dw;
    pa.x0[p] = (int32_t)cw;
    cw += d.dw + (p + 1 < P ? PN_SEP : 0);
  }
  for (int p = 0; p < P; ++p)
    MX_CHECK_ARG(!draw_overlap(canvas, cw * target_h * 3, pa.src[p], (int64_t)pa.h[p] * pa.w[p] * 3),
                 "mx_panels_compose_u8: the canvas overlaps panel %d", p);
  pa.dst = canvas;
  pa.P = P;
  pa.TH = target_h;
  pa.CW = (int32_t)cw;
  pa.tiles_x = (int32_t)cdiv(cw, CB_COLS);
  const int64_t tiles = (int64_t)pa.tiles_x * cdiv(target_h, CB_ROWS);
  panels_compose_kernel<<<(unsigned)tiles, CB_THREADS, 0, (hipStream_t)stream>>>(pa);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
