// mx_weather.hip — night, haze and rain for a whole batch in one launch (gfx950): per-image op, parameters
// and size, one workgroup per output tile of one image, the scheme of mx_corrupt.hip (same tile, same
// store side: mx_corrupt_tile.h). Built -ffp-contract=off. The three ops are this project's own
// definitions (include/mx_det.h states them in full); every random bit is a Philox4x32-10 word
// (mx_corrupt_ops.h) keyed by the image's seed, so a numpy restatement gives the same bytes.
//   night: f32, per byte; no LDS. d = v * gain, out = clip(d + sqrt(shot * d + read2) * g), g from the
//     call's field or from gauss(seed, flat index). Each f32 op rounds once; the sqrt is the IEEE one.
//   haze: integers. Four octaves of value noise on the lattice hash L_o(j, i); the <= 2 x 5 lattice
//     points per octave that the tile touches are hashed once into LDS, then each pixel's alpha (q16) is
//     interpolated into LDS, then the store pass blends v towards `air`.
//   rain: integers. The drop heads of rows y0 .. y0 + rows + len - 2 and of the columns the slant reaches
//     are hashed into LDS as bytes (one Philox per 4 columns), then each pixel's streak strength R (the
//     nearest head up the streak) goes into LDS, then the store pass lightens v.
// Every op reads only the pixel it writes, so src == dst is allowed.
#include <cmath>

#include "mx_common.h"
#include "mx_corrupt_ops.h"
#include "mx_corrupt_tile.h"

namespace mx {

static constexpr int WX_IMGS = 16;                 // per chunk (kernel argument)
static constexpr int WX_HAZE_OCT = 4, WX_HAZE_NJ = 2, WX_HAZE_NI = 5;  // lattice points per octave and tile
static constexpr int WX_RAIN_LEN = 32, WX_RAIN_SLANT = 8;
static constexpr int WX_RAIN_ROWS = CB_ROWS + WX_RAIN_LEN - 1;
// columns a tile reads: its own plus the reach ((len - 1) * |slant|) >> 3 on one side, in groups of 4
// that start anywhere in a group: ceil((CB_COLS + reach + 3) / 4)
static constexpr int WX_RAIN_REACH = ((WX_RAIN_LEN - 1) * WX_RAIN_SLANT) >> 3;
static constexpr int WX_RAIN_GROUPS = (CB_COLS + WX_RAIN_REACH + 3 + 3) / 4;
static constexpr int WX_RAIN_STRIDE = WX_RAIN_GROUPS * 4;  // bytes per staged row
static constexpr int WX_PX_BYTES = CB_ROWS * CB_COLS * 2;  // the per-pixel alpha / R, u16
static constexpr int WX_LDS = WX_PX_BYTES + WX_RAIN_ROWS * WX_RAIN_STRIDE;
static_assert(WX_HAZE_OCT * WX_HAZE_NJ * WX_HAZE_NI * 4 <= WX_RAIN_ROWS * WX_RAIN_STRIDE, "the lattice shares the flags' space");
static_assert(256 % CB_ROWS == 0 && (256 >> (WX_HAZE_OCT - 1)) >= CB_ROWS, "a tile's rows lie in one cell of every octave");
static_assert((CB_COLS - 1 + (256 >> (WX_HAZE_OCT - 1)) - 1) / (256 >> (WX_HAZE_OCT - 1)) + 2 <= WX_HAZE_NI, "lattice columns per tile");
static_assert(WX_PX_BYTES % 4 == 0 && WX_LDS < 16384, "LDS budget");

struct WxImg {
  const uint8_t* src;
  uint8_t* dst;
  const float* noise;  // this image's slice of the call's field, or NULL
  uint64_t seed;
  int32_t H, W, op;
  int32_t tile0;       // first workgroup of this image
  int32_t tiles_x;
  float gain, shot, read2;             // night
  int32_t lo, hi, air;                 // haze
  int32_t thr, len, slant, fade, beta; // rain
};
struct WxChunk {
  WxImg im[WX_IMGS];
  int32_t n;
};
static_assert(sizeof(WxChunk) <= 3072, "the chunk travels as a kernel argument");

// night, one byte: every f32 op rounds once (the file is built without contraction)
__device__ __forceinline__ uint8_t night_px(int v, float g, float gain, float shot, float read2) {
  const float d = (float)v * gain;
  const float s = __fsqrt_rn(shot * d + read2);
  float o = d + s * g;
  o = o < 0.f ? 0.f : (o > 255.f ? 255.f : o);
  return (uint8_t)o;
}

__global__ void __launch_bounds__(CB_THREADS) weather_batch_kernel(WxChunk ck) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[WX_LDS];
  int b = 0;
  while (b + 1 < ck.n && (int)blockIdx.x >= ck.im[b + 1].tile0) ++b;
  const WxImg& m = ck.im[b];
  const int H = m.H, W = m.W;
  const int t = (int)blockIdx.x - m.tile0;
  const int ty = t / m.tiles_x, tx = t - ty * m.tiles_x;
  const int y0 = ty * CB_ROWS, x0 = tx * CB_COLS;
  const int rows = min(CB_ROWS, H - y0), cols = min(CB_COLS, W - x0);
  const uint8_t* src = m.src;  // may be dst (in place): no restrict
  const int tid = threadIdx.x;
  const uint2 key = make_uint2((uint32_t)m.seed, (uint32_t)(m.seed >> 32));
  uint16_t* px = (uint16_t*)lds;          // [CB_ROWS][CB_COLS]: alpha (haze) or R (rain)
  uint8_t* aux = lds + WX_PX_BYTES;       // the lattice (haze) or the drop heads (rain)

  if (m.op == 1) {  // night; a thread reads exactly the bytes it writes, first
    const float* __restrict__ noise = m.noise;
    const float gain = m.gain, shot = m.shot, read2 = m.read2;
    const uint64_t seed = m.seed;
    cb_store_tile(m.dst, W, y0, x0, rows, cols, [&](int r, int e) {
      const int64_t i = ((int64_t)(y0 + r) * W + x0) * 3 + e;  // flat index within this image
      const float g = noise ? noise[i] : gauss(seed, (uint64_t)i);
      return night_px(src[i], g, gain, shot, read2);
    });
  } else if (m.op == 2) {  // haze
    uint32_t* lat = (uint32_t*)aux;  // [octave][WX_HAZE_NJ][WX_HAZE_NI]
    for (int i = tid; i < WX_HAZE_OCT * WX_HAZE_NJ * WX_HAZE_NI; i += CB_THREADS) {
      const int o = i / (WX_HAZE_NJ * WX_HAZE_NI), q = i - o * (WX_HAZE_NJ * WX_HAZE_NI);
      const int lj = q / WX_HAZE_NI, li = q - lj * WX_HAZE_NI;
      const int s = 8 - o;
      const uint4 w = philox(make_uint4((uint32_t)((x0 >> s) + li), (uint32_t)((y0 >> s) + lj), 0x48415a45u, (uint32_t)o), key);
      lat[i] = w.x >> 16;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)m.lo, span = (uint32_t)(m.hi - m.lo);
    for (int i = tid; i < rows * cols; i += CB_THREADS) {
      const int r = i / cols, xl = i - r * cols;
      const uint32_t y = (uint32_t)(y0 + r), x = (uint32_t)(x0 + xl);
      uint32_t S = 0;
#pragma unroll
      for (int o = 0; o < WX_HAZE_OCT; ++o) {
        const int s = 8 - o;
        const uint32_t c = 256u >> o, fy = y & (c - 1), fx = x & (c - 1);
        // the clamps never bind (see the static_asserts) and keep every read inside the array
        const int lj = min((int)(y >> s) - (y0 >> s), WX_HAZE_NJ - 2), li = min((int)(x >> s) - (x0 >> s), WX_HAZE_NI - 2);
        const uint32_t* L = lat + (o * WX_HAZE_NJ + lj) * WX_HAZE_NI + li;
        const uint32_t top = L[0] * (c - fx) + L[1] * fx;
        const uint32_t bot = L[WX_HAZE_NI] * (c - fx) + L[WX_HAZE_NI + 1] * fx;
        S += (8u >> o) * ((top * (c - fy) + bot * fy) >> (2 * s));
      }
      const uint32_t S16 = (S * 4369u) >> 16;
      px[r * CB_COLS + xl] = (uint16_t)(lo + ((span * S16) >> 16));
    }
    __syncthreads();
    const uint32_t air = (uint32_t)m.air;
    cb_store_tile(m.dst, W, y0, x0, rows, cols, [&](int r, int e) {
      const uint32_t alpha = px[r * CB_COLS + e / 3];
      const uint32_t v = src[((int64_t)(y0 + r) * W + x0) * 3 + e];
      return (uint8_t)((v * (65536u - alpha) + air * alpha + 32768u) >> 16);
    });
  } else {  // rain
    const int len = m.len, slant = m.slant, fade = m.fade;
    const int far = ((len - 1) * slant) >> 3;  // the streak's last column offset; (k * slant) >> 3 is monotonic in k
    const int X0 = x0 + min(far, 0) + 4096, X1 = x0 + cols - 1 + max(far, 0) + 4096;
    const int g0 = X0 >> 2;
    const int ngroups = min((X1 >> 2) - g0 + 1, WX_RAIN_GROUPS), nrows = min(rows + len - 1, WX_RAIN_ROWS);
    const uint32_t thr = (uint32_t)m.thr;
    for (int i = tid; i < nrows * ngroups; i += CB_THREADS) {
      const int ry = i / ngroups, g = i - ry * ngroups;
      const uint4 w = philox(make_uint4((uint32_t)(g0 + g), (uint32_t)(y0 + ry), 0x5241494eu, 0u), key);
      const uint32_t f = (uint32_t)((w.x & 0xffffu) < thr) | (uint32_t)((w.y & 0xffffu) < thr) << 8 |
                         (uint32_t)((w.z & 0xffffu) < thr) << 16 | (uint32_t)((w.w & 0xffffu) < thr) << 24;
      *(uint32_t*)(aux + ry * WX_RAIN_STRIDE + g * 4) = f;
    }
    __syncthreads();
    const int base = x0 + 4096 - (g0 << 2);  // staged column of the tile's first pixel at offset 0
    for (int i = tid; i < rows * cols; i += CB_THREADS) {
      const int r = i / cols, xl = i - r * cols;
      int R = 0;
      for (int k = 0; k < len; ++k) {
        // the clamps never bind (X0, X1 span every offset) and keep every read inside the array
        const int col = min(max(base + xl + ((k * slant) >> 3), 0), WX_RAIN_STRIDE - 1);
        const int row = min(r + k, WX_RAIN_ROWS - 1);
        R = max(R, (int)aux[row * WX_RAIN_STRIDE + col] * (256 - k * fade));
      }
      px[r * CB_COLS + xl] = (uint16_t)R;
    }
    __syncthreads();
    const uint32_t beta = (uint32_t)m.beta;
    cb_store_tile(m.dst, W, y0, x0, rows, cols, [&](int r, int e) {
      const uint32_t R = px[r * CB_COLS + e / 3];
      const uint32_t v = src[((int64_t)(y0 + r) * W + x0) * 3 + e];
      return (uint8_t)(v + (((255u - v) * beta * R) >> 16));
    });
  }
}

static bool wx_overlap(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace mx

using namespace mx;

extern "C" int mx_weather_batch_tile(int32_t out[2]) {
  MX_CHECK_ARG(out != nullptr, "mx_weather_batch_tile: null output");
  out[0] = CB_ROWS;
  out[1] = CB_COLS;
  return MX_OK;
}

extern "C" int mx_weather_batch_u8(const mx_weather_desc* descs_host, int64_t n, const float* noise, mx_stream_t stream) {
  MX_CHECK_ARG(n >= 0 && (n == 0 || descs_host), "mx_weather_batch_u8: bad descriptor array");
  // every descriptor is checked before the first launch
  for (int64_t b = 0; b < n; ++b) {
    const mx_weather_desc& d = descs_host[b];
    MX_CHECK_ARG(d.op >= 1 && d.op <= 3, "mx_weather_batch_u8: image %lld: bad op %d", (long long)b, d.op);
    MX_CHECK_ARG(d.src && d.dst && d.H >= 1 && d.W >= 1 && d.H <= 32768 && d.W <= 32768,
                 "mx_weather_batch_u8: image %lld: null image or bad size %d x %d", (long long)b, d.H, d.W);
    const int64_t per = (int64_t)d.H * d.W * 3;
    if (d.src != d.dst)
      MX_CHECK_ARG(!wx_overlap(d.src, per, d.dst, per), "mx_weather_batch_u8: image %lld: src and dst overlap", (long long)b);
    if (d.op == 1)
      MX_CHECK_ARG(std::isfinite(d.gain) && std::isfinite(d.shot) && std::isfinite(d.read2) && d.gain >= 0.f &&
                       d.shot >= 0.f && d.read2 >= 0.f,
                   "mx_weather_batch_u8: image %lld: night parameters must be finite and >= 0", (long long)b);
    if (d.op == 2)
      MX_CHECK_ARG(0 <= d.lo && d.lo <= d.hi && d.hi <= 65535 && d.air >= 0 && d.air <= 255,
                   "mx_weather_batch_u8: image %lld: haze parameters outside 0 <= lo <= hi <= 65535, air 0..255",
                   (long long)b);
    if (d.op == 3)
      MX_CHECK_ARG(d.thr >= 0 && d.thr <= 65535 && d.len >= 1 && d.len <= WX_RAIN_LEN && d.slant >= -WX_RAIN_SLANT &&
                       d.slant <= WX_RAIN_SLANT && d.fade >= 0 && (d.len - 1) * (int64_t)d.fade < 256 && d.beta >= 0 &&
                       d.beta <= 256,
                   "mx_weather_batch_u8: image %lld: rain parameters outside thr 0..65535, len 1..32, slant -8..8, "
                   "0 <= (len-1)*fade < 256, beta 0..256",
                   (long long)b);
  }
  // no image's output may meet another image's input or output
  for (int64_t i = 0; i < n; ++i) {
    const mx_weather_desc& a = descs_host[i];
    const int64_t na = (int64_t)a.H * a.W * 3;
    for (int64_t j = 0; j < n; ++j) {
      if (j == i) continue;
      const mx_weather_desc& c = descs_host[j];
      const int64_t nc = (int64_t)c.H * c.W * 3;
      MX_CHECK_ARG(!wx_overlap(a.dst, na, c.src, nc), "mx_weather_batch_u8: output %lld overlaps input %lld", (long long)i,
                   (long long)j);
      if (j > i)
        MX_CHECK_ARG(!wx_overlap(a.dst, na, c.dst, nc), "mx_weather_batch_u8: outputs %lld and %lld overlap", (long long)i,
                     (long long)j);
    }
  }

  hipStream_t s = (hipStream_t)stream;
  WxChunk ck{};
  int64_t tiles = 0;
  auto flush = [&]() -> int {
    if (ck.n > 0 && tiles > 0) {
      weather_batch_kernel<<<(unsigned)tiles, CB_THREADS, 0, s>>>(ck);
      MX_LAUNCH_CHECK();
    }
    ck.n = 0;
    tiles = 0;
    return MX_OK;
  };
  int64_t noise_off = 0;
  for (int64_t b = 0; b < n; ++b) {
    const mx_weather_desc& d = descs_host[b];
    const int64_t my_noise = noise_off;
    noise_off += (int64_t)d.H * d.W * 3;
    const int64_t tx = cdiv(d.W, CB_COLS), tyn = cdiv(d.H, CB_ROWS);
    if (ck.n == WX_IMGS || tiles + tx * tyn > 0x7fffffff) {
      const int rc = flush();
      if (rc) return rc;
    }
    WxImg& m = ck.im[ck.n];
    m = WxImg{};
    m.src = d.src;
    m.dst = d.dst;
    m.noise = noise ? noise + my_noise : nullptr;
    m.seed = d.seed;
    m.H = d.H; m.W = d.W; m.op = d.op;
    m.gain = d.gain; m.shot = d.shot; m.read2 = d.read2;
    m.lo = d.lo; m.hi = d.hi; m.air = d.air;
    m.thr = d.thr; m.len = d.len; m.slant = d.slant; m.fade = d.fade; m.beta = d.beta;
    m.tile0 = (int32_t)tiles;
    m.tiles_x = (int32_t)tx;
    tiles += tx * tyn;
    ++ck.n;
  }
  return flush();
}
