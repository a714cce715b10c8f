// mx_pack.hip — per-step bf16 operand pack of the conv weights (wk / wt layouts, mx_conv_layout.h),
// alone (mx_conv_pack_weight, mx_conv_pack_batched) and fused with the optimizer update
// (mx_sgd_pack_step, mx_adamw_pack_step) on gfx950. Built with the flags of mx_optim.hip, so the fused
// and the multi-tensor updates (both from mx_common.h) produce the same bits.
#include "mx_common.h"
#include "mx_conv_layout.h"

#include <vector>

namespace mx {

// Two tile kinds, each with contiguous f32 reads and 128-B bf16 write runs (values staged in LDS as
// bf16, so the rounding is the one f2bf of the f32 master value):
//  * wk tile: kr whole output rows (cw input channels x all taps each; cw = Cpad unless one row
//    exceeds the LDS tile) -- a per-row [C][RS] -> [RS][Cpad] transpose, both sides contiguous;
//  * wt tile: 64 output channels x tct input channels x all taps -- read as 64 contiguous runs of
//    tct*RS floats, written along the innermost Kpad axis as output-channel pairs.
static constexpr int PACK_LDS = 25600;  // bf16 elements (50 KiB)
static constexpr int PK = 64;

__device__ __forceinline__ uint32_t fdiv(uint32_t a, uint32_t d, float inv) {  // a / d for a < 2^22
  uint32_t q = (uint32_t)((float)a * inv);
  if (q * d > a) --q;
  else if ((q + 1) * d <= a) ++q;
  return q;
}

__device__ __forceinline__ void st_bf2(uint16_t* d, uint16_t a, uint16_t b, bool two) {
  if (two && ((uintptr_t)d & 3) == 0) {
    *(uint32_t*)d = (uint32_t)a | ((uint32_t)b << 16);
  } else {
    d[0] = a;
    if (two) d[1] = b;
  }
}

// plane 0 (hi) / 1 (lo) of the bf16x3 split of an f32 weight
__device__ __forceinline__ uint16_t plane_bf(float v, int plane) {
  const uint16_t h = f2bf(v);
  return plane ? f2bf(v - bf2f(h)) : h;
}

// T[row * ldt + j] = bf16(w[(k0 + row) * C * RS + c0 * RS + j]) for j < n_valid (zero past the real
// input channels / output rows); ldt % 4 == 0. plane 1: the lo part bf16(w - bf16(w)).
__device__ __forceinline__ void pack_stage(const PackP& p, int64_t k0, int64_t c0, int rows, int width, int ldt,
                                           uint16_t* T, int plane) {
  const int RS = p.R * p.S;
  const int64_t cend = p.C < c0 + width / RS ? p.C : c0 + width / RS;
  const int nvalid = cend > c0 ? (int)((cend - c0) * RS) : 0;
  // U independent loads in flight per thread before the first LDS write (a load -> ds_write loop
  // would wait out the full memory latency once per element)
  constexpr int U = 8;
  if ((p.C & 3) == 0 && (c0 & 3) == 0 && (width & 3) == 0 && ((uintptr_t)p.w & 15) == 0) {
    // float4 path: every row run starts 16-B aligned and holds whole groups of 4
    const int w4 = width >> 2, total4 = rows * w4, nv4 = nvalid >> 2;
    const float inv4 = 1.f / (float)w4;
    for (int base = 0; base < total4; base += 256 * U) {
      float4 v[U];
      int dst[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = base + u * 256 + threadIdx.x;
        const int row = (int)fdiv((uint32_t)e, (uint32_t)w4, inv4), j4 = e - row * w4;
        const int64_t k = k0 + row;
        dst[u] = e < total4 ? row * ldt + 4 * j4 : -1;
        v[u] = (e < total4 && k < p.K && j4 < nv4) ? *(const float4*)(p.w + (k * p.C + c0) * RS + 4 * j4)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (dst[u] >= 0)
          *(uint2*)(T + dst[u]) =
              make_uint2((uint32_t)plane_bf(v[u].x, plane) | ((uint32_t)plane_bf(v[u].y, plane) << 16),
                         (uint32_t)plane_bf(v[u].z, plane) | ((uint32_t)plane_bf(v[u].w, plane) << 16));
    }
    __syncthreads();
    return;
  }
  const float inv = 1.f / (float)width;
  const int total = rows * width;
  for (int base = 0; base < total; base += 256 * U) {
    float v[U];
    int dst[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = base + u * 256 + threadIdx.x;
      const int row = (int)fdiv((uint32_t)e, (uint32_t)width, inv), j = e - row * width;
      const int64_t k = k0 + row;
      dst[u] = e < total ? row * ldt + j : -1;
      v[u] = (e < total && k < p.K && j < nvalid) ? p.w[(k * p.C + c0) * RS + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (dst[u] >= 0) T[dst[u]] = plane_bf(v[u], plane);
  }
  __syncthreads();
}

__device__ __forceinline__ void pack_wk_tile(const PackP& p, int64_t t, uint16_t* T, int plane) {
  const int RS = p.R * p.S;
  const int64_t nc = (p.Cpad + p.cw - 1) / p.cw;
  const int64_t k0 = (t / nc) * p.kr, c0 = (t % nc) * p.cw;
  const int cwv = (int)(p.Cpad - c0 < p.cw ? p.Cpad - c0 : p.cw);
  const int width = cwv * RS, ldt = width + 4;
  pack_stage(p, k0, c0, p.kr, width, ldt, T, plane);
  uint16_t* wk = p.wk + plane * p.wk_plane;
  const int h = (cwv + 1) >> 1, per = RS * h;  // channel pairs per (row, tap)
  const float inv_per = 1.f / (float)per, inv_h = 1.f / (float)h;
  for (int e = threadIdx.x; e < p.kr * per; e += 256) {
    const int row = (int)fdiv((uint32_t)e, (uint32_t)per, inv_per), rem = e - row * per;
    const int rs = (int)fdiv((uint32_t)rem, (uint32_t)h, inv_h), c2 = rem - rs * h;
    const int64_t k = k0 + row;
    if (k >= p.K) continue;
    const int cc = 2 * c2;
    const uint16_t* tt = T + row * ldt + cc * RS + rs;
    st_bf2(wk + (k * RS + rs) * p.Cpad + c0 + cc, tt[0], cc + 1 < cwv ? tt[RS] : (uint16_t)0, cc + 1 < cwv);
  }
}

__device__ __forceinline__ void pack_wt_tile(const PackP& p, int64_t t, uint16_t* T, int plane) {
  const int RS = p.R * p.S;
  const int64_t nc = (p.Cpad + p.tct - 1) / p.tct;
  const int64_t k0 = (t / nc) * PK, c0 = (t % nc) * p.tct;
  const int width = p.tct * RS, ldt = width + 4;
  pack_stage(p, k0, c0, PK, width, ldt, T, plane);
  uint16_t* wt = p.wt + plane * p.wt_plane;
  constexpr int PK2 = PK / 2;
  const int per = RS * PK2;
  const float inv_per = 1.f / (float)per;
  for (int e = threadIdx.x; e < p.tct * per; e += 256) {
    const int cc = (int)fdiv((uint32_t)e, (uint32_t)per, inv_per), rem = e - cc * per;
    const int rs = rem / PK2, k2 = rem % PK2;  // PK2 is a power of two
    const int64_t k = k0 + 2 * k2, c = c0 + cc;
    if (k >= p.Kpad || c >= p.Cpad) continue;
    const uint16_t* tt = T + 2 * k2 * ldt + cc * RS + rs;
    int64_t dst;
    if (p.dense) {  // [R][S][Cpad][Kpad]: the 1x1-GEMM dgrad operand of a conv whose output is 1x1
      dst = ((int64_t)rs * p.Cpad + c) * p.Kpad + k;
    } else {  // tap-parity class q (r % st_h, s % st_w): [c][r / st_h][s / st_w][Kpad]
      const int r = rs / p.S, sx = rs - r * p.S;
      const int q = (r % p.st_h) * p.st_w + (sx % p.st_w);
      dst = p.off[q] + ((c * p.Rc[q] + r / p.st_h) * p.Sc[q] + sx / p.st_w) * p.Kpad + k;
    }
    st_bf2(wt + dst, tt[0], tt[ldt], k + 1 < p.Kpad);
  }
}

// tiles: nwk wk tiles, then nwt wt tiles; a split job's block writes both planes of its tile, the
// second staging re-reading the f32 region it has just read (L2-hot) instead of another block
// fetching it from HBM again
__device__ __forceinline__ void pack_tile(const PackP& p, int64_t t) {
  __shared__ uint16_t T[PACK_LDS];
  const int np = p.split ? 2 : 1;
  for (int plane = 0; plane < np; ++plane) {
    if (plane) __syncthreads();  // the previous plane's writes have read T
    if (t < p.nwk) pack_wk_tile(p, t, T, plane);
    else pack_wt_tile(p, t - p.nwk, T, plane);
  }
}

__global__ void __launch_bounds__(256) pack_weight_kernel(PackP p) { pack_tile(p, blockIdx.x); }

// Every conv weight of a step in one launch: block -> (job, tile) through the tile prefix sums.
__global__ void __launch_bounds__(256) pack_batched_kernel(const PackP* __restrict__ jobs, const int64_t* __restrict__ prefix,
                                                           int njobs) {
  const int j = last_job(prefix, njobs, blockIdx.x);
  const PackP p = jobs[j];
  pack_tile(p, blockIdx.x - prefix[j]);
}

// ---------------------------------------------------------------------------------------------
// Optimizer step fused with the operand pack: a conv weight's update and its bf16 operand layouts in
// ONE pass (mx_sgd_pack_step, mx_adamw_pack_step), written once over the update rule R (SgdRule,
// AdamwRule: mx_common.h). The per-step order was the multi-tensor update (p, g, state -> p, state)
// and then pack_batched_kernel re-reading every updated f32 weight twice (wk tile, wt tile); here a
// block owns a kr x tc x (all taps) tile of w[K][C][R][S]: it updates the tile in registers (p and the
// state written back), keeps the (hi, lo) bf16 pair of each new weight in LDS as one u32, and writes
// both the wk and the wt layout from there. Each weight element is read once and written once per
// layout, as update + pack would produce it (same R::apply, same rounding). Non-conv parameters take
// the plain multi-tensor blocks (update_chunk) of the same launch.
template <typename R>
struct Job {
  float* p;
  float* s[R::NS];  // the rule's state arrays
  int64_t n;
  int first, fused;  // first: SGD's first momentum step (0 under other rules)
  int kr, tc;        // fused tile: kr output rows x tc input channels x all taps (powers of two)
  int64_t ncb;       // channel blocks (cdiv(Cpad, tc)) per row block
  PackP pk;          // fused: pk.w == p
};
static constexpr int SGDP_PER_BLOCK = UPDATE_PER_BLOCK;

__device__ __forceinline__ uint32_t hilo_word(float v) {  // bf16(v) | bf16(v - bf16(v)) << 16
  const uint16_t h = f2bf(v);
  return (uint32_t)h | ((uint32_t)f2bf(v - bf2f(h)) << 16);
}

// The wk and wt layouts of one kr x tc x (all taps) tile whose new weights sit in LDS as (hi, lo) bf16
// pairs (hilo_word), T[row * ldt + channel * RS + tap]; rows / channels past K / C hold 0.
__device__ __forceinline__ void tile_store_layouts(const PackP& pk, int kr, int tc, int64_t k0, int64_t c0,
                                                   const uint32_t* T, int ldt) {
  const int RS = pk.R * pk.S;
  const int np = pk.split ? 2 : 1;
  // 2. wk [K][R][S][Cpad]: runs of tc channels per (row, tap), written as channel pairs
  if (pk.wk) {
    const int h2 = tc >> 1, per = RS * h2;
    const float inv_per = 1.f / (float)per, inv_h = 1.f / (float)h2;
    for (int e = threadIdx.x; e < kr * per; e += 256) {
      const int row = (int)fdiv((uint32_t)e, (uint32_t)per, inv_per), rem = e - row * per;
      const int rs = (int)fdiv((uint32_t)rem, (uint32_t)h2, inv_h), c2 = rem - rs * h2;
      const int64_t k = k0 + row, c = c0 + 2 * c2;
      if (k >= pk.K || c >= pk.Cpad) continue;
      const uint32_t* tt = T + row * ldt + 2 * c2 * RS + rs;
      const uint32_t a = tt[0], a2 = tt[RS];  // Cpad is even: c + 1 < Cpad
      const int64_t dst = (k * RS + rs) * pk.Cpad + c;
      for (int pl = 0; pl < np; ++pl)
        *(uint32_t*)(pk.wk + pl * pk.wk_plane + dst) =
            pl ? (a >> 16) | (a2 & 0xffff0000u) : (a & 0xffffu) | (a2 << 16);
    }
  }
  // 3. wt (dgrad layout): runs along the output channels, written as output-channel pairs
  if (pk.wt) {
    const int kr2 = kr >> 1, per = RS * kr2;
    const float inv_per = 1.f / (float)per, inv_k = 1.f / (float)kr2;
    for (int e = threadIdx.x; e < tc * per; e += 256) {
      const int cc = (int)fdiv((uint32_t)e, (uint32_t)per, inv_per), rem = e - cc * per;
      const int rs = (int)fdiv((uint32_t)rem, (uint32_t)kr2, inv_k), k2 = rem - rs * kr2;
      const int64_t k = k0 + 2 * k2, c = c0 + cc;
      if (k >= pk.Kpad || c >= pk.Cpad) continue;
      const uint32_t* tt = T + 2 * k2 * ldt + cc * RS + rs;
      const uint32_t a = tt[0], a2 = tt[ldt];  // Kpad is even: k + 1 < Kpad
      int64_t dst;
      if (pk.dense) {
        dst = ((int64_t)rs * pk.Cpad + c) * pk.Kpad + k;
      } else {
        const int r = rs / pk.S, sx = rs - r * pk.S;
        const int q = (r % pk.st_h) * pk.st_w + (sx % pk.st_w);
        dst = pk.off[q] + ((c * pk.Rc[q] + r / pk.st_h) * pk.Sc[q] + sx / pk.st_w) * pk.Kpad + k;
      }
      for (int pl = 0; pl < np; ++pl)
        *(uint32_t*)(pk.wt + pl * pk.wt_plane + dst) =
            pl ? (a >> 16) | (a2 & 0xffff0000u) : (a & 0xffffu) | (a2 << 16);
    }
  }
}

template <typename R>
__device__ __forceinline__ void update_pack_tile(const Job<R>& J, const float* __restrict__ g, int64_t t,
                                                 const typename R::Hyper& h, const typename R::Tensor& c, uint32_t* T) {
  const PackP& pk = J.pk;
  const int RS = pk.R * pk.S;
  const int kr = J.kr, tc = J.tc;
  const int64_t k0 = (t / J.ncb) * kr, c0 = (t % J.ncb) * tc;
  const int width = tc * RS, ldt = width + 1;  // odd row stride: column reads spread over the banks
  const int64_t cend = pk.C < c0 + tc ? pk.C : c0 + tc;
  const int nvalid = cend > c0 ? (int)((cend - c0) * RS) : 0;
  // 1. update the tile: row k's run of nvalid weights starts at (k * C + c0) * RS
  if ((pk.C & 3) == 0 && update_aligned<R>(J.p, g, J.s)) {
    const int w4 = width >> 2, nv4 = nvalid >> 2;
    const float inv4 = 1.f / (float)w4;
    for (int e = threadIdx.x; e < kr * w4; e += 256) {
      const int row = (int)fdiv((uint32_t)e, (uint32_t)w4, inv4), j4 = e - row * w4;
      const int64_t k = k0 + row;
      uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
      if (k < pk.K && j4 < nv4) {
        float pv[4];
        update4<R>(J.p, g, J.s, (k * pk.C + c0) * RS + 4 * j4, h, c, pv);
        o0 = hilo_word(pv[0]); o1 = hilo_word(pv[1]); o2 = hilo_word(pv[2]); o3 = hilo_word(pv[3]);
      }
      uint32_t* d = T + row * ldt + 4 * j4;
      d[0] = o0; d[1] = o1; d[2] = o2; d[3] = o3;
    }
  } else {
    const float inv = 1.f / (float)width;
    for (int e = threadIdx.x; e < kr * width; e += 256) {
      const int row = (int)fdiv((uint32_t)e, (uint32_t)width, inv), j = e - row * width;
      const int64_t k = k0 + row;
      uint32_t o = 0;
      if (k < pk.K && j < nvalid) o = hilo_word(update1<R>(J.p, g, J.s, (k * pk.C + c0) * RS + j, h, c));
      T[row * ldt + j] = o;
    }
  }
  __syncthreads();
  tile_store_layouts(pk, kr, tc, k0, c0, T, ldt);
}

// The per-tensor constants of a job. SGD's first flag is the job's own (momentum buffers appear tensor
// by tensor); AdamW's bias corrections are the launch's: one launch serves a parameter group that
// shares one step number, so they are launch arguments beside the other constants.
__device__ __forceinline__ SgdRule::Tensor job_consts(const Job<SgdRule>& J, const SgdRule::Tensor&) { return {J.first}; }
__device__ __forceinline__ AdamwRule::Tensor job_consts(const Job<AdamwRule>&, const AdamwRule::Tensor& t) { return t; }

// block -> (job, tile or UPDATE_PER_BLOCK-element chunk) through the prefix sums; grads by job index
// (their pointers change more often than the job table)
template <typename R>
__device__ __forceinline__ void update_pack_block(const Job<R>* __restrict__ jobs, const int64_t* __restrict__ prefix,
                                                  const float* const* __restrict__ grads, int njobs,
                                                  const typename R::Hyper& h, const typename R::Tensor& t) {
  extern __shared__ uint32_t Tsm[];
  const int j = last_job(prefix, njobs, blockIdx.x);
  const Job<R> J = jobs[j];
  const int64_t b = blockIdx.x - prefix[j];
  if (J.fused) update_pack_tile<R>(J, grads[j], b, h, job_consts(J, t), Tsm);
  else update_chunk<R>(J.p, grads[j], J.s, J.n, b, h, job_consts(J, t));
}
// the two instantiations under the names profiles and tools know them by
__global__ void __launch_bounds__(256) sgd_pack_kernel(const Job<SgdRule>* __restrict__ jobs, const int64_t* __restrict__ prefix,
                                                       const float* const* __restrict__ grads, int njobs, SgdHyper h) {
  update_pack_block<SgdRule>(jobs, prefix, grads, njobs, h, SgdRule::Tensor{});
}
__global__ void __launch_bounds__(256) adamw_pack_kernel(const Job<AdamwRule>* __restrict__ jobs,
                                                         const int64_t* __restrict__ prefix,
                                                         const float* const* __restrict__ grads, int njobs,
                                                         AdamwHyper h, AdamwRule::Tensor t) {
  update_pack_block<AdamwRule>(jobs, prefix, grads, njobs, h, t);
}

// Host: tile sizes of one pack job (both tile kinds fit PACK_LDS, rows padded by 4 elements)
static int pack_plan(PackP& p) {
  const int RS = p.R * p.S;
  if (RS > 196) return MX_EINVAL;
  p.tct = RS == 1 ? 64 : (RS <= 9 ? 32 : ((392 / RS) & ~3));  // multiples of 4: float4 staging
  if (p.tct < 2) p.tct = 2;
  int64_t cw = p.Cpad;
  if (cw * RS + 4 > PACK_LDS) cw = ((PACK_LDS - 4) / RS) & ~3ll;
  p.cw = (int)cw;
  int64_t kr = 12288 / (cw * RS);
  if (kr > 64) kr = 64;
  while (kr > 1 && kr * (cw * RS + 4) > PACK_LDS) --kr;
  if (kr < 1) kr = 1;
  p.kr = (int)kr;
  p.nwk = p.wk ? cdiv(p.K, p.kr) * cdiv(p.Cpad, p.cw) : 0;
  p.nwt = p.wt ? cdiv(p.Kpad, (int64_t)PK) * cdiv(p.Cpad, (int64_t)p.tct) : 0;
  p.wk_plane = p.K * RS * p.Cpad;
  p.wt_plane = p.Cpad * RS * p.Kpad;
  return MX_OK;
}

}  // namespace mx

using namespace mx;

extern "C" int mx_conv_pack_weight(const mx_conv_shape* s, const float* w, int64_t Cin, int64_t Kout, uint16_t* wk,
                                   uint16_t* wt, int split, mx_stream_t stream) {
  // s->C / s->K are the padded channel counts the kernels see (Cin <= s->C real input channels,
  // Kout <= s->K real output channels of the f32 parameter w[Kout][Cin][R][S])
  MX_CHECK_ARG(s && w && s->R > 0 && s->S > 0 && Cin > 0 && Kout > 0 && Cin <= s->C && Kout <= s->K,
               "conv pack: bad shape");
  MX_CHECK_ARG(!wt || (s->stride_h >= 1 && s->stride_h <= 2 && s->stride_w >= 1 && s->stride_w <= 2),
               "conv pack: dgrad layout supports strides 1 and 2");
  if (!wk && !wt) return MX_OK;
  PackP p{};
  p.w = w; p.wk = wk; p.wt = wt;
  p.K = Kout; p.C = Cin; p.Cpad = s->C; p.Kpad = s->K;
  p.R = (int)s->R; p.S = (int)s->S; p.st_h = s->stride_h; p.st_w = s->stride_w;
  if (wt) {
    DClass cl[4];
    dgrad_classes(s, s->C, s->K, cl, p.off, p.Rc, p.Sc);
  } else {
    p.st_h = p.st_w = 1;
  }
  // wk covers Kout rows only; wt also covers the zero-padded output channels up to s->K
  MX_CHECK_ARG(pack_plan(p) == MX_OK, "conv pack: at most 196 taps");
  p.split = split ? 1 : 0;
  const int64_t tiles = p.nwk + p.nwt;
  MX_CHECK_ARG(tiles < (1ll << 31), "conv pack: too many tiles");
  pack_weight_kernel<<<(unsigned)tiles, 256, 0, (hipStream_t)stream>>>(p);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

static int make_pack(const mx_pack_desc& d, PackP& p, int64_t& tiles) {
  MX_CHECK_ARG(d.w && d.R > 0 && d.S > 0 && d.Cin > 0 && d.Kout > 0 && d.Cin <= d.Cpad && d.Kout <= d.Kpad,
               "conv pack: bad job");
  MX_CHECK_ARG(!d.wt || (d.stride_h >= 1 && d.stride_h <= 2 && d.stride_w >= 1 && d.stride_w <= 2),
               "conv pack: dgrad layout supports strides 1 and 2");
  p = PackP{};
  p.w = d.w; p.wk = d.wk; p.wt = d.wt;
  p.K = d.Kout; p.C = d.Cin; p.Cpad = d.Cpad; p.Kpad = d.Kpad;
  p.R = d.R; p.S = d.S; p.st_h = d.stride_h; p.st_w = d.stride_w;
  p.dense = d.flags & 1;
  p.split = (d.flags >> 1) & 1;
  if (d.wt && !p.dense) {
    mx_conv_shape s{};
    s.C = d.Cpad; s.K = d.Kpad; s.R = d.R; s.S = d.S; s.H = 1; s.W = 1;
    s.stride_h = d.stride_h; s.stride_w = d.stride_w; s.pad_h = d.pad_h; s.pad_w = d.pad_w;
    DClass cl[4];
    dgrad_classes(&s, d.Cpad, d.Kpad, cl, p.off, p.Rc, p.Sc);
  } else {
    p.st_h = p.st_w = 1;
  }
  MX_CHECK_ARG(pack_plan(p) == MX_OK, "conv pack: at most 196 taps");
  tiles = p.nwk + p.nwt;
  return MX_OK;
}

extern "C" size_t mx_conv_pack_plan_bytes(int64_t njobs) {
  return njobs > 0 ? sizeof(PackP) * (size_t)njobs + sizeof(int64_t) * (size_t)(njobs + 1) : 0;
}

extern "C" int mx_conv_pack_batched(const mx_pack_desc* jobs, int64_t njobs, void* plan, size_t plan_bytes, int upload,
                                    mx_stream_t stream) {
  MX_CHECK_ARG(jobs && njobs > 0 && njobs < (1 << 20), "conv pack batched: bad job list");
  MX_CHECK_ARG(plan && plan_bytes >= mx_conv_pack_plan_bytes(njobs), "conv pack batched: plan buffer too small");
  std::vector<PackP> host((size_t)njobs);
  std::vector<int64_t> prefix((size_t)njobs + 1, 0);
  for (int64_t j = 0; j < njobs; ++j) {
    int64_t t = 0;
    int rc = make_pack(jobs[j], host[(size_t)j], t);
    if (rc) return rc;
    if (!jobs[j].wk && !jobs[j].wt) t = 0;
    prefix[(size_t)j + 1] = prefix[(size_t)j] + t;
  }
  const int64_t total = prefix[(size_t)njobs];
  MX_CHECK_ARG(total < (1ll << 31), "conv pack batched: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  PackP* dj = (PackP*)plan;
  int64_t* dp = (int64_t*)((char*)plan + sizeof(PackP) * (size_t)njobs);
  if (upload) {
    // the host vectors die with this call: synchronous copies (the plan changes rarely)
    MX_HIP(hipStreamSynchronize(st));
    MX_HIP(hipMemcpy(dj, host.data(), sizeof(PackP) * (size_t)njobs, hipMemcpyHostToDevice));
    MX_HIP(hipMemcpy(dp, prefix.data(), sizeof(int64_t) * (size_t)(njobs + 1), hipMemcpyHostToDevice));
  }
  if (total == 0) return MX_OK;
  pack_batched_kernel<<<(unsigned)total, 256, 0, st>>>(dj, dp, (int)njobs);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

// fused tile for R*S taps (update_pack_tile): 64x64 (1x1), 32x32 (<= 9 taps), 16x8 (<= 49 taps; FC6).
// One launch reserves the largest tile's LDS for every block: FC6's 16x16 (50 KiB) held the whole
// launch to 3 blocks per CU; 16x8 (25 KiB) leaves the 3x3 tile (37 KiB) as the bound (4 per CU).
static bool sgd_tile(int RS, int& kr, int& tc) {
  if (RS == 1) { kr = 64; tc = 64; return true; }
  if (RS <= 9) { kr = 32; tc = 32; return true; }
  if (RS <= 49) { kr = 16; tc = 8; return true; }
  return false;
}

// One fused job of mx_sgd_pack_build / mx_adamw_pack_build (`who` in the messages): parameter j (p, n
// elements) as packs[pack] -> its PackP, tile, channel blocks per row block, block count; lds grows
// to the tile's (hi, lo) words, rows padded by one
static int fused_job(const char* who, const mx_pack_desc* packs, int32_t pack, int64_t j, const float* p, int64_t n,
                     PackP& pk, int& kr, int& tc, int64_t& ncb, int64_t& nb, size_t& lds) {
  MX_CHECK_ARG(packs, "%s pack build: pack index without pack list", who);
  const mx_pack_desc& d = packs[pack];
  int64_t tiles = 0;
  int rc = make_pack(d, pk, tiles);
  if (rc) return rc;
  const int RS = d.R * d.S;
  MX_CHECK_ARG(d.w == p && d.Kout * d.Cin * RS == n, "%s pack build: pack %lld is not parameter %lld", who,
               (long long)pack, (long long)j);
  MX_CHECK_ARG(sgd_tile(RS, kr, tc), "%s pack build: %d taps (fused packing takes <= 49)", who, RS);
  MX_CHECK_ARG(d.wk || d.wt, "%s pack build: pack %lld has no layout", who, (long long)pack);
  ncb = cdiv(pk.Cpad, tc);
  nb = cdiv(pk.Kpad, kr) * ncb;
  const size_t need = sizeof(uint32_t) * (size_t)kr * (size_t)(tc * RS + 1);
  if (need > lds) lds = need;
  return MX_OK;
}

// The plan of a fused launch (opaque to callers): nparams jobs, then nparams + 1 block prefix sums
template <typename R>
static size_t plan_bytes(int64_t nparams) {
  return nparams > 0 ? sizeof(Job<R>) * (size_t)nparams + sizeof(int64_t) * (size_t)(nparams + 1) : 0;
}
template <typename R>
static const int64_t* plan_prefix(const void* plan, int64_t nparams) {
  return (const int64_t*)((const char*)plan + sizeof(Job<R>) * (size_t)nparams);
}

// mx_sgd_pack_build / mx_adamw_pack_build (`who` in the messages) over their parameter struct P;
// state(q, j, J) checks parameter j's rule-specific fields and copies them into its job
template <typename R, typename P, typename F>
static int pack_build(const char* who, const P* params, int64_t nparams, const mx_pack_desc* packs, void* host_plan,
                      size_t plan_bytes_, int64_t* blocks, size_t* lds_bytes, F state) {
  MX_CHECK_ARG(params && nparams > 0 && nparams < (1 << 20) && blocks && lds_bytes, "%s pack build: bad lists", who);
  MX_CHECK_ARG(host_plan && plan_bytes_ >= plan_bytes<R>(nparams), "%s pack build: plan buffer too small", who);
  Job<R>* jobs = (Job<R>*)host_plan;
  int64_t* prefix = (int64_t*)plan_prefix<R>(host_plan, nparams);
  prefix[0] = 0;
  size_t lds = 0;
  for (int64_t j = 0; j < nparams; ++j) {
    const P& q = params[j];
    Job<R> J{};
    int rc = state(q, j, J);
    if (rc) return rc;
    J.p = q.p; J.n = q.n;
    int64_t nb = cdiv(q.n, SGDP_PER_BLOCK);
    if (q.pack >= 0) {
      rc = fused_job(who, packs, q.pack, j, q.p, q.n, J.pk, J.kr, J.tc, J.ncb, nb, lds);
      if (rc) return rc;
      J.fused = 1;
    }
    jobs[j] = J;
    prefix[j + 1] = prefix[j] + nb;
  }
  MX_CHECK_ARG(prefix[nparams] < (1ll << 31), "%s pack build: too many blocks", who);
  *blocks = prefix[nparams];
  *lds_bytes = lds;
  return MX_OK;
}

extern "C" size_t mx_sgd_pack_plan_bytes(int64_t nparams) { return plan_bytes<SgdRule>(nparams); }

extern "C" int mx_sgd_pack_build(const mx_sgd_param* params, int64_t nparams, const mx_pack_desc* packs,
                                 void* host_plan, size_t plan_bytes, int64_t* blocks, size_t* lds_bytes) {
  return pack_build<SgdRule>("sgd", params, nparams, packs, host_plan, plan_bytes, blocks, lds_bytes,
                             [](const mx_sgd_param& q, int64_t j, Job<SgdRule>& J) -> int {
    MX_CHECK_ARG(q.p && q.buf && q.n > 0, "sgd pack build: parameter %lld empty or null", (long long)j);
    J.s[0] = q.buf; J.first = q.first ? 1 : 0;
    return MX_OK;
  });
}

extern "C" int mx_sgd_pack_step(const void* plan, const float* const* grads, int64_t nparams, int64_t blocks,
                                size_t lds_bytes, float lr, float momentum, float dampening, float weight_decay,
                                int nesterov, mx_stream_t stream) {
  MX_CHECK_ARG(plan && grads && nparams > 0 && blocks > 0 && blocks < (1ll << 31) && lds_bytes <= 65536,
               "sgd pack step: bad plan");
  SgdHyper h{lr, momentum, dampening, weight_decay, nesterov};
  sgd_pack_kernel<<<(unsigned)blocks, 256, lds_bytes, (hipStream_t)stream>>>(
      (const Job<SgdRule>*)plan, plan_prefix<SgdRule>(plan, nparams), grads, (int)nparams, h);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

extern "C" size_t mx_adamw_pack_plan_bytes(int64_t nparams) { return plan_bytes<AdamwRule>(nparams); }

// the conventions and the tile choice (fused_job, sgd_tile) of mx_sgd_pack_build
extern "C" int mx_adamw_pack_build(const mx_adamw_param* params, int64_t nparams, const mx_pack_desc* packs,
                                   void* host_plan, size_t plan_bytes, int64_t* blocks, size_t* lds_bytes) {
  return pack_build<AdamwRule>("adamw", params, nparams, packs, host_plan, plan_bytes, blocks, lds_bytes,
                               [](const mx_adamw_param& q, int64_t j, Job<AdamwRule>& J) -> int {
    MX_CHECK_ARG(q.p && q.exp_avg && q.exp_avg_sq && q.n > 0, "adamw pack build: parameter %lld empty or null",
                 (long long)j);
    MX_CHECK_ARG(q.reserved == 0, "adamw pack build: parameter %lld has reserved != 0", (long long)j);
    J.s[0] = q.exp_avg; J.s[1] = q.exp_avg_sq;
    return MX_OK;
  });
}

extern "C" int mx_adamw_pack_step(const void* plan, const float* const* grads, int64_t nparams, int64_t blocks,
                                  size_t lds_bytes, int64_t step, double lr, double beta1, double beta2, double eps,
                                  double weight_decay, mx_stream_t stream) {
  MX_CHECK_ARG(plan && grads && nparams > 0 && blocks > 0 && blocks < (1ll << 31) && lds_bytes <= 65536,
               "adamw pack step: bad plan");
  MX_CHECK_ARG(step >= 1, "adamw pack step: step %lld (the step number after this step, >= 1)", (long long)step);
  MX_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adamw pack step: betas outside [0, 1)");
  MX_CHECK_ARG(eps >= 0.0, "adamw pack step: negative eps");
  AdamwRule::Tensor t{};
  adamw_bias(lr, beta1, beta2, step, t.step_size, t.bc2_sqrt);
  adamw_pack_kernel<<<(unsigned)blocks, 256, lds_bytes, (hipStream_t)stream>>>(
      (const Job<AdamwRule>*)plan, plan_prefix<AdamwRule>(plan, nparams), grads, (int)nparams,
      adamw_hyper(lr, beta1, beta2, eps, weight_decay), t);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
