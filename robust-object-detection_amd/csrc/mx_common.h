// mx_common.h — shared helpers for the libmx_det HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mx_det.h"

namespace mx {

void set_error(const char* fmt, ...);

#define MX_CHECK_ARG(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      ::mx::set_error(__VA_ARGS__);        \
      return MX_EINVAL;                    \
    }                                      \
  } while (0)

#define MX_HIP(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      ::mx::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return MX_EHIP;                                                             \
    }                                                                             \
  } while (0)

#define MX_LAUNCH_CHECK() MX_HIP(hipGetLastError())

// bf16 helpers (bit-level; round-to-nearest-even like v_cvt_pk_bf16_f32)
// XCD-aware bijective remap of a linear block id (cdna_hip_programming.md §5 / T1): the blocks one
// XCD receives (id % 8) get one contiguous run of work indices, in dispatch order
__device__ __forceinline__ int64_t xcd_remap(int64_t id, int64_t nwg) {
  if (nwg < 8) return id;
  int64_t q = nwg / 8, r = nwg % 8, xcd = id % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + id / 8;
}

__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

template <typename T> struct io;
template <> struct io<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct io<uint16_t> {
  static __device__ __forceinline__ float ld(const uint16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st(uint16_t* p, float v) { *p = f2bf(v); }
};

// 8 consecutive activation elements of storage type T (bf16 bits or f32) <-> float[8]: one 16-B
// access for bf16, two for f32 (NHWC rows are 8-element aligned everywhere: C % 8 == 0)
template <typename T>
__device__ __forceinline__ void ld8(const T* p, float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    const uint4 u = *(const uint4*)p;
    const uint16_t* h = (const uint16_t*)&u;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = bf2f(h[q]);
  } else {
    *(float4*)&v[0] = *(const float4*)p;
    *(float4*)&v[4] = *(const float4*)(p + 4);
  }
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    uint4 u;
    uint16_t* h = (uint16_t*)&u;
#pragma unroll
    for (int q = 0; q < 8; ++q) h[q] = f2bf(v[q]);
    *(uint4*)p = u;
  } else {
    *(float4*)p = *(const float4*)&v[0];
    *(float4*)(p + 4) = *(const float4*)&v[4];
  }
}
// storage element as stored (no rounding when T is f32)
template <typename T>
__device__ __forceinline__ float ld1(const T* p) {
  if constexpr (sizeof(T) == 2) return bf2f(*p);
  else return *p;
}
template <typename T>
__device__ __forceinline__ void st1(T* p, float v) {
  if constexpr (sizeof(T) == 2) *p = f2bf(v);
  else *p = v;
}

// bf16x3 split of f32 operands (precision-faithful conv mode): x = hi + lo + O(2^-17 |x|), hi = RNE
// bf16(x), lo = RNE bf16(x - hi); products hi*hi + hi*lo + lo*hi in f32 accumulation differ from the
// f32 product by O(2^-16) relative (TF32 rounds each operand to 2^-11). One v_cvt_pk_bf16_f32 per
// pair and plane.
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
  typedef float f2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 b2_t __attribute__((ext_vector_type(2)));
  const b2_t r = __builtin_convertvector((f2_t){a, b}, b2_t);
  return __builtin_bit_cast(uint32_t, r);
}
// scalar v_sub_f32: plain `a - b` pairs get SLP-packed into v_pk_add_f32, which costs ~13 extra
// cycles per instruction beside MFMAs (MI355X_MICROARCH.md, filler prices)
__device__ __forceinline__ float sub_f32(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pk_bf16(a, b);
  const float ha = __uint_as_float(hi << 16), hb = __uint_as_float(hi & 0xffff0000u);
  lo = pk_bf16(sub_f32(a, ha), sub_f32(b, hb));
}
// 8 f32 -> 8 bf16 hi (16 B) + 8 bf16 lo (16 B)
__device__ __forceinline__ void split8(const float4 a, const float4 b, uint4& hi, uint4& lo) {
  split2(a.x, a.y, hi.x, lo.x);
  split2(a.z, a.w, hi.y, lo.y);
  split2(b.x, b.y, hi.z, lo.z);
  split2(b.z, b.w, hi.w, lo.w);
}

// host: call F<uint16_t> (MX_BF16) or F<float> (MX_F32) with the arguments; other codes -> MX_EINVAL
#define MX_DT_DISPATCH(dt, F, ...)                                   \
  do {                                                              \
    MX_CHECK_ARG((dt) == MX_BF16 || (dt) == MX_F32, "bad dtype %d", (int)(dt)); \
    if ((dt) == MX_BF16) F<uint16_t>(__VA_ARGS__);                  \
    else F<float>(__VA_ARGS__);                                     \
  } while (0)

// torch.optim.SGD's update of one element (scripts/train_frcnn_baseline.py:149-153):
//   d = g + wd * p;  buf = first ? d : momentum * buf + (1 - dampening) * d;
//   d = nesterov ? d + momentum * buf : buf;  p -= lr * d
// Shared by sgd_kernel (mx_optim.hip) and the pack-fused sgd_pack_kernel (mx_pack.hip), both built with
// the same flags, so the two paths produce the same bits.
__device__ __forceinline__ float sgd_update(float& p, float g, float& b, bool first, float lr, float momentum,
                                            float dampening, float wd, int nesterov) {
  // explicit fused multiply-adds: the same rounding in every kernel that inlines this, whatever
  // contraction the compiler would pick around it
  const float d = __fmaf_rn(wd, p, g);
  b = first ? d : __fmaf_rn(momentum, b, __fmul_rn(1.f - dampening, d));
  const float u = nesterov ? __fmaf_rn(momentum, b, d) : b;
  p = __fmaf_rn(-lr, u, p);
  return p;
}

// torch.optim.AdamW's update of one element (decoupled decay, no amsgrad, no maximize; the reference's
// AdamW(lr 1e-3, weight_decay 1e-4), train_restoration.py:246, step at :272), in torch's op order:
//   p *= decay;  m += w1 * (g - m);  v = v * b2 + w2 * (g * g);
//   d = sqrt(v) / bc2_sqrt + eps;  p -= step_size * (m / d)
// The constants are derived on the host in double (adamw_hyper / adamw_bias below: decay = 1 - lr*wd,
// w1 = 1 - beta1, b2 = beta2, w2 = 1 - beta2, bc2_sqrt = sqrt(1 - beta2^step), step_size =
// lr / (1 - beta1^step)) and rounded to f32 once. Every f32 op
// rounds once: no contraction in here, whatever the flags of the file that inlines it, so
// adamw_kernel (mx_optim.hip) and the pack-fused adamw_pack_kernel (mx_pack.hip) produce the same
// bits. Division and square root are the IEEE-rounded ones.
struct AdamwHyper {
  float decay, w1, b2, w2, eps;
};
__device__ __forceinline__ void adamw_update(float& p, float g, float& m, float& v, const AdamwHyper& h,
                                             float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
  const float pd = p * h.decay;
  const float dm = g - m;
  const float mn = m + h.w1 * dm;
  const float g2 = g * g;
  const float vb = v * h.b2;
  const float vn = vb + h.w2 * g2;
  const float d = __fsqrt_rn(vn) / bc2_sqrt + h.eps;
  const float q = mn / d;
  p = pd - step_size * q;
  m = mn;
  v = vn;
}
// Host: the f32 constants of adamw_update from double hyper-parameters, as torch derives them from
// Python floats (pow as Python's float ** float)
inline AdamwHyper adamw_hyper(double lr, double beta1, double beta2, double eps, double wd) {
  return AdamwHyper{(float)(1.0 - lr * wd), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
}
inline void adamw_bias(double lr, double beta1, double beta2, int64_t step, float& step_size, float& bc2_sqrt) {
  step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
  bc2_sqrt = (float)pow(1.0 - pow(beta2, (double)step), 0.5);
}

// An update rule names what one optimizer's kernels differ in: NS state arrays, the constants of a
// launch (Hyper) and of a tensor (Tensor), and apply() = the element update above. The multi-tensor
// kernels (mx_optim.hip) and the pack-fused ones (mx_pack.hip) are written once over a rule R; the
// state is indexed by unrolled constants only, so it lives in registers.
struct SgdHyper {
  float lr, momentum, dampening, wd;
  int nesterov;
};
struct SgdRule {
  static constexpr int NS = 1;  // buf
  typedef SgdHyper Hyper;
  struct Tensor {
    int first;  // the tensor takes its first momentum step
  };
  static __device__ __forceinline__ void apply(float& p, float g, float (&s)[NS], const Hyper& h, const Tensor& t) {
    sgd_update(p, g, s[0], t.first, h.lr, h.momentum, h.dampening, h.wd, h.nesterov);
  }
};
struct AdamwRule {
  static constexpr int NS = 2;  // exp_avg, exp_avg_sq
  typedef AdamwHyper Hyper;
  struct Tensor {
    float step_size, bc2_sqrt;
  };
  static __device__ __forceinline__ void apply(float& p, float g, float (&s)[NS], const Hyper& h, const Tensor& t) {
    adamw_update(p, g, s[0], s[1], h, t.step_size, t.bc2_sqrt);
  }
};

// p, g and every state array 16-B aligned: the float4 forms below may be used
template <typename R>
__device__ __forceinline__ bool update_aligned(const float* p, const float* g, float* const (&s)[R::NS]) {
  uintptr_t bits = (uintptr_t)p | (uintptr_t)g;
#pragma unroll
  for (int k = 0; k < R::NS; ++k) bits |= (uintptr_t)s[k];
  return (bits & 15u) == 0;
}
// element i (update1) / elements i .. i + 3 as float4s (update4) of p and the state arrays updated in
// place with gradient g; the new parameter value(s) are handed back
template <typename R>
__device__ __forceinline__ float update1(float* p, const float* g, float* const (&s)[R::NS], int64_t i,
                                         const typename R::Hyper& h, const typename R::Tensor& t) {
  float pv = p[i], sv[R::NS];
#pragma unroll
  for (int k = 0; k < R::NS; ++k) sv[k] = s[k][i];
  R::apply(pv, g[i], sv, h, t);
  p[i] = pv;
#pragma unroll
  for (int k = 0; k < R::NS; ++k) s[k][i] = sv[k];
  return pv;
}
template <typename R>
__device__ __forceinline__ void update4(float* p, const float* g, float* const (&s)[R::NS], int64_t i,
                                        const typename R::Hyper& h, const typename R::Tensor& t, float (&pv)[4]) {
  float gv[4], sv[R::NS][4];
  *(float4*)pv = *(const float4*)(p + i);
#pragma unroll
  for (int k = 0; k < R::NS; ++k) *(float4*)sv[k] = *(const float4*)(s[k] + i);
  *(float4*)gv = *(const float4*)(g + i);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float sq[R::NS];
#pragma unroll
    for (int k = 0; k < R::NS; ++k) sq[k] = sv[k][q];
    R::apply(pv[q], gv[q], sq, h, t);
#pragma unroll
    for (int k = 0; k < R::NS; ++k) sv[k][q] = sq[k];
  }
  *(float4*)(p + i) = *(const float4*)pv;
#pragma unroll
  for (int k = 0; k < R::NS; ++k) *(float4*)(s[k] + i) = *(const float4*)sv[k];
}

// The streaming body of every multi-tensor update: block blk of a 256-thread launch takes elements
// [blk * UPDATE_PER_BLOCK, +UPDATE_PER_BLOCK) of an n-element tensor, as float4s when every pointer
// is 16-B aligned (then a scalar tail), else element by element.
static constexpr int UPDATE_PER_BLOCK = 2048;
template <typename R>
__device__ __forceinline__ void update_chunk(float* p, const float* __restrict__ g, float* const (&s)[R::NS], int64_t n,
                                             int64_t blk, const typename R::Hyper& h, const typename R::Tensor& t) {
  const int64_t e0 = blk * UPDATE_PER_BLOCK, e1 = min<int64_t>(n, e0 + UPDATE_PER_BLOCK);
  if (update_aligned<R>(p, g, s)) {
    float pv[4];
    for (int64_t e = e0 + threadIdx.x * 4; e + 3 < e1; e += 256 * 4) update4<R>(p, g, s, e, h, t, pv);
    const int64_t tail = e0 + ((e1 - e0) & ~(int64_t)3);
    for (int64_t e = tail + threadIdx.x; e < e1; e += 256) update1<R>(p, g, s, e, h, t);
  } else {
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) update1<R>(p, g, s, e, h, t);
  }
}

// Block -> job through prefix sums: the last j < n with prefix[j] <= b (prefix[0] == 0)
template <typename T>
__device__ __forceinline__ int last_job(const T* prefix, int n, int64_t b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Carves a caller-owned workspace into aligned slabs.
struct Carver {
  char* base;
  size_t cap, off = 0;
  Carver(void* b, size_t c) : base((char*)b), cap(c) {}
  template <typename T> T* take(size_t count) {
    size_t o = align_up(off);
    off = o + sizeof(T) * count;
    return base ? (T*)(base + o) : nullptr;
  }
  bool ok() const { return off <= cap; }
};

}  // namespace mx
