// mx_coco.hip — COCOeval (bbox) matching and accumulation on the device: pycocotools' computeIoU +
// evaluateImg and accumulate as mx_det/coco.py restates them (the metric behind
// train_frcnn_baseline.py:92-96 and eval_all.py:131-156). All arithmetic is f64 and follows the host
// code operation by operation; built -ffp-contract=off (EXACT_SRC) so a box area never fuses into
// the union's sum. Results are bit-identical to mx_det.coco.COCOeval (tests/test_gpu_coco_device.py).
#include "mx_common.h"

namespace mx {

// ---------------------------------------------------------------------------------------------
// Matching. One wave per (segment, area range, IoU threshold); a segment is one (image, category)
// pair. evaluateImg visits the GTs non-ignored first, then ignored, each group in annotation order,
// and keeps a running best that an equal IoU replaces; it stops at the first ignored GT once a
// non-ignored one is matched. So a detection's match is the arg-max over the still-available GTs
// with IoU >= min(t, 1 - 1e-10) of the key (non-ignored, IoU, annotation index): lanes stride the
// GTs (any count), a butterfly reduces the key. IoUs are recomputed per detection from the boxes (no
// D x G matrix); the only per-GT state is one flag byte in LDS.
// ---------------------------------------------------------------------------------------------
static constexpr int kFlagIgnore = 1, kFlagCrowd = 2, kFlagMatched = 4;
static constexpr int64_t kMaxSegGt = 61440;  // flag bytes of one segment in LDS (60 KiB)

__global__ __launch_bounds__(64) void coco_match_kernel(
    const double* __restrict__ dt_xywh, const double* __restrict__ dt_area, const int32_t* __restrict__ dt_off, int64_t ND,
    const double* __restrict__ gt_xywh, const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_crowd,
    const int64_t* __restrict__ gt_id, const int32_t* __restrict__ gt_off, int64_t NG, const double* __restrict__ area_rng,
    int A, const double* __restrict__ iou_thr, int T, int max_g, int64_t* __restrict__ dtm, uint8_t* __restrict__ dt_ig,
    uint8_t* __restrict__ gt_ig) {
  extern __shared__ __attribute__((aligned(16))) uint8_t flags[];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int t = (int)(b % T), a = (int)((b / T) % A);
  const int64_t s = b / ((int64_t)T * A);
  // offsets are device data the host cannot check: clamp so a bad table cannot index out of bounds
  const int64_t d0 = min(max((int64_t)dt_off[s], (int64_t)0), ND), d1 = min(max((int64_t)dt_off[s + 1], d0), ND);
  const int64_t g0 = min(max((int64_t)gt_off[s], (int64_t)0), NG), g1 = min(max((int64_t)gt_off[s + 1], g0), NG);
  const int G = (int)(g1 - g0), D = (int)(d1 - d0);
  const double a0 = area_rng[2 * a], a1 = area_rng[2 * a + 1];
  int64_t* dtm_o = dtm + ((int64_t)a * T + t) * ND + d0;
  uint8_t* dig_o = dt_ig + ((int64_t)a * T + t) * ND + d0;
  if (G > max_g) {  // the caller's bound was wrong: mark the segment, never truncate it
    for (int d = lane; d < D; d += 64) {
      dtm_o[d] = -1;
      dig_o[d] = 1;
    }
    if (t == 0)
      for (int g = lane; g < G; g += 64) gt_ig[(int64_t)a * NG + g0 + g] = 1;
    return;
  }
  for (int g = lane; g < G; g += 64) {
    const bool crowd = gt_crowd[g0 + g] != 0;
    const double ar = gt_area[g0 + g];
    const bool ig = crowd || ar < a0 || ar > a1;
    flags[g] = (uint8_t)((ig ? kFlagIgnore : 0) | (crowd ? kFlagCrowd : 0));
    if (t == 0) gt_ig[(int64_t)a * NG + g0 + g] = ig ? 1 : 0;
  }
  __syncthreads();
  const double tv = iou_thr[t], cap = 1 - 1e-10;
  const double thr0 = tv <= cap ? tv : cap;
  for (int d = 0; d < D; ++d) {
    const double* db = dt_xywh + 4 * (d0 + d);
    const double dx1 = db[0], dy1 = db[1], dw = db[2], dh = db[3];
    const double dx2 = dx1 + dw, dy2 = dy1 + dh, da = dw * dh;
    int bk = 0, bg = -1;  // bk: 0 none, 1 an ignored GT, 2 a non-ignored GT
    double bi = 0.0;
    for (int g = lane; g < G; g += 64) {
      const int f = flags[g];
      if ((f & kFlagMatched) && !(f & kFlagCrowd)) continue;
      const double* gb = gt_xywh + 4 * (g0 + g);
      const double gx1 = gb[0], gy1 = gb[1], gw = gb[2], gh = gb[3];
      const double gx2 = gx1 + gw, gy2 = gy1 + gh, ga = gw * gh;
      const double w = (dx2 < gx2 ? dx2 : gx2) - (dx1 > gx1 ? dx1 : gx1);
      const double h = (dy2 < gy2 ? dy2 : gy2) - (dy1 > gy1 ? dy1 : gy1);
      const double inter = (w > 0 && h > 0) ? w * h : 0.0;
      const double uni = (f & kFlagCrowd) ? da : (da + ga) - inter;
      const double iou = inter / uni;
      if (!(iou >= thr0)) continue;  // a 0/0 IoU never matches
      const int kc = (f & kFlagIgnore) ? 1 : 2;
      if (kc > bk || (kc == bk && iou >= bi)) {
        bk = kc;
        bi = iou;
        bg = g;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int ok = __shfl_xor(bk, o), og = __shfl_xor(bg, o);
      const double oi = __shfl_xor(bi, o);
      if (ok > bk || (ok == bk && (oi > bi || (oi == bi && og > bg)))) {
        bk = ok;
        bi = oi;
        bg = og;
      }
    }
    if (lane == 0) {
      int64_t id = 0;
      int ig = 0;
      if (bk) {
        id = gt_id[g0 + bg];
        ig = flags[bg] & kFlagIgnore;
        flags[bg] |= kFlagMatched;
      }
      // accumulate reads dtm == 0 as unmatched, a match to GT id 0 included (pycocotools' quirk)
      const double ar = dt_area[d0 + d];
      if (id == 0 && (ar < a0 || ar > a1)) ig = 1;
      dtm_o[d] = id;
      dig_o[d] = (uint8_t)ig;
    }
    __syncthreads();
  }
}

// rank[i] = position of detection i inside its segment (the segment is score-descending)
__global__ __launch_bounds__(64) void coco_rank_kernel(const int32_t* __restrict__ dt_off, int64_t ND, int32_t* __restrict__ rank) {
  const int64_t s = blockIdx.x;
  const int64_t d0 = min(max((int64_t)dt_off[s], (int64_t)0), ND), d1 = min(max((int64_t)dt_off[s + 1], d0), ND);
  for (int64_t i = d0 + threadIdx.x; i < d1; i += 64) rank[i] = (int32_t)(i - d0);
}

// ---------------------------------------------------------------------------------------------
// Accumulation. One block per (category, area range, maxDet, IoU threshold). Pass 1 scans the
// category's detections in score order (perm) for the running tp / fp counts and records, for every
// recall threshold, the first detection whose recall tp / npig reaches it (searchsorted left): only a
// true positive (or the first detection) can be such a position, and it serves the thresholds in
// (recall before, recall at]. Pass 2 repeats the scan and takes the maximum precision of each stretch
// between two recorded positions; the precision envelope at a position (the host's running maximum
// from the right) is the maximum over its own and all later stretches. max is exact, so the order of
// the reduction does not matter.
// ---------------------------------------------------------------------------------------------
static constexpr int kAccThreads = 256;
static constexpr int64_t kMaxRecThr = 2048;

__device__ __forceinline__ unsigned long long wave_scan(unsigned long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// first index r in [0, n) with v[r] > x (v ascending)
__device__ __forceinline__ int upper_bound_f64(const double* v, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ int upper_bound_i32(const int32_t* v, int n, int32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kAccThreads) void coco_accumulate_kernel(
    const int64_t* __restrict__ dtm, const uint8_t* __restrict__ dt_ig, const uint8_t* __restrict__ gt_ig,
    const double* __restrict__ dt_score, const int64_t* __restrict__ perm, const int32_t* __restrict__ rank, int64_t ND,
    int64_t NG, const int32_t* __restrict__ cat_dt_off, const int32_t* __restrict__ cat_gt_off, int K, int A, int T,
    const int32_t* __restrict__ max_dets, int M, const double* __restrict__ rec_thr, int R, double* __restrict__ precision,
    double* __restrict__ scores, double* __restrict__ recall) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // carve (every offset a multiple of 16): thr[R] f64 | ss[R] f64 | bmax[R] u64 | pos[R] i32 | wsum[2][4] u64 | cnt
  const int R2 = (R + 1) & ~1, R4 = (R + 3) & ~3;
  double* thr = (double*)smem;
  double* ss = thr + R2;
  unsigned long long* bmax = (unsigned long long*)(ss + R2);
  int32_t* pos = (int32_t*)(bmax + R2);
  unsigned long long* wsum = (unsigned long long*)(pos + R4);
  int32_t* cnt = (int32_t*)(wsum + 8);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int t = (int)(b % T), m = (int)((b / T) % M), a = (int)((b / ((int64_t)T * M)) % A);
  const int k = (int)(b / ((int64_t)T * M * A));
  const int64_t c0 = min(max((int64_t)cat_dt_off[k], (int64_t)0), ND), c1 = min(max((int64_t)cat_dt_off[k + 1], c0), ND);
  const int64_t h0 = min(max((int64_t)cat_gt_off[k], (int64_t)0), NG), h1 = min(max((int64_t)cat_gt_off[k + 1], h0), NG);
  if (tid == 0) *cnt = 0;
  for (int r = tid; r < R; r += kAccThreads) {
    thr[r] = rec_thr[r];
    ss[r] = 0.0;
    bmax[r] = 0ull;
    pos[r] = INT32_MAX;
  }
  __syncthreads();
  int c = 0;
  for (int64_t g = h0 + tid; g < h1; g += kAccThreads) c += gt_ig[(int64_t)a * NG + g] == 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0 && c) atomicAdd(cnt, c);
  __syncthreads();
  const int npig = *cnt;
  const int64_t KAM = (int64_t)K * A * M, kam = ((int64_t)k * A + a) * M + m;
  if (npig == 0) {  // the host's `continue`: a category without GT, or with ignored GT only
    for (int r = tid; r < R; r += kAccThreads) {
      precision[((int64_t)t * R + r) * KAM + kam] = -1.0;
      scores[((int64_t)t * R + r) * KAM + kam] = -1.0;
    }
    if (tid == 0) recall[(int64_t)t * KAM + kam] = -1.0;
    return;
  }
  const double np = (double)npig;
  const int md = max_dets[m];
  const int64_t* dtm_i = dtm + ((int64_t)a * T + t) * ND;
  const uint8_t* dig_i = dt_ig + ((int64_t)a * T + t) * ND;
  unsigned long long tp_total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    unsigned long long carry = 0, carry_v = 0;  // carry: tp in the low word, fp in the high word
    for (int64_t base = c0; base < c1; base += kAccThreads) {
      const int64_t j = base + tid;
      unsigned long long x = 0, v = 0;
      int64_t i = 0;
      if (j < c1) {
        i = perm[j];
        if ((uint64_t)i < (uint64_t)ND && rank[i] < md) {
          v = 1;
          const bool matched = dtm_i[i] != 0, ig = dig_i[i] != 0;
          if (!ig) x = matched ? 1ull : (1ull << 32);
        }
      }
      const bool is_tp = (x & 1ull) != 0;
      const unsigned long long valid = v;
      x = wave_scan(x, lane);
      v = wave_scan(v, lane);
      if (lane == 63) {
        wsum[wave] = x;
        wsum[4 + wave] = v;
      }
      __syncthreads();
      unsigned long long tot = 0, tot_v = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) {
          x += wsum[w];
          v += wsum[4 + w];
        }
        tot += wsum[w];
        tot_v += wsum[4 + w];
      }
      x += carry;
      v += carry_v;
      carry += tot;
      carry_v += tot_v;
      const unsigned long long tp = x & 0xffffffffull, fp = x >> 32;
      if (valid) {
        if (pass == 0) {
          if (is_tp || v == 1) {
            const double rc = (double)tp / np;
            const int r_lo = v == 1 ? 0 : upper_bound_f64(thr, R, (double)(tp - 1) / np);
            const int r_hi = upper_bound_f64(thr, R, rc);
            const double sc = dt_score[i];
            for (int r = r_lo; r < r_hi; ++r) {
              pos[r] = (int32_t)(j - c0);
              ss[r] = sc;
            }
          }
        } else {
          const double pr = (double)tp / (((double)fp + (double)tp) + 2.220446049250313e-16);
          const int bin = upper_bound_i32(pos, R, (int32_t)(j - c0)) - 1;
          if (bin >= 0) atomicMax(&bmax[bin], (unsigned long long)__double_as_longlong(pr));  // pr >= 0: bit order
        }
      }
      __syncthreads();
    }
    tp_total = carry & 0xffffffffull;
    __syncthreads();
  }
  if (tid == 0) recall[(int64_t)t * KAM + kam] = (double)tp_total / np;  // no detections: 0
  for (int r = tid; r < R; r += kAccThreads) {
    double q = 0.0, sc = 0.0;
    if (pos[r] != INT32_MAX) {  // thresholds past the last detection's recall keep 0
      unsigned long long best = 0;
      for (int r2 = r; r2 < R; ++r2) best = bmax[r2] > best ? bmax[r2] : best;
      q = __longlong_as_double((long long)best);
      sc = ss[r];
    }
    precision[((int64_t)t * R + r) * KAM + kam] = q;
    scores[((int64_t)t * R + r) * KAM + kam] = sc;
  }
}

}  // namespace mx

using namespace mx;

extern "C" int mx_coco_match(const double* dt_xywh, const double* dt_area, const int32_t* dt_off, int64_t ND,
                             const double* gt_xywh, const double* gt_area, const uint8_t* gt_crowd, const int64_t* gt_id,
                             const int32_t* gt_off, int64_t NG, int64_t S, const double* area_rng, int64_t A,
                             const double* iou_thr, int64_t T, int64_t max_g, int64_t max_d, int64_t* dtm, uint8_t* dt_ig,
                             uint8_t* gt_ig, mx_stream_t stream) {
  MX_CHECK_ARG(ND >= 0 && NG >= 0 && S >= 0 && A >= 1 && T >= 1 && max_g >= 0 && max_d >= 0,
               "mx_coco_match: bad sizes ND=%lld NG=%lld S=%lld A=%lld T=%lld max_g=%lld max_d=%lld", (long long)ND,
               (long long)NG, (long long)S, (long long)A, (long long)T, (long long)max_g, (long long)max_d);
  MX_CHECK_ARG(ND < INT32_MAX && NG < INT32_MAX && S < INT32_MAX && max_g <= NG && max_d <= ND,
               "mx_coco_match: counts above the int32 offsets or bounds above the totals");
  MX_CHECK_ARG(A <= 65535 && T <= 65535 && S * A * T < INT32_MAX, "mx_coco_match: S*A*T too large for one grid");
  if (max_g > kMaxSegGt) {
    set_error("mx_coco_match: %lld GT in one (image, category) segment, limit %lld", (long long)max_g,
              (long long)kMaxSegGt);
    return MX_EUNSUPPORTED;
  }
  if (S == 0) return MX_OK;
  MX_CHECK_ARG(dt_off && gt_off && area_rng && iou_thr && (ND == 0 || (dt_xywh && dt_area && dtm && dt_ig)) &&
                   (NG == 0 || (gt_xywh && gt_area && gt_crowd && gt_id && gt_ig)),
               "mx_coco_match: null pointer");
  const size_t lds = align_up((size_t)(max_g > 0 ? max_g : 1), 16);
  coco_match_kernel<<<(unsigned)(S * A * T), 64, lds, (hipStream_t)stream>>>(
      dt_xywh, dt_area, dt_off, ND, gt_xywh, gt_area, gt_crowd, gt_id, gt_off, NG, area_rng, (int)A, iou_thr, (int)T,
      (int)max_g, dtm, dt_ig, gt_ig);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

extern "C" size_t mx_coco_accumulate_workspace(int64_t ND) {
  Carver c(nullptr, 0);
  c.take<int32_t>(ND > 0 ? ND : 1);  // rank of each detection in its segment
  return c.off;
}

extern "C" int mx_coco_accumulate(const int64_t* dtm, const uint8_t* dt_ig, const uint8_t* gt_ig, const double* dt_score,
                                  const int64_t* perm, const int32_t* dt_off, int64_t S, int64_t ND, int64_t NG,
                                  const int32_t* cat_dt_off, const int32_t* cat_gt_off, int64_t K, int64_t A, int64_t T,
                                  const int32_t* max_dets, int64_t M, const double* rec_thr, int64_t R,
                                  double* precision, double* scores, double* recall, void* ws, size_t ws_bytes,
                                  mx_stream_t stream) {
  MX_CHECK_ARG(ND >= 0 && NG >= 0 && S >= 0 && K >= 0 && A >= 1 && T >= 1 && M >= 1 && R >= 0,
               "mx_coco_accumulate: bad sizes ND=%lld NG=%lld S=%lld K=%lld A=%lld T=%lld M=%lld R=%lld", (long long)ND,
               (long long)NG, (long long)S, (long long)K, (long long)A, (long long)T, (long long)M, (long long)R);
  MX_CHECK_ARG(ND < INT32_MAX && NG < INT32_MAX && S < INT32_MAX, "mx_coco_accumulate: counts above the int32 offsets");
  MX_CHECK_ARG(K <= 65535 && A <= 65535 && T <= 65535 && M <= 65535 && K * A * M * T < INT32_MAX,
               "mx_coco_accumulate: K*A*M*T too large for one grid");
  if (R > kMaxRecThr) {
    set_error("mx_coco_accumulate: %lld recall thresholds, limit %lld", (long long)R, (long long)kMaxRecThr);
    return MX_EUNSUPPORTED;
  }
  MX_CHECK_ARG(ws_bytes >= mx_coco_accumulate_workspace(ND), "mx_coco_accumulate: workspace too small");
  if (K == 0) return MX_OK;
  MX_CHECK_ARG(ws && cat_dt_off && cat_gt_off && max_dets && precision && scores && recall && (R == 0 || rec_thr) &&
                   (S == 0 || dt_off) && (ND == 0 || (dtm && dt_ig && dt_score && perm)) && (NG == 0 || gt_ig),
               "mx_coco_accumulate: null pointer");
  hipStream_t s = (hipStream_t)stream;
  Carver c(ws, ws_bytes);
  int32_t* rank = c.take<int32_t>(ND > 0 ? ND : 1);
  if (S > 0 && ND > 0) {
    coco_rank_kernel<<<(unsigned)S, 64, 0, s>>>(dt_off, ND, rank);
    MX_LAUNCH_CHECK();
  }
  const size_t R2 = (size_t)((R + 1) & ~(int64_t)1), R4 = (size_t)((R + 3) & ~(int64_t)3);
  const size_t lds = R2 * 24 + R4 * 4 + 8 * 8 + 16;
  coco_accumulate_kernel<<<(unsigned)(K * A * M * T), kAccThreads, lds, s>>>(
      dtm, dt_ig, gt_ig, dt_score, perm, rank, ND, NG, cat_dt_off, cat_gt_off, (int)K, (int)A, (int)T, max_dets, (int)M,
      rec_thr, (int)R, precision, scores, recall);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
