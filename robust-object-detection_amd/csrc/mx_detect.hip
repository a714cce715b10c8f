// mx_detect.hip — detection postprocessing for every image of a batch (gfx950): the front half
// (softmax, box decode, clip, score / small-box filter) and the back half (top detections_per_img
// per image, rescale to the original image size) of torchvision RoIHeads.postprocess_detections +
// GeneralizedRCNNTransform.postprocess; the class-wise NMS between them is mx_batched_nms_grouped.
// Built -ffp-contract=off: every f32 op rounds once, in the order the header states.
#include "mx_common.h"
#include "mx_boxcoder.h"

namespace mx {

constexpr int DET_T = 256;          // threads per block: 4 waves, one RoI row per wave
constexpr int DET_ROWS = DET_T / 64;
constexpr int DET_CMAX = 1024;      // classes per row held in LDS (4 KiB per wave)

// torch.clamp(v, 0, hi) with scalar bounds (aten clamp_scalar_kernel_impl: NaN returned as is, else
// min(max(v, 0), hi)): +inf -> hi, -inf -> 0
__device__ __forceinline__ float clamp0(float v, float hi) { return v != v ? v : fminf(fmaxf(v, 0.f), hi); }

// One wave per row r. The row's C logits are read once (lane-strided), m = their maximum (exact, so
// its reduction order is free), e_j = expf(x_j - m) goes to the wave's LDS slice, and every lane adds
// the C values in ascending j -- the one summation order the result may have, independent of the
// launch geometry. Lane l then owns classes 1 + l, 65 + l, ...: consecutive dense slots t, so the four
// output streams are written coalesced.
__global__ void __launch_bounds__(DET_T)
det_candidates_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ reg, int64_t ldr,
                      const float4* __restrict__ rois, const int32_t* __restrict__ img, const float* __restrict__ hw,
                      int64_t R, int C, int N, float4 w, float clip, float score_thresh, float min_size,
                      float* __restrict__ scores, float4* __restrict__ boxes, int64_t* __restrict__ labels,
                      int32_t* __restrict__ grp) {
  __shared__ float e_s[DET_ROWS][DET_CMAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * DET_ROWS + wv;
  const bool row = r < R;  // no early return: every wave reaches the barrier
  float* e = e_s[wv];
  const float* x = logits + (row ? r : 0) * ldl;
  float m = -INFINITY;
  if (row)
    for (int j = lane; j < C; j += 64) m = fmaxf(m, x[j]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (row)
    for (int j = lane; j < C; j += 64) e[j] = expf(x[j] - m);
  __syncthreads();
  if (!row) return;
  float s = 0.f;
  for (int j = 0; j < C; ++j) s = s + e[j];
  const int im = img[r];
  const bool in_img = im >= 0 && im < N;
  const float h = in_img ? hw[2 * im] : 0.f, wd = in_img ? hw[2 * im + 1] : 0.f;
  const float4 roi = rois[r];
  for (int c = 1 + lane; c < C; c += 64) {
    const float p = e[c] / s;
    const float* q = reg + r * ldr + 4 * (int64_t)c;  // scalar loads: ldr need not keep 16-byte alignment
    float4 b = decode_box(roi, make_float4(q[0], q[1], q[2], q[3]), w, clip);
    if (in_img) b = make_float4(clamp0(b.x, wd), clamp0(b.y, h), clamp0(b.z, wd), clamp0(b.w, h));
    const int64_t t = r * (C - 1) + (c - 1);
    scores[t] = p;
    boxes[t] = b;
    labels[t] = c;
    // every comparison is false on NaN, as torch's: a NaN score or coordinate is dead
    const bool live = in_img && p > score_thresh && (b.z - b.x >= min_size) && (b.w - b.y >= min_size);
    grp[t] = live ? im : N;
  }
}

// One block per image n. keep[0:num_keep] is ordered by image, so the image's survivors are the run
// [lo, hi) found by two binary searches over grp[keep[i]]; slot d < min(hi - lo, D) takes survivor
// lo + d, the slots past it are zeroed. A keep entry outside [0, n) reads as dead (never
// dereferenced).
__device__ __forceinline__ int64_t det_lower_bound(const int64_t* __restrict__ keep, const int32_t* __restrict__ grp,
                                                   int64_t nk, int64_t n, int g) {
  int64_t lo = 0, hi = nk;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int64_t k = keep[mid];
    const int gm = (k >= 0 && k < n) ? grp[k] : 0x7fffffff;
    if (gm < g) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(DET_T)
det_select_kernel(const int64_t* __restrict__ keep, const int64_t* __restrict__ num_keep,
                  const float4* __restrict__ boxes, const float* __restrict__ scores,
                  const int64_t* __restrict__ labels, const int32_t* __restrict__ grp, int64_t n, int D,
                  const float* __restrict__ ratios, float4* __restrict__ out_boxes, float* __restrict__ out_scores,
                  int64_t* __restrict__ out_labels, int32_t* __restrict__ counts) {
  __shared__ int64_t lo_s;
  __shared__ int cnt_s;
  const int g = blockIdx.x;
  if (threadIdx.x == 0) {
    int64_t nk = *num_keep;
    const bool failed = nk < 0;
    nk = nk < 0 ? 0 : (nk > n ? n : nk);
    const int64_t lo = det_lower_bound(keep, grp, nk, n, g);
    const int64_t hi = det_lower_bound(keep, grp, nk, n, g + 1);
    const int cnt = (int)(hi - lo < D ? hi - lo : D);
    lo_s = lo;
    cnt_s = cnt;
    counts[g] = failed ? -1 : cnt;
  }
  __syncthreads();
  const int64_t lo = lo_s;
  const int cnt = cnt_s;
  float rh = 1.f, rw = 1.f;
  if (ratios) {
    rh = ratios[2 * g];
    rw = ratios[2 * g + 1];
  }
  for (int d = threadIdx.x; d < D; d += DET_T) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    int64_t l = 0;
    if (d < cnt) {
      const int64_t k = keep[lo + d];  // in [0, n): the search saw it as image g
      b = boxes[k];
      if (ratios) b = make_float4(b.x * rw, b.y * rh, b.z * rw, b.w * rh);
      s = scores[k];
      l = labels[k];
    }
    const int64_t o = (int64_t)g * D + d;
    out_boxes[o] = b;
    out_scores[o] = s;
    out_labels[o] = l;
  }
}

// ---- test-time augmentation: several views of each image fused by box voting ------------------
// Candidates of V views x N images (mx_det_candidates over V*N "images", P rows per block): slot
// t = ((v*N + i)*P + r)*(C-1) + (c-1). The fold brings every live slot into image i's frame and
// image group i; the voting select replaces each selected NMS survivor by the score-weighted mean
// of the candidates of its image and class that overlap it (Gidaris & Komodakis 2015).

// One thread per slot; per = P*(C-1) slots per (view, image) block. flips: bit v set = view v is
// mirrored horizontally. Reads its slot before it writes it, so out == in is fine.
__global__ void __launch_bounds__(DET_T)
det_views_fold_kernel(const float4* boxes, const int32_t* grp, const float* __restrict__ hw,
                      int64_t n, int64_t per, int N, uint64_t flips, float4* boxes_out, int32_t* grp_out) {
  const int64_t t = (int64_t)blockIdx.x * DET_T + threadIdx.x;
  if (t >= n) return;
  const int64_t b = t / per;
  const int v = (int)(b / N), i = (int)(b % N);
  float4 bx = boxes[t];
  const bool live = grp[t] == (int32_t)b;
  if (live && ((flips >> v) & 1)) {
    const float w = hw[2 * i + 1];
    bx = make_float4(w - bx.z, bx.y, w - bx.x, bx.w);
  }
  boxes_out[t] = bx;
  grp_out[t] = live ? i : N;
}

// torchvision box_iou of one pair in f32 (iou_tv of mx_match.hip): every operation rounds once
__device__ __forceinline__ float det_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }
__device__ __forceinline__ float det_iou(float4 a, float area_a, float4 b, float area_b) {
  const float ltx = fmaxf(a.x, b.x), lty = fmaxf(a.y, b.y);
  const float rbx = fminf(a.z, b.z), rby = fminf(a.w, b.w);
  float w = rbx - ltx, h = rby - lty;
  w = w < 0.f ? 0.f : w;
  h = h < 0.f ? 0.f : h;
  const float inter = w * h;
  return inter / ((area_a + area_b) - inter);
}

constexpr int VOTE_PER = DET_ROWS;  // output slots per block: one wave each

// Block (g, part) owns the output slots d = part*VOTE_PER + wave of image g; every block redoes the
// two searches of det_select_kernel (lanes 0 of waves 0 and 1, side by side). A wave with a survivor
// walks the V*P slots of its image and class in ascending slot order, 64 per round: the lanes test
// one candidate each, a ballot collects the voters, and every lane adds them in ascending bit order
// from broadcast values -- one f64 accumulation chain per sum, whatever the launch geometry. The
// next round's loads are issued before the current round's voters are added.
__global__ void __launch_bounds__(DET_T)
det_select_vote_kernel(const int64_t* __restrict__ keep, const int64_t* __restrict__ num_keep,
                       const float4* __restrict__ boxes, const float* __restrict__ scores,
                       const int64_t* __restrict__ labels, const int32_t* __restrict__ grp, int64_t n, int V, int N,
                       int P, int C, int D, int parts, bool vote, float vote_iou, const float* __restrict__ ratios,
                       float4* __restrict__ out_boxes, float* __restrict__ out_scores,
                       int64_t* __restrict__ out_labels, int32_t* __restrict__ counts) {
  __shared__ int64_t bound_s[2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = blockIdx.x / parts, part = blockIdx.x % parts;
  int64_t nk = *num_keep;
  const bool failed = nk < 0;
  nk = nk < 0 ? 0 : (nk > n ? n : nk);
  if (lane == 0 && wv < 2) bound_s[wv] = det_lower_bound(keep, grp, nk, n, g + wv);
  __syncthreads();
  const int64_t lo = bound_s[0], hi = bound_s[1];
  const int cnt = (int)(hi - lo < D ? hi - lo : D);
  if (part == 0 && threadIdx.x == 0) counts[g] = failed ? -1 : cnt;
  const int d = part * VOTE_PER + wv;  // wave-uniform
  if (d >= D) return;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  float s = 0.f;
  int64_t l = 0;
  if (d < cnt) {
    const int64_t k = keep[lo + d];  // in [0, n): the search saw it as image g
    b = boxes[k];
    s = scores[k];
    l = labels[k];
    if (vote && l >= 1 && l < C) {
      const float area_k = det_area(b);
      const int VP = V * P;  // <= n < 2^30
      // candidate j = v*P + r of this image and class: slot ((v*N + g)*P + r)*(C-1) + (l-1) < n
      auto slot = [&](int j) { return (((int64_t)(j / P) * N + g) * P + j % P) * (C - 1) + (l - 1); };
      float4 cb = make_float4(0.f, 0.f, 0.f, 0.f);
      float cs = 0.f;
      bool cl = false;
      if (lane < VP) {
        const int64_t t = slot(lane);
        cl = grp[t] == g;
        cb = boxes[t];
        cs = scores[t];
      }
      double ss = 0.0, sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
      bool any = false;
      for (int j0 = 0; j0 < VP; j0 += 64) {
        float4 nb = make_float4(0.f, 0.f, 0.f, 0.f);
        float ns = 0.f;
        bool nl = false;
        if (j0 + 64 + lane < VP) {
          const int64_t t = slot(j0 + 64 + lane);
          nl = grp[t] == g;
          nb = boxes[t];
          ns = scores[t];
        }
        // false on NaN: a NaN IoU never votes
        uint64_t hits = __ballot(cl && det_iou(b, area_k, cb, det_area(cb)) >= vote_iou);
        any |= hits != 0;
        while (hits) {
          const int src = __ffsll((unsigned long long)hits) - 1;
          hits &= hits - 1;
          const double w = (double)__shfl(cs, src);
          ss = ss + w;
          sx1 = sx1 + w * (double)__shfl(cb.x, src);  // f32 x f32 is exact in f64
          sy1 = sy1 + w * (double)__shfl(cb.y, src);
          sx2 = sx2 + w * (double)__shfl(cb.z, src);
          sy2 = sy2 + w * (double)__shfl(cb.w, src);
        }
        cb = nb;
        cs = ns;
        cl = nl;
      }
      if (any) b = make_float4((float)(sx1 / ss), (float)(sy1 / ss), (float)(sx2 / ss), (float)(sy2 / ss));
    }
    if (ratios) {
      const float rh = ratios[2 * g], rw = ratios[2 * g + 1];
      b = make_float4(b.x * rw, b.y * rh, b.z * rw, b.w * rh);
    }
  }
  if (lane == 0) {
    const int64_t o = (int64_t)g * D + d;
    out_boxes[o] = b;
    out_scores[o] = s;
    out_labels[o] = l;
  }
}

// n == V*N*P*(C-1) < 2^30 without overflow on the way
static bool det_views_sizes(int64_t n, int64_t V, int64_t N, int64_t P, int64_t C) {
  if (!(V >= 1 && V <= 64 && N >= 1 && N < (1ll << 31) && P >= 0 && P < (1ll << 30) && C >= 2 && C <= DET_CMAX))
    return false;
  if (P && V * N > (1ll << 30) / P) return false;  // V*N < 2^37: no overflow here or below
  return V * N * P * (C - 1) == n && n < (1ll << 30);
}

}  // namespace mx

using namespace mx;

extern "C" int mx_det_candidates(const float* logits, int64_t ldl, const float* reg, int64_t ldr, const float* rois,
                                 const int32_t* img, const float* hw, int64_t R, int64_t C, int64_t N,
                                 const float* weights4_host, float clip, float score_thresh, float min_size,
                                 float* scores, float* boxes, int64_t* labels, int32_t* grp, mx_stream_t stream) {
  MX_CHECK_ARG(R >= 0 && C >= 2 && C <= DET_CMAX && N >= 1 && N < (1ll << 31) && R * (C - 1) < (1ll << 30),
               "mx_det_candidates: bad sizes R=%lld C=%lld (2..%d) N=%lld", (long long)R, (long long)C, DET_CMAX,
               (long long)N);
  MX_CHECK_ARG(ldl >= C && ldr >= 4 * C, "mx_det_candidates: bad row strides ldl=%lld (>= C) ldr=%lld (>= 4C)",
               (long long)ldl, (long long)ldr);
  MX_CHECK_ARG(weights4_host, "mx_det_candidates: null weights");
  if (R == 0) return MX_OK;
  MX_CHECK_ARG(logits && reg && rois && img && hw && scores && boxes && labels && grp,
               "mx_det_candidates: null pointer");
  const float* w = weights4_host;
  det_candidates_kernel<<<(unsigned)cdiv(R, DET_ROWS), DET_T, 0, (hipStream_t)stream>>>(
      logits, ldl, reg, ldr, (const float4*)rois, img, hw, R, (int)C, (int)N, make_float4(w[0], w[1], w[2], w[3]), clip,
      score_thresh, min_size, scores, (float4*)boxes, labels, grp);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

extern "C" int mx_det_select(const int64_t* keep, const int64_t* num_keep, const float* boxes, const float* scores,
                             const int64_t* labels, const int32_t* grp, int64_t n, int64_t N, int64_t D,
                             const float* ratios, float* out_boxes, float* out_scores, int64_t* out_labels,
                             int32_t* counts, mx_stream_t stream) {
  MX_CHECK_ARG(n >= 0 && n < (1ll << 30) && N >= 1 && N < (1ll << 31) && D >= 1 && D < (1ll << 24),
               "mx_det_select: bad sizes n=%lld N=%lld D=%lld", (long long)n, (long long)N, (long long)D);
  MX_CHECK_ARG(num_keep && out_boxes && out_scores && out_labels && counts &&
                   (n == 0 || (keep && boxes && scores && labels && grp)),
               "mx_det_select: null pointer");
  det_select_kernel<<<(unsigned)N, DET_T, 0, (hipStream_t)stream>>>(keep, num_keep, (const float4*)boxes, scores, labels,
                                                                     grp, n, (int)D, ratios, (float4*)out_boxes,
                                                                     out_scores, out_labels, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

extern "C" int mx_det_views_fold(const float* boxes, const int32_t* grp, const float* hw, int64_t n, int64_t V,
                                 int64_t N, int64_t P, int64_t C, const int32_t* flip_host, float* boxes_out,
                                 int32_t* grp_out, mx_stream_t stream) {
  MX_CHECK_ARG(det_views_sizes(n, V, N, P, C),
               "mx_det_views_fold: bad sizes n=%lld (= V*N*P*(C-1) < 2^30) V=%lld (1..64) N=%lld P=%lld C=%lld (2..%d)",
               (long long)n, (long long)V, (long long)N, (long long)P, (long long)C, DET_CMAX);
  MX_CHECK_ARG(flip_host, "mx_det_views_fold: null flip flags");
  if (n == 0) return MX_OK;
  MX_CHECK_ARG(boxes && grp && hw && boxes_out && grp_out, "mx_det_views_fold: null pointer");
  uint64_t flips = 0;
  for (int v = 0; v < V; ++v) flips |= (uint64_t)(flip_host[v] != 0) << v;
  det_views_fold_kernel<<<(unsigned)cdiv(n, DET_T), DET_T, 0, (hipStream_t)stream>>>(
      (const float4*)boxes, grp, hw, n, P * (C - 1), (int)N, flips, (float4*)boxes_out, grp_out);
  MX_LAUNCH_CHECK();
  return MX_OK;
}

extern "C" int mx_det_select_vote(const int64_t* keep, const int64_t* num_keep, const float* boxes, const float* scores,
                                  const int64_t* labels, const int32_t* grp, int64_t n, int64_t V, int64_t N, int64_t P,
                                  int64_t C, int64_t D, double vote_iou, const float* ratios, float* out_boxes,
                                  float* out_scores, int64_t* out_labels, int32_t* counts, mx_stream_t stream) {
  MX_CHECK_ARG(det_views_sizes(n, V, N, P, C) && D >= 1 && D < (1ll << 24),
               "mx_det_select_vote: bad sizes n=%lld (= V*N*P*(C-1) < 2^30) V=%lld (1..64) N=%lld P=%lld C=%lld (2..%d) "
               "D=%lld",
               (long long)n, (long long)V, (long long)N, (long long)P, (long long)C, DET_CMAX, (long long)D);
  const int64_t parts = cdiv(D, VOTE_PER);
  MX_CHECK_ARG(N * parts < (1ll << 31), "mx_det_select_vote: N=%lld x D=%lld too large for one launch", (long long)N,
               (long long)D);
  MX_CHECK_ARG(num_keep && out_boxes && out_scores && out_labels && counts &&
                   (n == 0 || (keep && boxes && scores && labels && grp)),
               "mx_det_select_vote: null pointer");
  const float thr = (float)vote_iou;  // rounded once; > 1 or NaN: no voting, mx_det_select's result
  det_select_vote_kernel<<<(unsigned)(N * parts), DET_T, 0, (hipStream_t)stream>>>(
      keep, num_keep, (const float4*)boxes, scores, labels, grp, n, (int)V, (int)N, (int)P, (int)C, (int)D, (int)parts,
      thr <= 1.f, thr, ratios, (float4*)out_boxes, out_scores, out_labels, counts);
  MX_LAUNCH_CHECK();
  return MX_OK;
}
