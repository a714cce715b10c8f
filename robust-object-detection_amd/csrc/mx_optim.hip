// mx_optim.hip — multi-tensor SGD (momentum, weight decay) and AdamW, one launch per 64 tensors (gfx950).
//
// torch.optim.SGD semantics (the reference: SGD(params, lr=0.005, momentum=0.9, weight_decay=5e-4),
// scripts/train_frcnn_baseline.py:149-153, step at :176):
//   d = g + wd * p;  buf = first ? d : momentum * buf + (1 - dampening) * d;
//   d = nesterov ? d + momentum * buf : buf;  p -= lr * d
// Replaces the three multi_tensor_apply launches (plus their host-side grouping) of torch's foreach
// path with one streaming pass: 20 B of HBM traffic per parameter (p, g, buf read; p, buf written).
// The element updates, the update rules and the streaming body (update_chunk) are in mx_common.h,
// shared with the forms fused with the conv operand pack (mx_pack.hip).
#include "mx_common.h"

namespace mx {

static constexpr int SGD_CHUNK = 64;  // tensors per launch (kernel-argument struct < 4 KiB)

struct SgdArgs {
  float* p[SGD_CHUNK];
  const float* g[SGD_CHUNK];
  float* buf[SGD_CHUNK];
  int64_t n[SGD_CHUNK];
  int32_t first_block[SGD_CHUNK + 1];  // prefix of blocks per tensor
  uint64_t first_mask;                 // bit t: tensor t takes its first momentum step
  int count;
  SgdHyper h;
};

// block -> tensor t with first_block[t] <= block < first_block[t + 1], then its chunk of t
__global__ void __launch_bounds__(256) sgd_kernel(SgdArgs a) {
  const int t = last_job(a.first_block, a.count, blockIdx.x);
  float* const s[1] = {a.buf[t]};
  update_chunk<SgdRule>(a.p[t], a.g[t], s, a.n[t], blockIdx.x - a.first_block[t], a.h,
                        SgdRule::Tensor{(int)((a.first_mask >> t) & 1ull)});
}

// torch.optim.AdamW (the reference: AdamW(lr=1e-3, weight_decay=1e-4), train_restoration.py:246, step
// at :272; adamw_update in mx_common.h). Replaces torch's foreach path (several multi_tensor_apply
// launches over the ~70 tensors of the U-Net plus host-side grouping) with one streaming pass: 28 B of
// HBM traffic per parameter (p, g, m, v read; p, m, v written). The bias corrections depend on each
// tensor's own step number, so they travel per tensor.
static constexpr int ADAMW_CHUNK = 64;  // tensors per launch: 52 B each, the struct stays < 4 KiB

struct AdamwArgs {
  float* p[ADAMW_CHUNK];
  const float* g[ADAMW_CHUNK];
  float* m[ADAMW_CHUNK];
  float* v[ADAMW_CHUNK];
  int64_t n[ADAMW_CHUNK];
  int32_t first_block[ADAMW_CHUNK + 1];
  float step_size[ADAMW_CHUNK], bc2_sqrt[ADAMW_CHUNK];
  AdamwHyper h;
  int count;
};
static_assert(sizeof(AdamwArgs) <= 4096, "kernel-argument struct");

__global__ void __launch_bounds__(256) adamw_kernel(AdamwArgs a) {
  const int t = last_job(a.first_block, a.count, blockIdx.x);
  float* const s[2] = {a.m[t], a.v[t]};
  update_chunk<AdamwRule>(a.p[t], a.g[t], s, a.n[t], blockIdx.x - a.first_block[t], a.h,
                          AdamwRule::Tensor{a.step_size[t], a.bc2_sqrt[t]});
}

}  // namespace mx

using namespace mx;

extern "C" int mx_sgd_step(float* const* params, const float* const* grads, float* const* bufs, const int64_t* numels,
                           const uint8_t* first, int64_t count, float lr, float momentum, float dampening,
                           float weight_decay, int nesterov, mx_stream_t stream) {
  MX_CHECK_ARG(count >= 0 && (count == 0 || (params && grads && bufs && numels && first)), "sgd_step: bad tensor lists");
  for (int64_t c0 = 0; c0 < count; c0 += SGD_CHUNK) {
    SgdArgs a{};
    a.count = (int)std::min<int64_t>(SGD_CHUNK, count - c0);
    a.h = SgdHyper{lr, momentum, dampening, weight_decay, nesterov};
    int64_t blocks = 0;
    for (int i = 0; i < a.count; ++i) {
      const int64_t j = c0 + i;
      MX_CHECK_ARG(params[j] && grads[j] && bufs[j] && numels[j] > 0, "sgd_step: tensor %lld empty or null", (long long)j);
      a.p[i] = params[j]; a.g[i] = grads[j]; a.buf[i] = bufs[j]; a.n[i] = numels[j];
      if (first[j]) a.first_mask |= 1ull << i;
      a.first_block[i] = (int32_t)blocks;
      blocks += cdiv(numels[j], UPDATE_PER_BLOCK);
      MX_CHECK_ARG(blocks < (1ll << 31), "sgd_step: too many elements");
    }
    a.first_block[a.count] = (int32_t)blocks;
    sgd_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}

extern "C" int mx_adamw_step(float* const* params, const float* const* grads, float* const* exp_avgs,
                             float* const* exp_avg_sqs, const int64_t* numels, const int64_t* steps, int64_t count,
                             double lr, double beta1, double beta2, double eps, double weight_decay,
                             mx_stream_t stream) {
  MX_CHECK_ARG(count >= 0 && (count == 0 || (params && grads && exp_avgs && exp_avg_sqs && numels && steps)),
               "adamw_step: bad tensor lists");
  MX_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adamw_step: betas outside [0, 1)");
  MX_CHECK_ARG(eps >= 0.0, "adamw_step: negative eps");
  for (int64_t j = 0; j < count; ++j) {  // every argument before the first launch
    MX_CHECK_ARG(params[j] && grads[j] && exp_avgs[j] && exp_avg_sqs[j] && numels[j] > 0,
                 "adamw_step: tensor %lld empty or null", (long long)j);
    MX_CHECK_ARG(steps[j] >= 1, "adamw_step: tensor %lld has step %lld (the step number after this step, >= 1)",
                 (long long)j, (long long)steps[j]);
  }
  for (int64_t c0 = 0; c0 < count; c0 += ADAMW_CHUNK) {
    AdamwArgs a{};
    a.count = (int)std::min<int64_t>(ADAMW_CHUNK, count - c0);
    a.h = adamw_hyper(lr, beta1, beta2, eps, weight_decay);
    int64_t blocks = 0;
    for (int i = 0; i < a.count; ++i) {
      const int64_t j = c0 + i;
      a.p[i] = params[j]; a.g[i] = grads[j]; a.m[i] = exp_avgs[j]; a.v[i] = exp_avg_sqs[j]; a.n[i] = numels[j];
      adamw_bias(lr, beta1, beta2, steps[j], a.step_size[i], a.bc2_sqrt[i]);
      a.first_block[i] = (int32_t)blocks;
      blocks += cdiv(numels[j], UPDATE_PER_BLOCK);
      MX_CHECK_ARG(blocks < (1ll << 31), "adamw_step: too many elements");
    }
    a.first_block[a.count] = (int32_t)blocks;
    adamw_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
    MX_LAUNCH_CHECK();
  }
  return MX_OK;
}
