// mx_boxcoder.h — BoxCoder.decode_single of one box (torchvision _utils.py; oracle orc_box_decode), shared
// by decode_kernel (mx_elementwise.hip) and det_candidates_kernel (mx_detect.hip) so both produce the
// same bits: every f32 op rounds once, in this order, whatever the flags of the file that inlines it.
#pragma once
#include <hip/hip_runtime.h>

namespace mx {

// b = reference box (x1, y1, x2, y2), r = (dx, dy, dw, dh), w = coder weights; dw / dh clamped at `clip`
__device__ __forceinline__ float4 decode_box(float4 b, float4 r, float4 w, float clip) {
#pragma clang fp contract(off)
  float widths = b.z - b.x, heights = b.w - b.y;
  float cx = b.x + 0.5f * widths, cy = b.y + 0.5f * heights;
  float dx = r.x / w.x, dy = r.y / w.y, dw = r.z / w.z, dh = r.w / w.w;
  dw = dw > clip ? clip : dw;
  dh = dh > clip ? clip : dh;
  float pcx = dx * widths + cx, pcy = dy * heights + cy;
  float pw = expf(dw) * widths, ph = expf(dh) * heights;
  float hw = 0.5f * pw, hh = 0.5f * ph;
  return make_float4(pcx - hw, pcy - hh, pcx + hw, pcy + hh);
}

}  // namespace mx
