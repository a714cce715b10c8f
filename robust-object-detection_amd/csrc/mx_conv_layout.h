// mx_conv_layout.h — the weight-operand layouts the conv kernels (mx_conv.hip) read and the pack
// kernels (mx_pack.hip) write: the stride-parity classes of the dgrad operand, and the pack job.
#pragma once
#include "mx_common.h"

namespace mx {

// dgrad stride-parity classes. dx(h) receives dy((h + pad - r) / st) only from taps with
// r = (h + pad) mod st, so the rows with h = st*hh + ph form an independent dense GEMM over the
// taps r = r0 + st*ri (r0 = (ph + pad) mod st): dx[n, st*hh+ph] = sum dy[n, hh + dh - ri] w_t[ri],
// dh = (ph + pad - r0) / st. The classes partition both dx and the taps; wt stores each tap-parity
// class's [C][Rc][Sc][K] block contiguously (block index = tap parity r0*st_w + s0).
struct DClass {
  int ph, pw, r0, s0, Rc, Sc, dh, dw;
  int64_t Hc, Wc, off;
};
static int tap_count(int R, int r0, int st) { return r0 < R ? (R - r0 + st - 1) / st : 0; }
static int dgrad_classes(const mx_conv_shape* s, int64_t Cpad, int64_t Kpad, DClass* out, int64_t* blk_off,
                         int* blk_R, int* blk_S) {
  const int sh = s->stride_h, sw = s->stride_w;
  // block offsets by tap parity
  int64_t off = 0;
  for (int a = 0; a < sh; ++a)
    for (int b = 0; b < sw; ++b) {
      const int q = a * sw + b;
      blk_R[q] = tap_count((int)s->R, a, sh);
      blk_S[q] = tap_count((int)s->S, b, sw);
      blk_off[q] = off;
      off += Cpad * blk_R[q] * blk_S[q] * Kpad;
    }
  int n = 0;
  for (int ph = 0; ph < sh; ++ph)
    for (int pw = 0; pw < sw; ++pw) {
      DClass c;
      c.ph = ph; c.pw = pw;
      c.r0 = (ph + s->pad_h) % sh; c.s0 = (pw + s->pad_w) % sw;
      const int q = c.r0 * sw + c.s0;
      c.Rc = blk_R[q]; c.Sc = blk_S[q]; c.off = blk_off[q];
      c.dh = (ph + s->pad_h - c.r0) / sh; c.dw = (pw + s->pad_w - c.s0) / sw;
      c.Hc = ph < s->H ? (s->H - ph + sh - 1) / sh : 0;
      c.Wc = pw < s->W ? (s->W - pw + sw - 1) / sw : 0;
      out[n++] = c;
    }
  return n;
}

// Per-step weight preparation, one pass over the f32 master weight w[K][C][R][S] (torch layout):
//   wk [K][R][S][Cpad] bf16      — fwd / wgrad operand (input channels zero-padded to Cpad)
//   wt [class][Cpad][Rc][Sc][Kpad] bf16 — dgrad operand, taps grouped by stride-parity class
// Tiles go through LDS so the f32 reads and both bf16 writes run along their contiguous axes
// (pack_plan; R*S <= 196).
struct PackP {
  const float* w;
  uint16_t* wk;
  uint16_t* wt;
  int64_t K, C, Cpad, Kpad;
  int R, S, st_h, st_w;
  int64_t off[4];
  int Rc[4], Sc[4];
  int dense;  // wt as [R][S][Cpad][Kpad]: the 1x1-GEMM dgrad operand of a conv whose output is 1x1
  // split: bf16x3 operands -- every layout is written twice, plane 0 = bf16(w) (hi) and plane 1 =
  // bf16(w - hi) (lo), the lo plane wk_plane / wt_plane elements after the hi plane
  int split;
  int64_t wk_plane, wt_plane;
  // tiling (pack_plan): wk tiles = kr output rows x cw input channels x all taps (nwk of them, first),
  // then wt tiles = 64 output channels x tct input channels x all taps
  int kr, cw, tct;
  int64_t nwk, nwt;
};

}  // namespace mx
