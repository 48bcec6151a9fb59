// Bilinear source taps as ATen forms them (`F.interpolate(mode='bilinear')`, align_corners = False, no anti-aliasing):
// scale = in / out in fp32, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1),
// l1 = src - i0, l0 = 1 - l1.  Shared by pseudo_label.hip and msc_inference.hip.
#pragma once

#include "common.hpp"

namespace spml {

struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap make_tap(int dst, float scale, int in) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  Tap t;
  t.i0 = min((int)src, in - 1);        // (src >= 0: the conversion is the floor)
  t.i1 = min(t.i0 + 1, in - 1);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

// the four element offsets of output pixel p of an oh x ow map over the top-left rh x rw region of a plane with
// strides (sy, sx); with `flip` logical column x is stored at rw - 1 - x.  Shared by pseudo_label.hip and dense_crf.hip:
// value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
struct Taps4 {
  int64_t o00, o01, o10, o11;
  float h0, h1, w0, w1;
};

__device__ __forceinline__ Taps4 make_taps(int p, int ow, float scale_h, float scale_w, int rh, int rw, int flip,
                                            int64_t sy, int64_t sx) {
  const int oy = p / ow, ox = p - oy * ow;
  const Tap ty = make_tap(oy, scale_h, rh), tx = make_tap(ox, scale_w, rw);
  const int x0 = flip ? rw - 1 - tx.i0 : tx.i0, x1 = flip ? rw - 1 - tx.i1 : tx.i1;
  Taps4 t;
  t.o00 = ty.i0 * sy + x0 * sx;
  t.o01 = ty.i0 * sy + x1 * sx;
  t.o10 = ty.i1 * sy + x0 * sx;
  t.o11 = ty.i1 * sy + x1 * sx;
  t.h0 = ty.l0; t.h1 = ty.l1; t.w0 = tx.l0; t.w1 = tx.l1;
  return t;
}

__device__ __forceinline__ float blend(const Taps4& t, float a, float b, float c, float d) {
  return t.h0 * (t.w0 * a + t.w1 * b) + t.h1 * (t.w0 * c + t.w1 * d);
}

}  // namespace spml
