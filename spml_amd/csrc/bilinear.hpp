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

}  // namespace spml
