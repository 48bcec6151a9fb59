// N8: multi-scale + flip softmax inference -- the per-view tail of
// pyscripts/inference/inference_softmax_msc.py:135-143, 146-147.  Per view the reference divides the summed window
// logits by the overlap counts (:135), crops to the un-padded region (:136), interpolates bilinearly to the image
// (:137-138), soft-maxes over the classes (:139), flips the RESULT back (:141-142) and adds it to the sum over the
// views (:146-147): six full passes over an ncls x H x W tensor, one of them through host numpy.  Here it is one kernel:
//
//   view_probs<NC>   canvas [ncls][Hp][Wp] (read once) -> acc [ncls][h][w] += softmax_c(bilinear(canvas / counts))
//
// At 21 classes and a 375 x 500 image the accumulator is 15.75 MB and a view's canvas up to 35 MB, against the 3 MB of
// the 1/8-resolution kernels of pseudo_label.hip (16 lanes per pixel, class planes read with a stride across lanes): here
// a thread owns one output pixel and consecutive lanes own consecutive x, so the read-modify-write of acc is perfectly
// coalesced and the tap reads are near-coalesced runs (reversed for a flipped view).  The four tap offsets, the two
// weight pairs and the four count products are formed once per pixel; the interpolated logits of all classes stay in
// registers between the maximum and the exp pass (NC = the class count padded to 8, 16, 24, 32 or 64: every loop
// unrolls and the tap loads are in flight before the first use -- DESIGN 5e, 8e; measured: profiles/softmax_msc.md).
// No LDS, no atomics, no workspace: two calls on equal inputs are bit-identical, with or without the deterministic mode.
//
// Bilinear taps: bilinear.hpp (ATen's rule), with in = rh / rw, never Hp / Wp -- the padding must not leak;
// value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
#include "bilinear.hpp"
#include "common.hpp"

namespace spml {
namespace {

constexpr int kChunk = 8;              // class planes whose taps are loaded together

// thread = output pixel i = y * w + x of acc [ncls][h * w].  The mapping is evaluated at xd = flip ? w - 1 - x : x and
// the result stored at x: the reference interpolates the still-flipped view and flips the result (:141-142).
template <int NC>
__global__ __launch_bounds__(256) void view_probs(const float* __restrict__ canvas, int ncls, int Wp, size_t plane,
                                                  const float* __restrict__ cnt_y, const float* __restrict__ cnt_x,
                                                  int rh, int rw, int flip, int h, int w, float scale_h,
                                                  float scale_w, float* __restrict__ acc) {
  const int n = h * w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int y = i / w, x = i - y * w;
  const Tap ty = make_tap(y, scale_h, rh), tx = make_tap(flip ? w - 1 - x : x, scale_w, rw);
  const int o00 = ty.i0 * Wp + tx.i0, o01 = ty.i0 * Wp + tx.i1, o10 = ty.i1 * Wp + tx.i0, o11 = ty.i1 * Wp + tx.i1;
  const float cy0 = cnt_y[ty.i0], cy1 = cnt_y[ty.i1], cx0 = cnt_x[tx.i0], cx1 = cnt_x[tx.i1];
  // counts[y][x] of :134 = cnt_y[y] * cnt_x[x] (the windows are a Cartesian product; small integers: exact)
  const float d00 = cy0 * cx0, d01 = cy0 * cx1, d10 = cy1 * cx0, d11 = cy1 * cx1;

  float val[NC];
  float m = -INFINITY;
#pragma unroll
  for (int c0 = 0; c0 < NC; c0 += kChunk) {
    float a[kChunk], b[kChunk], c[kChunk], d[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      // (a class above ncls reads the last plane -- a valid address, no branch around the loads -- and is dropped below)
      const float* base = canvas + (size_t)min(c0 + j, ncls - 1) * plane;
      a[j] = base[o00]; b[j] = base[o01]; c[j] = base[o10]; d[j] = base[o11];
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      // a true division per tap, before the interpolation (:135)
      const float v = ty.l0 * (tx.l0 * (a[j] / d00) + tx.l1 * (b[j] / d01)) +
                      ty.l1 * (tx.l0 * (c[j] / d10) + tx.l1 * (d[j] / d11));
      val[c0 + j] = c0 + j < ncls ? v : -INFINITY;
      m = fmaxf(m, val[c0 + j]);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    val[c] = c < ncls ? expf(val[c] - m) : 0.f;
    s += val[c];
  }
  float* dst = acc + i;
#pragma unroll
  for (int c0 = 0; c0 < NC; c0 += kChunk) {
    float old[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) old[j] = c0 + j < ncls ? dst[(size_t)(c0 + j) * n] : 0.f;
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (c0 + j < ncls) dst[(size_t)(c0 + j) * n] = old[j] + val[c0 + j] / s;
  }
}

constexpr int kMaxClasses = 64;

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" int spml_view_probs_accumulate_f32(const float* canvas, int ncls, int Hp, int Wp, const float* cnt_y,
                                              const float* cnt_x, int rh, int rw, int flip, int h, int w, float* acc,
                                              void* stream) {
  if (!canvas || !cnt_y || !cnt_x || !acc || ncls <= 0 || Hp <= 0 || Wp <= 0 || rh <= 0 || rw <= 0 || rh > Hp ||
      rw > Wp || h <= 0 || w <= 0)
    return SPML_ERR_INVALID_ARG;
  if (ncls > kMaxClasses || (int64_t)Hp * Wp > (1 << 30) || (int64_t)h * w > (1 << 30)) return SPML_ERR_UNSUPPORTED;
  const size_t plane = (size_t)Hp * Wp;
  const int n = h * w;
  const uintptr_t c0 = (uintptr_t)canvas, c1 = c0 + (size_t)ncls * plane * sizeof(float);
  const uintptr_t a0 = (uintptr_t)acc, a1 = a0 + (size_t)ncls * n * sizeof(float);
  if (a0 < c1 && c0 < a1) return SPML_ERR_INVALID_ARG;               // acc may not alias canvas
  const float sh = (float)rh / (float)h, sw = (float)rw / (float)w;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define SPML_VIEW(NC)                                                                                              \
  hipLaunchKernelGGL(view_probs<NC>, grid, block, 0, s, canvas, ncls, Wp, plane, cnt_y, cnt_x, rh, rw, flip, h, w, \
                     sh, sw, acc)
  if (ncls <= 8) SPML_VIEW(8);
  else if (ncls <= 16) SPML_VIEW(16);
  else if (ncls <= 24) SPML_VIEW(24);
  else if (ncls <= 32) SPML_VIEW(32);
  else SPML_VIEW(64);
#undef SPML_VIEW
  return launch_status();
}
