// The CAM files of another model, from the planes a file carries to the class maps the random walk takes: one launch
// (include/spml_hip.h, "CAM ingest").
//
// replaces pseudo_camrw_crf.py:108-111 (a zeroed [ncls, h, w] array, the planes written into it, the background
// (1 - max over the foreground) ** ALPHA) and :151-152 (F.interpolate(scale_factor=1/8, mode='bilinear') of that array).
//
// F.interpolate uses the GIVEN factor for the source coordinate: 8 * (d + 0.5) - 0.5 = 8 d + 3.5, so an output value is
// the mean of the source at rows 8 y + 3, 8 y + 4 and columns 8 x + 3, 8 x + 4, whatever h % 8 and w % 8 are (the last
// tap is 8 (h / 8 - 1) + 4 <= h - 4).  The full-resolution array is never formed: a thread owns one output pixel, reads
// the four taps of every plane the file carries and keeps the maximum per TAP (the background is a function of the
// maximum at a source pixel, and the mean is taken after the power).
//
// Shape of the work: h / 8 x w / 8 output pixels (46 x 62 = 2852 for a 375 x 500 file), K planes, four taps each, no
// value read twice -- so no LDS, and the launch is bound by the latency of one round of loads, not by bytes.  What
// shortens it: every load of a thread is independent (the loop over the classes is unrolled and the class -> plane
// table is wave-uniform kernel-argument data, so the compiler issues the loads of several planes before the first
// wait), and one wave per workgroup spreads the few waves over as many CUs.  A wave's load instruction reads 64 pairs
// of floats 32 bytes apart: two rows of eight are touched, a quarter of the planes' cache lines.  The rows of `out`
// are written with consecutive lanes on consecutive floats.
//
// The sums and the power run in fp64 (a few thousand threads: the rate does not matter) and are rounded to fp32 once,
// so every output is within one rounding of the exact four-tap expression on the fp32 inputs.
#include "common.hpp"

namespace spml {
namespace {

constexpr int kCamMaxClasses = 256;      // label maps are uint8
constexpr int kCamMaxSide = 16384;
constexpr int kCamThreads = kWave;

// class row c (1 .. ncls - 1) -> index of its plane in `planes`, or -1 for a class the file does not carry
struct cam_planes_of {
  int plane[kCamMaxClasses];
};

bool cam_shape_ok(int K, int h, int w, int ncls) {
  return ncls >= 1 && ncls <= kCamMaxClasses && K >= 0 && K <= ncls - 1 && h >= 8 && w >= 8 && h <= kCamMaxSide &&
         w <= kCamMaxSide;
}

// torch.max / np.max: a NaN wins
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ double ipow(double x, int n) {
  double r = 1.0;
  for (; n > 0; n >>= 1) {
    if (n & 1) r *= x;
    x *= x;
  }
  return r;
}

__global__ __launch_bounds__(kCamThreads) void cam_ingest(const float* __restrict__ planes, cam_planes_of table,
                                                           int all_present, int h, int w, int ncls, int alpha, int oh,
                                                           int ow, float* __restrict__ out) {
  const int p = blockIdx.x * kCamThreads + threadIdx.x;
  if (p >= oh * ow) return;
  const int y = p / ow, x = p - y * ow;
  const size_t plane_px = (size_t)h * w, out_px = (size_t)oh * ow;
  const size_t tap = (size_t)(8 * y + 3) * w + (8 * x + 3);          // rows 8y+3, 8y+4 <= h-4; columns 8x+3, 8x+4 <= w-4
  // with a class absent the maximum runs over that class's zeros too
  const float start = all_present ? -INFINITY : 0.f;
  float m00 = start, m01 = start, m10 = start, m11 = start;
#pragma unroll 4
  for (int c = 1; c < ncls; ++c) {
    const int k = table.plane[c];                                     // wave-uniform
    float mean = 0.f;
    if (k >= 0) {
      const float* src = planes + (size_t)k * plane_px + tap;
      const float a = src[0], b = src[1], d = src[w], e = src[w + 1];
      m00 = max_nan(m00, a);
      m01 = max_nan(m01, b);
      m10 = max_nan(m10, d);
      m11 = max_nan(m11, e);
      mean = (float)((((double)a + (double)b) + ((double)d + (double)e)) * 0.25);
    }
    out[(size_t)c * out_px + p] = mean;                               // zeros for an absent class: no memset before
  }
  double background = 1.0;                                            // ncls == 1: cam_with_background's 1
  if (ncls > 1)
    background = ((ipow(1.0 - (double)m00, alpha) + ipow(1.0 - (double)m01, alpha)) +
                  (ipow(1.0 - (double)m10, alpha) + ipow(1.0 - (double)m11, alpha))) * 0.25;
  out[p] = (float)background;
}

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" const char* spml_cam_ingest_path_name(int K, int h, int w, int ncls) {
  return cam_shape_ok(K, h, w, ncls) ? "cam_ingest" : "unsupported";
}

extern "C" int spml_cam_ingest_f32(const float* planes, const int* classes, int K, int h, int w, int ncls, int alpha,
                                   float* out, void* stream) {
  if (!out || ((uintptr_t)out & 3) != 0 || ((uintptr_t)planes & 3) != 0) return SPML_ERR_INVALID_ARG;
  if (K > 0 && (!planes || !classes)) return SPML_ERR_INVALID_ARG;
  if (alpha < 0) return SPML_ERR_INVALID_ARG;
  if (!cam_shape_ok(K, h, w, ncls)) return SPML_ERR_UNSUPPORTED;
  cam_planes_of table;
  for (int c = 0; c < kCamMaxClasses; ++c) table.plane[c] = -1;
  for (int k = 0; k < K; ++k) {
    const int key = classes[k];                                       // the file's key: class - 1
    if (key < 0 || key > ncls - 2 || table.plane[key + 1] >= 0) return SPML_ERR_INVALID_ARG;
    table.plane[key + 1] = k;
  }
  const int oh = h / 8, ow = w / 8;
  const size_t out_bytes = (size_t)ncls * oh * ow * sizeof(float);
  if (overlap(out, out_bytes, planes, (size_t)K * h * w * sizeof(float))) return SPML_ERR_INVALID_ARG;
  const unsigned grid = (unsigned)((oh * ow + kCamThreads - 1) / kCamThreads);
  hipLaunchKernelGGL(cam_ingest, dim3(grid), dim3(kCamThreads), 0, (hipStream_t)stream, planes, table,
                     K == ncls - 1 ? 1 : 0, h, w, ncls, alpha, oh, ow, out);
  return launch_status();
}
