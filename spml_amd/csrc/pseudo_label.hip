// N7: pseudo-label generation from the softmax head -- the pieces of
// pyscripts/inference/pseudo_softmaxrw_crf.py:130-176 and pseudo_softmax.py:129-179 around the affinity kernel
// (affinity.hip) and the walk's library GEMMs.  Per flipped / rescaled view the reference crops the network's outputs to
// the un-padded region, flips them back, resamples them bilinearly to 1/8 of the image, normalises the embedding and
// soft-maxes the logits; after the last view it averages, normalises every class map by its maximum, masks the classes
// that are not among the image's tags, walks, up-samples to the image and arg-maxes.  Here:
//
//   resample_unit          embedding (any strides) -> cropped, un-flipped, resampled, x / |x|  -> view slice of [B][C][n]
//   resample_classes       logits (any strides)    -> cropped, un-flipped, resampled, (softmax) -> += acc [ncls][n]
//   cam_pixel_softmax      logit_mean only: softmax(acc / B) over the classes
//   cam_class_normalize    (acc / B) / max over the pixels, tag mask, background threshold
//   upsample_argmax        walked CAMs [ncls][oh][ow] -> bilinear to h x w, arg-max -> int64 [h][w]
//
// All of them move a few MB at most and are bound by latency and launch count: the two view kernels give a pixel to 16
// lanes (a channel slice each, so a 46 x 62 map is 716 waves and not 45) and combine the slices with four xor-shuffles;
// the four taps of every channel a lane owns are loaded before the first use.  No atomics anywhere: every result is
// bit-reproducible and the same in either mode of the library.
//
// Bilinear weights as ATen forms them (align_corners = False, no anti-aliasing): scale = in / out in fp32,
// src = max(scale * (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1,
// value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
#include "bilinear.hpp"
#include "common.hpp"

namespace spml {
namespace {

constexpr int kSlices = 16;            // lanes per pixel in the view kernels
constexpr int kViewPix = 16;           // pixels per 256-thread workgroup there
constexpr int kOwn = 4;                // channels of one 64-channel chunk a lane owns (slice, +16, +32, +48)

// (Taps4, make_taps and blend -- the four taps of an output pixel and their weighted sum -- are in bilinear.hpp)

// sum / max over the 16 lanes of a pixel (xor 8, 4, 2, 1 stays inside an aligned group of 16): every lane ends with the
// same value, formed in the same order whatever the input's memory layout
__device__ __forceinline__ float slices_sum(float v) {
#pragma unroll
  for (int o = kSlices / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ float slices_max(float v) {
#pragma unroll
  for (int o = kSlices / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// resampled values of the channels a lane owns: channel = 64 * k + 16 * j + slice -> val[k * kOwn + j] (0 above C).
// NCH 64-channel chunks, fully unrolled: the 16 loads of a chunk are in flight together.
template <int NCH>
__device__ __forceinline__ void resample_owned(const float* __restrict__ src, int C, int64_t sc, const Taps4& t,
                                               int slice, bool live, float (&val)[NCH * kOwn]) {
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    float a[kOwn], b[kOwn], c[kOwn], d[kOwn];
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ch = 64 * k + kSlices * j + slice;
      const bool ok = live && ch < C;
      const float* base = src + (int64_t)ch * sc;
      a[j] = ok ? base[t.o00] : 0.f;
      b[j] = ok ? base[t.o01] : 0.f;
      c[j] = ok ? base[t.o10] : 0.f;
      d[j] = ok ? base[t.o11] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kOwn; ++j) val[k * kOwn + j] = blend(t, a[j], b[j], c[j], d[j]);
  }
}

// ---------------------------------------------------------------------------------------
// out[c][p] = r[c][p] / sqrt(sum_c r[c][p]^2),  r = the resampled view (pseudo_softmaxrw_crf.py:130-136)
template <int NCH>
__global__ __launch_bounds__(256) void resample_unit(const float* __restrict__ emb, int C, int64_t sc, int64_t sy,
                                                     int64_t sx, int rh, int rw, int flip, int oh, int ow,
                                                     float scale_h, float scale_w, float* __restrict__ out) {
  const int slice = threadIdx.x & (kSlices - 1);
  const int n = oh * ow;
  const int p = blockIdx.x * kViewPix + (threadIdx.x >> 4);
  const bool live = p < n;
  const Taps4 t = make_taps(live ? p : 0, ow, scale_h, scale_w, rh, rw, flip, sy, sx);
  float val[NCH * kOwn];
  resample_owned<NCH>(emb, C, sc, t, slice, live, val);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NCH * kOwn; ++i) ss += val[i] * val[i];
  const float norm = sqrtf(slices_sum(ss));          // (plain division below, no epsilon: :136)
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ch = 64 * k + kSlices * j + slice;
      if (live && ch < C) out[(size_t)ch * n + p] = val[k * kOwn + j] / norm;
    }
}

// ---------------------------------------------------------------------------------------
// acc[c][p] += softmax_c(r[c][p]) (SOFTMAX: pseudo_softmaxrw_crf.py:141-144) or r[c][p] (pseudo_softmax.py:140-144)
template <int NCH, bool SOFTMAX>
__global__ __launch_bounds__(256) void resample_classes(const float* __restrict__ logit, int ncls, int64_t sc,
                                                        int64_t sy, int64_t sx, int rh, int rw, int flip, int oh,
                                                        int ow, float scale_h, float scale_w,
                                                        float* __restrict__ acc) {
  const int slice = threadIdx.x & (kSlices - 1);
  const int n = oh * ow;
  const int p = blockIdx.x * kViewPix + (threadIdx.x >> 4);
  const bool live = p < n;
  const Taps4 t = make_taps(live ? p : 0, ow, scale_h, scale_w, rh, rw, flip, sy, sx);
  float val[NCH * kOwn];
  resample_owned<NCH>(logit, ncls, sc, t, slice, live, val);
  float old[NCH * kOwn];
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ch = 64 * k + kSlices * j + slice;
      old[k * kOwn + j] = live && ch < ncls ? acc[(size_t)ch * n + p] : 0.f;
    }
  if (SOFTMAX) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int j = 0; j < kOwn; ++j)
        if (64 * k + kSlices * j + slice < ncls) m = fmaxf(m, val[k * kOwn + j]);
    m = slices_max(m);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int j = 0; j < kOwn; ++j) {
        const float e = 64 * k + kSlices * j + slice < ncls ? expf(val[k * kOwn + j] - m) : 0.f;
        val[k * kOwn + j] = e;
        s += e;
      }
    s = slices_sum(s);
#pragma unroll
    for (int i = 0; i < NCH * kOwn; ++i) val[i] = val[i] / s;
  }
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ch = 64 * k + kSlices * j + slice;
      if (live && ch < ncls) acc[(size_t)ch * n + p] = old[k * kOwn + j] + val[k * kOwn + j];
    }
}

// ---------------------------------------------------------------------------------------
// logit_mean: cam[c][p] = softmax_c(acc[c][p] / B) (pseudo_softmax.py:149-150).  The layout of the view kernels: 16
// lanes per pixel, a lane's classes stay in registers between the maximum, the sum and the division (one thread per
// pixel is 12 workgroups at n = 2852 and three dependent passes over the planes: profiles/pseudo_labels.md).
template <int NCH>
__global__ __launch_bounds__(256) void cam_pixel_softmax(const float* __restrict__ acc, int ncls, int n, float views,
                                                         float* __restrict__ cam) {
  const int slice = threadIdx.x & (kSlices - 1);
  const int p = blockIdx.x * kViewPix + (threadIdx.x >> 4);
  const bool live = p < n;
  float val[NCH * kOwn];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ch = 64 * k + kSlices * j + slice;
      val[k * kOwn + j] = live && ch < ncls ? acc[(size_t)ch * n + p] / views : -INFINITY;
      m = fmaxf(m, val[k * kOwn + j]);
    }
  m = slices_max(m);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const float e = live && 64 * k + kSlices * j + slice < ncls ? expf(val[k * kOwn + j] - m) : 0.f;
      val[k * kOwn + j] = e;
      s += e;
    }
  s = slices_sum(s);
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ch = 64 * k + kSlices * j + slice;
      if (live && ch < ncls) cam[(size_t)ch * n + p] = val[k * kOwn + j] / s;
    }
}

// workgroup = class: cam[c][:] = (src[c][:] / views) / max_p(src[c][p] / views); 0 where the tag is absent; class 0 =
// threshold when one is given (pseudo_softmaxrw_crf.py:150-157).  `src` may be `cam` itself (in place): every element is
// read and written by one thread, and the barrier of the reduction separates the reads of the first pass from the writes.
constexpr int kClassThreads = 1024;

__global__ __launch_bounds__(kClassThreads) void cam_class_normalize(const float* src, int n, float views,
                                                                      const unsigned char* __restrict__ tags,
                                                                      int has_threshold, float threshold,
                                                                      float* cam) {
  __shared__ float part[kClassThreads / 64];
  const int c = blockIdx.x;
  const float* row = src + (size_t)c * n;
  float* dst = cam + (size_t)c * n;
  if (c == 0 && has_threshold) {                       // (block-uniform)
    for (int i = threadIdx.x; i < n; i += kClassThreads) dst[i] = threshold;
    return;
  }
  if (!tags[c]) {
    for (int i = threadIdx.x; i < n; i += kClassThreads) dst[i] = 0.f;
    return;
  }
  float m = -INFINITY;
  for (int i = threadIdx.x; i < n; i += kClassThreads) m = fmaxf(m, row[i] / views);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  m = part[0];
#pragma unroll
  for (int i = 1; i < kClassThreads / 64; ++i) m = fmaxf(m, part[i]);
  for (int i = threadIdx.x; i < n; i += kClassThreads) dst[i] = (row[i] / views) / m;
}

// ---------------------------------------------------------------------------------------
// thread = one pixel of the h x w image; its four taps are shared by all classes, eight class planes in flight before
// the first comparison.  The 1/8 map is a few hundred KB: every tap after the first touch comes from the cache.
__global__ __launch_bounds__(256) void upsample_argmax(const float* __restrict__ cam, int ncls, int oh, int ow, int h,
                                                       int w, float scale_h, float scale_w,
                                                       int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)h * w) return;
  const Taps4 t = make_taps((int)i, w, scale_h, scale_w, oh, ow, 0, ow, 1);
  const size_t plane = (size_t)oh * ow;
  float best = blend(t, cam[t.o00], cam[t.o01], cam[t.o10], cam[t.o11]);
  int arg = 0;
  for (int c0 = 1; c0 < ncls; c0 += 8) {
    float a[8], b[8], c[8], d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = c0 + j < ncls;
      const float* base = cam + (size_t)(ok ? c0 + j : 0) * plane;
      a[j] = base[t.o00]; b[j] = base[t.o01]; c[j] = base[t.o10]; d[j] = base[t.o11];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = c0 + j < ncls ? blend(t, a[j], b[j], c[j], d[j]) : -INFINITY;
      // strict '>' keeps the lowest index of a tie (the -inf fillers never win); a NaN wins over every number and the
      // first NaN is kept (what torch.argmax returns) -- the rules of argmax_channels (softmax_head.hip)
      if (v > best || (v != v && best == best)) {
        best = v;
        arg = c0 + j;
      }
    }
  }
  out[i] = arg;
}

constexpr int kMaxChannels = 256;      // 4 chunks of 64

bool view_args_ok(const void* src, int C, int Hp, int Wp, int rh, int rw, int oh, int ow) {
  return src && C > 0 && Hp > 0 && Wp > 0 && rh > 0 && rw > 0 && rh <= Hp && rw <= Wp && oh > 0 && ow > 0;
}

// the largest element offset a view kernel forms must fit the strides' claim of a [C][Hp][Wp] tensor; negative strides
// are outside what the kernels take
bool strides_ok(int64_t sc, int64_t sy, int64_t sx) { return sc > 0 && sy > 0 && sx > 0; }

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" int spml_resample_unit_f32(const float* emb, int C, int Hp, int Wp, int64_t stride_c, int64_t stride_y,
                                      int64_t stride_x, int rh, int rw, int flip, int oh, int ow, float* out, int B,
                                      int b, void* stream) {
  if (!view_args_ok(emb, C, Hp, Wp, rh, rw, oh, ow) || !out || B <= 0 || b < 0 || b >= B)
    return SPML_ERR_INVALID_ARG;
  if (C > kMaxChannels || !strides_ok(stride_c, stride_y, stride_x) || (int64_t)oh * ow > (1 << 24))
    return SPML_ERR_UNSUPPORTED;
  const int n = oh * ow;
  const float sh = (float)rh / (float)oh, sw = (float)rw / (float)ow;
  float* dst = out + (size_t)b * C * n;
  const dim3 grid((unsigned)((n + kViewPix - 1) / kViewPix)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define SPML_UNIT(NCH)                                                                                              \
  hipLaunchKernelGGL(resample_unit<NCH>, grid, block, 0, s, emb, C, stride_c, stride_y, stride_x, rh, rw, flip, oh, \
                     ow, sh, sw, dst)
  if (C <= 64) SPML_UNIT(1);
  else if (C <= 128) SPML_UNIT(2);
  else SPML_UNIT(4);
#undef SPML_UNIT
  return launch_status();
}

extern "C" int spml_resample_classes_accumulate_f32(const float* logit, int ncls, int Hp, int Wp, int64_t stride_c,
                                                    int64_t stride_y, int64_t stride_x, int rh, int rw, int flip,
                                                    int oh, int ow, int combine, float* acc, void* stream) {
  if (!view_args_ok(logit, ncls, Hp, Wp, rh, rw, oh, ow) || !acc ||
      (combine != SPML_COMBINE_PROB_MEAN && combine != SPML_COMBINE_LOGIT_MEAN))
    return SPML_ERR_INVALID_ARG;
  if (ncls > kMaxChannels || !strides_ok(stride_c, stride_y, stride_x) || (int64_t)oh * ow > (1 << 24))
    return SPML_ERR_UNSUPPORTED;
  const int n = oh * ow;
  const float sh = (float)rh / (float)oh, sw = (float)rw / (float)ow;
  const dim3 grid((unsigned)((n + kViewPix - 1) / kViewPix)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define SPML_CLS(NCH, SM)                                                                                          \
  hipLaunchKernelGGL((resample_classes<NCH, SM>), grid, block, 0, s, logit, ncls, stride_c, stride_y, stride_x, rh, \
                     rw, flip, oh, ow, sh, sw, acc)
#define SPML_CLS2(NCH)                                                  \
  do {                                                                  \
    if (combine == SPML_COMBINE_PROB_MEAN) SPML_CLS(NCH, true);         \
    else SPML_CLS(NCH, false);                                          \
  } while (0)
  if (ncls <= 64) SPML_CLS2(1);
  else if (ncls <= 128) SPML_CLS2(2);
  else SPML_CLS2(4);
#undef SPML_CLS2
#undef SPML_CLS
  return launch_status();
}

extern "C" int spml_cam_finalize_f32(const float* acc, int ncls, int64_t n, int B, int combine,
                                     const unsigned char* tags, int has_threshold, float threshold, float* cam,
                                     void* stream) {
  if (!acc || !tags || !cam || ncls <= 0 || n <= 0 || B <= 0 ||
      (combine != SPML_COMBINE_PROB_MEAN && combine != SPML_COMBINE_LOGIT_MEAN))
    return SPML_ERR_INVALID_ARG;
  if (n > (1 << 24) || ncls > kMaxChannels) return SPML_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (combine == SPML_COMBINE_LOGIT_MEAN) {
    const dim3 grid((unsigned)((n + kViewPix - 1) / kViewPix)), block(256);
#define SPML_SM(NCH) hipLaunchKernelGGL(cam_pixel_softmax<NCH>, grid, block, 0, s, acc, ncls, (int)n, (float)B, cam)
    if (ncls <= 64) SPML_SM(1);
    else if (ncls <= 128) SPML_SM(2);
    else SPML_SM(4);
#undef SPML_SM
    hipLaunchKernelGGL(cam_class_normalize, dim3((unsigned)ncls), dim3(kClassThreads), 0, s, cam, (int)n, 1.0f, tags,
                       has_threshold, threshold, cam);
  } else {
    hipLaunchKernelGGL(cam_class_normalize, dim3((unsigned)ncls), dim3(kClassThreads), 0, s, acc, (int)n, (float)B,
                       tags, has_threshold, threshold, cam);
  }
  return launch_status();
}

extern "C" int spml_upsample_argmax_i64(const float* cam, int ncls, int oh, int ow, int h, int w, int64_t* out,
                                        void* stream) {
  if (!cam || !out || ncls <= 0 || oh <= 0 || ow <= 0 || h <= 0 || w <= 0) return SPML_ERR_INVALID_ARG;
  if ((int64_t)h * w > (int64_t)1 << 30 || (int64_t)oh * ow > (1 << 24)) return SPML_ERR_UNSUPPORTED;
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(upsample_argmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam, ncls,
                     oh, ow, h, w, (float)oh / (float)h, (float)ow / (float)w, out);
  return launch_status();
}
