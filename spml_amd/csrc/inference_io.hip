// N15: the two ends of an inference program that reads image files -- the host-side chains of the
// reference's programs (spml/data/datasets/base_dataset.py:105-119,157-171 normalise; spml/utils/general/others.py:10-47
// create_image_pyramid with spml/data/transforms.py:26-37 resize; inference_softmax.py:89-103 resize_with_interpolation +
// resize_with_pad; :142-160 crop, cv2.resize(INTER_NEAREST), colour) as ONE launch each:
//
//   image_views    u8 RGB HWC (+ the u8 semantic plane) of one file, one record per view
//                  -> every view [3][pad_h][pad_w] fp32 in one buffer (+ its label [new_h][new_w] int64 in another)
//   label_export   prediction int64 [pred_h][pred_w], its valid top-left rectangle
//                  -> gray u8 [out_h][out_w], rgb u8 [out_h][out_w][3] at the file's own size
//
// and, for the programs that end in the dense CRF (inference_softmax_crf_msc.py:159-164, the uint8 image
// rebuilt from the network's input; inference_crf.py:257-261 with benchmark_by_mIoU.py:25-53):
//
//   crf_guide            u8 RGB HWC of one file -> the CRF's guide u8 [new_h][new_w][3]: the value image_views writes,
//                        denormalised again by the reference's lossy chain (a table in LDS when new == src)
//   label_export_scored  label_export of the refined labels + the same resampling of the labels before the CRF, both
//                        scored against the file's ground truth, and the count of pixels the CRF changed
//
// Every output pixel is composed BACKWARDS through the reference's stages: pad (zeros, 'left_top') -> mirror of the
// RESIZED image -> cv2.resize (INTER_LINEAR on the normalised float image, INTER_NEAREST on the label) -> normalise.
// The tap rule is the one of csrc/augment.hip, restated here (that file's helpers sit in its unnamed namespace next to
// its own record): source coordinates in fp64 from the integers of the record, the fraction rounded to fp32,
// contraction off for the whole file.
//
// blockIdx.z is the view: the record is uniform per workgroup.  Thread = one output pixel of a 32 x 8 tile, lanes along
// x: a wave stores two 128-byte row pieces per channel.  The tile grid is the largest view's; a workgroup whose tile
// lies outside its own view's plane returns at once.  Every element of every plane is written (the caller allocates
// without a memset).  No inline assembly, no workspace, no host read anywhere in this file; image_views and label_export
// use no LDS and no atomics, crf_guide a 768-byte table in LDS, label_export_scored integer atomics only.
#include "common.hpp"

#pragma clang fp contract(off)

#ifndef SPML_EXPORT_TABLE_LDS
#define SPML_EXPORT_TABLE_LDS 0      // 1: the other side of the A/B of tools/bench_inference_io.py (the table staged in LDS)
#endif

namespace spml {
namespace {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kMaxSide = 16384;                 // of a source, a view and its padded plane: 3 * h * w * 4 stays below 2^32
constexpr int kMaxViews = 64;

// The one expression that decides whether a record runs -- the host entry (before anything is launched), the kernel
// (a record that fails writes nothing and forms no address) and spml_image_views_path_name read it.
__host__ __device__ inline bool view_ok(const spml_view_params& p, int h, int w, int64_t image_bytes,
                                        int64_t label_bytes, bool with_labels) {
  if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return false;
  if (p.new_h < 1 || p.new_w < 1 || p.new_h > kMaxSide || p.new_w > kMaxSide) return false;
  if (p.pad_h < p.new_h || p.pad_w < p.new_w || p.pad_h > kMaxSide || p.pad_w > kMaxSide) return false;
  const int64_t plane = 3 * (int64_t)p.pad_h * p.pad_w * (int64_t)sizeof(float);
  if (p.image_off < 0 || (p.image_off & 3) != 0 || p.image_off > image_bytes - plane) return false;
  if (with_labels) {
    const int64_t lab = (int64_t)p.new_h * p.new_w * (int64_t)sizeof(int64_t);
    if (p.label_off < 0 || (p.label_off & 7) != 0 || p.label_off > label_bytes - lab) return false;
  }
  return true;
}

inline bool ranges_overlap(int64_t a, int64_t a_bytes, int64_t b, int64_t b_bytes) {
  return a < b + b_bytes && b < a + a_bytes;
}

// ... and whether the whole call runs: V, every record, no two planes of one buffer overlapping
inline bool views_ok(const spml_view_params* p, int V, int h, int w, int64_t image_bytes, int64_t label_bytes,
                     bool with_labels) {
  if (!p || V < 1 || V > kMaxViews) return false;
  for (int v = 0; v < V; ++v)
    if (!view_ok(p[v], h, w, image_bytes, label_bytes, with_labels)) return false;
  for (int a = 0; a < V; ++a)
    for (int b = a + 1; b < V; ++b) {
      if (ranges_overlap(p[a].image_off, 12 * (int64_t)p[a].pad_h * p[a].pad_w, p[b].image_off,
                         12 * (int64_t)p[b].pad_h * p[b].pad_w))
        return false;
      if (with_labels && ranges_overlap(p[a].label_off, 8 * (int64_t)p[a].new_h * p[a].new_w, p[b].label_off,
                                        8 * (int64_t)p[b].new_h * p[b].new_w))
        return false;
    }
  return true;
}

__host__ __device__ inline bool export_ok(int pred_h, int pred_w, int valid_h, int valid_w, int out_h, int out_w) {
  if (pred_h < 1 || pred_w < 1 || pred_h > kMaxSide || pred_w > kMaxSide) return false;
  if (valid_h < 1 || valid_w < 1 || valid_h > pred_h || valid_w > pred_w) return false;
  if (out_h < 1 || out_w < 1 || out_h > kMaxSide || out_w > kMaxSide) return false;
  return true;
}

// cv2.resize on an explicit size: scale = 1 / (new / src), both in double
__device__ __forceinline__ double axis_scale(int src, int dst) { return 1.0 / ((double)dst / (double)src); }

// INTER_LINEAR: the first tap and the fp32 fraction of destination coordinate d
__device__ __forceinline__ void linear_tap(int d, double scale, int src, int& s, float& frac) {
  double f = ((double)d + 0.5) * scale - 0.5;
  double fl = floor(f);
  f -= fl;
  s = (int)fl;
  if (s < 0) { s = 0; f = 0.0; }
  if (s >= src - 1) { s = src - 1; f = 0.0; }
  frac = (float)f;
}

// INTER_NEAREST
__device__ __forceinline__ int nearest_tap(int d, double scale, int src) {
  const int s = (int)floor((double)d * scale);
  return s < src - 1 ? s : src - 1;
}

// The four taps and the weights of pixel (y, X) of an un-flipped new_h x new_w view (sy, sx: axis_scale of the two
// axes), and the value of one channel from them: what image_views writes, and what crf_guide denormalises again -- one
// piece of code, so that the guide of a file is the guide of the view the network saw.
struct view_taps {
  const unsigned char* row0;
  const unsigned char* row1;
  int c0, c1;
  float a0, a1, b0, b1;
};

__device__ __forceinline__ view_taps taps_at(const unsigned char* __restrict__ rgb, int h, int w, double sy, double sx,
                                             int y, int X) {
  int r0, c0;
  float fy, fx;
  linear_tap(y, sy, h, r0, fy);
  linear_tap(X, sx, w, c0, fx);
  const int r1 = r0 + 1 < h ? r0 + 1 : r0, c1 = c0 + 1 < w ? c0 + 1 : c0;        // (weight 0 where clamped)
  return {rgb + (size_t)r0 * w * 3, rgb + (size_t)r1 * w * 3, c0, c1, 1.f - fx, fx, 1.f - fy, fy};
}

__device__ __forceinline__ float normalised(unsigned char u8, float m, float s) { return ((float)u8 / 255.f - m) / s; }

__device__ __forceinline__ float view_value(const view_taps& t, int c, float m, float s) {
  const float v00 = normalised(t.row0[t.c0 * 3 + c], m, s), v01 = normalised(t.row0[t.c1 * 3 + c], m, s);
  const float v10 = normalised(t.row1[t.c0 * 3 + c], m, s), v11 = normalised(t.row1[t.c1 * 3 + c], m, s);
  return t.b0 * (t.a0 * v00 + t.a1 * v01) + t.b1 * (t.a0 * v10 + t.a1 * v11);
}

template <bool kLabels>
__global__ __launch_bounds__(kTileW * kTileH) void image_views(
    const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ semantic, int h, int w,
    const float* __restrict__ mean_dev, const float* __restrict__ std_dev, const spml_view_params* __restrict__ params,
    float* __restrict__ images, int64_t image_bytes, int64_t* __restrict__ labels, int64_t label_bytes) {
  const spml_view_params p = params[blockIdx.z];
  if (!view_ok(p, h, w, image_bytes, label_bytes, kLabels)) return;      // (the host entry refused it already)
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  if (x0 >= p.pad_w || y0 >= p.pad_h) return;                            // a smaller view than the launch's grid
  const int x = x0 + (threadIdx.x & (kTileW - 1)), y = y0 + threadIdx.x / kTileW;
  if (x >= p.pad_w || y >= p.pad_h) return;

  float* out = images + p.image_off / (int64_t)sizeof(float);
  const size_t plane = (size_t)p.pad_h * p.pad_w, at = (size_t)y * p.pad_w + x;
  if (y >= p.new_h || x >= p.new_w) {                                    // resize_with_pad(..., 0) of the normalised image
    out[at] = 0.f;
    out[plane + at] = 0.f;
    out[2 * plane + at] = 0.f;
    return;
  }
  const int X = p.flip ? p.new_w - 1 - x : x;                            // the RESIZED image is mirrored
  const double sy = axis_scale(h, p.new_h), sx = axis_scale(w, p.new_w);
  const view_taps t = taps_at(rgb, h, w, sy, sx, y, X);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c * plane + at] = view_value(t, c, mean_dev[c], std_dev[c]);
  if (kLabels) {
    const int r = nearest_tap(y, sy, h), s = nearest_tap(X, sx, w);
    labels[p.label_off / (int64_t)sizeof(int64_t) + (size_t)y * p.new_w + x] = semantic[(size_t)r * w + s];
  }
}

// Thread = one output pixel of a 32 x 8 tile.  The 768-byte table is read through the cache: 256 entries that every
// workgroup of the launch reads stay in L2 / the vector cache, and a workgroup would use 256 of them at most.  Staging it
// in LDS per workgroup (SPML_EXPORT_TABLE_LDS=1) measured the same, 16.1 against 16.5 us with equal minima:
// profiles/inference_io.md.
__global__ __launch_bounds__(kTileW * kTileH) void label_export(
    const int64_t* __restrict__ pred, int pred_h, int pred_w, int valid_h, int valid_w, int out_h, int out_w,
    const unsigned char* __restrict__ color_map, unsigned char* __restrict__ gray, unsigned char* __restrict__ rgb) {
  if (!export_ok(pred_h, pred_w, valid_h, valid_w, out_h, out_w)) return;
#if SPML_EXPORT_TABLE_LDS
  __shared__ unsigned char table[768];
  for (int i = threadIdx.x; i < 768; i += kTileW * kTileH) table[i] = color_map[i];
  __syncthreads();
  color_map = table;
#endif
  const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= out_w || y >= out_h) return;
  const int r = nearest_tap(y, axis_scale(valid_h, out_h), valid_h), s = nearest_tap(x, axis_scale(valid_w, out_w), valid_w);
  const unsigned char g = (unsigned char)pred[(size_t)r * pred_w + s];
  const size_t at = (size_t)y * out_w + x;
  gray[at] = g;
  rgb[at * 3 + 0] = color_map[g * 3 + 0];
  rgb[at * 3 + 1] = color_map[g * 3 + 1];
  rgb[at * 3 + 2] = color_map[g * 3 + 2];
}

// ---- the CRF's guide image -------------------------------------------------------------------------
// The reference hands its CRF the uint8 image it rebuilds from the network's normalised fp32 input
// (inference_softmax_crf_msc.py:159-164): image *= std, image += mean (float32 by float64: numpy computes in float64 and
// rounds each result to float32), * 255 in float32, truncate.  The round trip is lossy -- with the VOC statistics 129 of
// the 768 (byte, channel) pairs come back one lower -- so the file's bytes are not the guide; this chain on the value
// image_views writes is.
struct guide_stats { double std64[3], mean64[3]; };        // the config's values, by value in the kernel arguments

__device__ __forceinline__ unsigned char guide_byte(float v, double std64, double mean64) {
  float t = (float)((double)v * std64);
  t = (float)((double)t + mean64);
  t = t * 255.0f;
  return (unsigned char)((int)t & 255);
}

__host__ __device__ inline bool guide_ok(int h, int w, int new_h, int new_w) {
  return h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide && new_h >= 1 && new_w >= 1 && new_h <= kMaxSide &&
         new_w <= kMaxSide;
}

// new == src: the view holds the normalised byte itself, so the guide is a function of (byte, channel) alone.  Every
// workgroup evaluates the chain for the 768 pairs into LDS (three per thread; no fp64 per pixel), then streams the
// image through the table in 12-byte spans: three dwords = four pixels per lane, so byte k of a span is channel k % 3
// in every lane and a wave moves 768 contiguous bytes per instruction.  The last n % 12 bytes go one per thread.
constexpr int kGuideThreads = 256, kGuideSpan = 12, kGuideMaxBlocks = 2048;
struct guide_span { unsigned int d[3]; };

__global__ __launch_bounds__(kGuideThreads) void crf_guide_table(
    const unsigned char* __restrict__ rgb, size_t n, const float* __restrict__ mean_dev,
    const float* __restrict__ std_dev, guide_stats stats, unsigned char* __restrict__ guide) {
  __shared__ unsigned char table[3 * 256];                               // [channel][byte]
  for (int i = threadIdx.x; i < 3 * 256; i += kGuideThreads) {
    const int c = i >> 8;
    table[i] = guide_byte(normalised((unsigned char)(i & 255), mean_dev[c], std_dev[c]), stats.std64[c], stats.mean64[c]);
  }
  __syncthreads();
  const size_t spans = n / kGuideSpan;
  const guide_span* in = reinterpret_cast<const guide_span*>(rgb);
  guide_span* out = reinterpret_cast<guide_span*>(guide);
  for (size_t i = (size_t)blockIdx.x * kGuideThreads + threadIdx.x; i < spans; i += (size_t)gridDim.x * kGuideThreads) {
    const guide_span v = in[i];
    guide_span o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      unsigned int word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        word |= (unsigned int)table[((4 * k + b) % 3) * 256 + ((v.d[k] >> (8 * b)) & 255u)] << (8 * b);
      o.d[k] = word;
    }
    out[i] = o;
  }
  if (blockIdx.x == 0) {
    const size_t at = spans * kGuideSpan + threadIdx.x;                  // (spans * 12 is a multiple of 3)
    if (threadIdx.x < kGuideSpan && at < n) guide[at] = table[(threadIdx.x % 3) * 256 + rgb[at]];
  }
}

// Every other size: four taps per channel (the code of image_views), then the chain.  Thread = one output pixel of a
// 32 x 8 tile.
__global__ __launch_bounds__(kTileW * kTileH) void crf_guide_resized(
    const unsigned char* __restrict__ rgb, int h, int w, const float* __restrict__ mean_dev,
    const float* __restrict__ std_dev, guide_stats stats, int new_h, int new_w, unsigned char* __restrict__ guide) {
  if (!guide_ok(h, w, new_h, new_w)) return;
  const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= new_w || y >= new_h) return;
  const view_taps t = taps_at(rgb, h, w, axis_scale(h, new_h), axis_scale(w, new_w), y, x);
  unsigned char* out = guide + ((size_t)y * new_w + x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[c] = guide_byte(view_value(t, c, mean_dev[c], std_dev[c]), stats.std64[c], stats.mean64[c]);
}

// ---- the CRF tail of a file: both exports, both scores and the compare in one launch ------------------------------
// label_export for `refined`, the same index and cast for `before`; every workgroup counts its tile into an int32 LDS
// table [2][3][ncls] (+ the differing pixels) and adds its non-zero bins into `scores` with 64-bit integer atomics:
// sums of integers, the same bits in any order.
constexpr int kMaxScoreClasses = 256;

__global__ __launch_bounds__(kTileW * kTileH) void label_export_scored(
    const int64_t* __restrict__ refined, const int64_t* __restrict__ before, int pred_h, int pred_w, int valid_h,
    int valid_w, int out_h, int out_w, const unsigned char* __restrict__ color_map,
    const unsigned char* __restrict__ truth, int ncls, unsigned char* __restrict__ gray, unsigned char* __restrict__ rgb,
    unsigned long long* __restrict__ scores) {
  if (!export_ok(pred_h, pred_w, valid_h, valid_w, out_h, out_w) || ncls < 1 || ncls > kMaxScoreClasses) return;
  __shared__ int bins[2 * 3 * kMaxScoreClasses + 1];
  const int n_bins = 2 * 3 * ncls;                                       // bins[n_bins]: the pixels the CRF changed
  for (int i = threadIdx.x; i <= n_bins; i += kTileW * kTileH) bins[i] = 0;
  __syncthreads();
  const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x < out_w && y < out_h) {
    const int r = nearest_tap(y, axis_scale(valid_h, out_h), valid_h), s = nearest_tap(x, axis_scale(valid_w, out_w), valid_w);
    const size_t from = (size_t)r * pred_w + s, at = (size_t)y * out_w + x;
    const unsigned char g = (unsigned char)refined[from];
    gray[at] = g;
    rgb[at * 3 + 0] = color_map[g * 3 + 0];
    rgb[at * 3 + 1] = color_map[g * 3 + 1];
    rgb[at * 3 + 2] = color_map[g * 3 + 2];
    const int t = truth ? (int)truth[at] : ncls;                         // (>= ncls: the pixel counts nowhere)
    if (t < ncls) {
      atomicAdd(&bins[t], 1);
      if (g < ncls) atomicAdd(&bins[ncls + g], 1);
      if (g == t) atomicAdd(&bins[2 * ncls + t], 1);
    }
    if (before) {
      const unsigned char gb = (unsigned char)before[from];
      if (t < ncls) {
        atomicAdd(&bins[3 * ncls + t], 1);
        if (gb < ncls) atomicAdd(&bins[4 * ncls + gb], 1);
        if (gb == t) atomicAdd(&bins[5 * ncls + t], 1);
      }
      if (gb != g) atomicAdd(&bins[n_bins], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= n_bins; i += kTileW * kTileH)
    if (bins[i] != 0) atomicAdd(&scores[i], (unsigned long long)bins[i]);
}

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_view_params_bytes(void) { return sizeof(spml_view_params); }

extern "C" const char* spml_image_views_path_name(const spml_view_params* records, int V, int h, int w,
                                                  int64_t image_bytes, int64_t label_bytes, int with_labels) {
  if (!views_ok(records, V, h, w, image_bytes, label_bytes, with_labels != 0)) return "unsupported";
  return with_labels ? "views+labels" : "views";
}

extern "C" int spml_image_views_u8(const unsigned char* rgb, const unsigned char* semantic, int h, int w,
                                   const float* mean, const float* std, const spml_view_params* params_host,
                                   const spml_view_params* params_dev, int V, float* images, int64_t image_bytes,
                                   int64_t* labels, int64_t label_bytes, void* stream) {
  if (!rgb || !mean || !std || !params_host || !params_dev || !images || image_bytes < 0) return SPML_ERR_INVALID_ARG;
  if ((semantic != nullptr) != (labels != nullptr) || (labels && label_bytes < 0)) return SPML_ERR_INVALID_ARG;
  if (((uintptr_t)params_dev & 7) != 0 || ((uintptr_t)images & 15) != 0 || ((uintptr_t)labels & 15) != 0 ||
      ((uintptr_t)mean & 3) != 0 || ((uintptr_t)std & 3) != 0)
    return SPML_ERR_INVALID_ARG;
  const bool with_labels = labels != nullptr;
  if (!views_ok(params_host, V, h, w, image_bytes, with_labels ? label_bytes : 0, with_labels))
    return SPML_ERR_UNSUPPORTED;
  const size_t px = (size_t)h * w;
  const void* written[2] = {images, labels};
  const size_t written_bytes[2] = {(size_t)image_bytes, with_labels ? (size_t)label_bytes : 0};
  for (int i = 0; i < 2; ++i)
    if (overlap(written[i], written_bytes[i], rgb, 3 * px) || overlap(written[i], written_bytes[i], semantic, px) ||
        overlap(written[i], written_bytes[i], params_dev, (size_t)V * sizeof(spml_view_params)) ||
        overlap(written[i], written_bytes[i], mean, 12) || overlap(written[i], written_bytes[i], std, 12))
      return SPML_ERR_INVALID_ARG;
  if (overlap(images, written_bytes[0], labels, written_bytes[1])) return SPML_ERR_INVALID_ARG;
  int max_h = 0, max_w = 0;
  for (int v = 0; v < V; ++v) {
    max_h = params_host[v].pad_h > max_h ? params_host[v].pad_h : max_h;
    max_w = params_host[v].pad_w > max_w ? params_host[v].pad_w : max_w;
  }
  const dim3 grid((unsigned)((max_w + kTileW - 1) / kTileW), (unsigned)((max_h + kTileH - 1) / kTileH), (unsigned)V);
  hipLaunchKernelGGL(with_labels ? image_views<true> : image_views<false>, grid, dim3(kTileW * kTileH), 0,
                     (hipStream_t)stream, rgb, semantic, h, w, mean, std, params_dev, images, image_bytes, labels,
                     with_labels ? label_bytes : (int64_t)0);
  return launch_status();
}

extern "C" const char* spml_label_export_path_name(int pred_h, int pred_w, int valid_h, int valid_w, int out_h,
                                                   int out_w) {
  return export_ok(pred_h, pred_w, valid_h, valid_w, out_h, out_w) ? "export" : "unsupported";
}

extern "C" int spml_label_export_u8(const int64_t* prediction, int pred_h, int pred_w, int valid_h, int valid_w,
                                    int out_h, int out_w, const unsigned char* color_map, unsigned char* gray,
                                    unsigned char* rgb, void* stream) {
  if (!prediction || !color_map || !gray || !rgb || ((uintptr_t)prediction & 7) != 0) return SPML_ERR_INVALID_ARG;
  if (!export_ok(pred_h, pred_w, valid_h, valid_w, out_h, out_w)) return SPML_ERR_UNSUPPORTED;
  const size_t px = (size_t)out_h * out_w, pred_bytes = (size_t)pred_h * pred_w * sizeof(int64_t);
  if (overlap(gray, px, prediction, pred_bytes) || overlap(rgb, 3 * px, prediction, pred_bytes) ||
      overlap(gray, px, color_map, 768) || overlap(rgb, 3 * px, color_map, 768) || overlap(gray, px, rgb, 3 * px))
    return SPML_ERR_INVALID_ARG;
  const dim3 grid((unsigned)((out_w + kTileW - 1) / kTileW), (unsigned)((out_h + kTileH - 1) / kTileH));
  hipLaunchKernelGGL(label_export, grid, dim3(kTileW * kTileH), 0, (hipStream_t)stream, prediction, pred_h, pred_w,
                     valid_h, valid_w, out_h, out_w, color_map, gray, rgb);
  return launch_status();
}

extern "C" const char* spml_crf_guide_path_name(int h, int w, int new_h, int new_w) {
  if (!guide_ok(h, w, new_h, new_w)) return "unsupported";
  return new_h == h && new_w == w ? "guide_table" : "guide_resized";
}

extern "C" int spml_crf_guide_u8(const unsigned char* rgb, int h, int w, const float* mean, const float* std,
                                 const double* mean64_host, const double* std64_host, int new_h, int new_w,
                                 unsigned char* guide, void* stream) {
  if (!rgb || !mean || !std || !mean64_host || !std64_host || !guide) return SPML_ERR_INVALID_ARG;
  if (((uintptr_t)rgb & 3) != 0 || ((uintptr_t)guide & 3) != 0 || ((uintptr_t)mean & 3) != 0 || ((uintptr_t)std & 3) != 0)
    return SPML_ERR_INVALID_ARG;                                         // (the table path moves dwords)
  if (!guide_ok(h, w, new_h, new_w)) return SPML_ERR_UNSUPPORTED;
  const size_t n = 3 * (size_t)new_h * new_w;
  if (overlap(guide, n, rgb, 3 * (size_t)h * w) || overlap(guide, n, mean, 12) || overlap(guide, n, std, 12))
    return SPML_ERR_INVALID_ARG;
  guide_stats stats;
  for (int c = 0; c < 3; ++c) {
    stats.std64[c] = std64_host[c];
    stats.mean64[c] = mean64_host[c];
  }
  if (new_h == h && new_w == w) {
    const size_t blocks = (n / kGuideSpan + kGuideThreads - 1) / kGuideThreads;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : blocks > (size_t)kGuideMaxBlocks ? (size_t)kGuideMaxBlocks : blocks);
    hipLaunchKernelGGL(crf_guide_table, dim3(grid), dim3(kGuideThreads), 0, (hipStream_t)stream, rgb, n, mean, std, stats,
                       guide);
  } else {
    const dim3 grid((unsigned)((new_w + kTileW - 1) / kTileW), (unsigned)((new_h + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(crf_guide_resized, grid, dim3(kTileW * kTileH), 0, (hipStream_t)stream, rgb, h, w, mean, std, stats,
                       new_h, new_w, guide);
  }
  return launch_status();
}

extern "C" size_t spml_export_scores_bytes(int ncls) {
  return ncls >= 1 && ncls <= kMaxScoreClasses ? (size_t)(2 * 3 * ncls + 1) * sizeof(int64_t) : 0;
}

extern "C" int spml_label_export_scored_u8(const int64_t* refined, const int64_t* before, int pred_h, int pred_w,
                                           int valid_h, int valid_w, int out_h, int out_w,
                                           const unsigned char* color_map, const unsigned char* truth, int ncls,
                                           unsigned char* gray, unsigned char* rgb, int64_t* scores, void* stream) {
  if (!refined || !color_map || !gray || !rgb || !scores) return SPML_ERR_INVALID_ARG;
  if (((uintptr_t)refined & 7) != 0 || ((uintptr_t)before & 7) != 0 || ((uintptr_t)scores & 7) != 0)
    return SPML_ERR_INVALID_ARG;
  if (!export_ok(pred_h, pred_w, valid_h, valid_w, out_h, out_w) || spml_export_scores_bytes(ncls) == 0)
    return SPML_ERR_UNSUPPORTED;
  const size_t px = (size_t)out_h * out_w, pred_bytes = (size_t)pred_h * pred_w * sizeof(int64_t);
  const void* written[3] = {gray, rgb, scores};
  const size_t written_bytes[3] = {px, 3 * px, spml_export_scores_bytes(ncls)};
  for (int i = 0; i < 3; ++i) {
    if (overlap(written[i], written_bytes[i], refined, pred_bytes) || overlap(written[i], written_bytes[i], before, pred_bytes) ||
        overlap(written[i], written_bytes[i], color_map, 768) || overlap(written[i], written_bytes[i], truth, px))
      return SPML_ERR_INVALID_ARG;
    for (int j = i + 1; j < 3; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return SPML_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)((out_w + kTileW - 1) / kTileW), (unsigned)((out_h + kTileH - 1) / kTileH));
  hipLaunchKernelGGL(label_export_scored, grid, dim3(kTileW * kTileH), 0, (hipStream_t)stream, refined, before, pred_h,
                     pred_w, valid_h, valid_w, out_h, out_w, color_map, truth, ncls, gray, rgb,
                     reinterpret_cast<unsigned long long*>(scores));
  return launch_status();
}
