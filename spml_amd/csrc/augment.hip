// N14: the training batch from raw decoded files -- the host-side augmentation chain of the reference's
// dataset classes (spml/data/datasets/base_dataset.py:135-155,183-186, list_tag_dataset.py:179-218,
// densepose_dataset.py:78-103,157-198 with spml/data/transforms.py) as ONE launch per batch:
//
//   augment_batch   packed u8 (RGB HWC + two label planes per image), one record per image
//                   -> image [B][3][S_h][S_w] fp32, semantic / instance label [B][S_h][S_w] int64
//   tag_flags       the semantic planes of the same buffer -> semantic_tag [B][256] int64 (list_tag_dataset.py:75-78)
//
// Every output pixel is composed BACKWARDS through the reference's stages: crop -> pad ('left_top') -> resize
// (cv2.resize: INTER_LINEAR on the image, INTER_NEAREST on the labels, no anti-aliasing) -> mirror (+ the label remap
// of DensePose), then forwards through grayscale, the 5x5 blur (reflect-101 at the crop's edges) and the normalisation.
// The source coordinates are formed in fp64 from the integers of the record exactly as the host library forms them
// (full-rate on CDNA; no per-image index tables to build and upload), so the label maps are bit-exact; contraction is
// off for the whole file: a fused (X + 0.5) * scale - 0.5 rounds once where the host rounds twice.
//
// blockIdx.z is the image: flip / gray / blur are uniform per workgroup.  Thread = one output pixel of a 32 x 8 tile,
// lanes along x: a wave stores two 128-byte row pieces per channel and two 256-byte pieces per label map.  A blurred
// image stages the (8 + 4) x (32 + 4) pre-blur values of its tile per channel in LDS once and takes the 25 taps from
// there; an un-blurred image never touches LDS.  No atomics, no inline assembly, no workspace.
#include "common.hpp"

#pragma clang fp contract(off)

namespace spml {
namespace {

constexpr int kTileW = 32, kTileH = 8, kHalo = 2;
constexpr int kStageW = kTileW + 2 * kHalo, kStageH = kTileH + 2 * kHalo;
constexpr int kMaxSide = 16384;                 // of a source, a resized image and the crop: h * w * 3 stays below 2^30
constexpr int kTagBlocks = 16;                  // workgroups per image of tag_flags

enum Path { kUnsupported = 0, kPlain = 1, kBlur = 2 };

__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }

// The one expression that decides what a record runs as -- the host entry (before anything is launched), the kernels
// (a record that fails writes nothing and forms no address) and spml_augment_path_name read it.
__host__ __device__ inline Path record_path(const spml_augment_params& p, int64_t packed_bytes, int S_h, int S_w) {
  if (S_h < 1 || S_w < 1 || S_h > kMaxSide || S_w > kMaxSide) return kUnsupported;
  if (p.h < 1 || p.w < 1 || p.h > kMaxSide || p.w > kMaxSide) return kUnsupported;
  if (p.new_h < 1 || p.new_w < 1 || p.new_h > kMaxSide || p.new_w > kMaxSide) return kUnsupported;
  if (p.start_h < 0 || p.start_h > imax(p.new_h, S_h) - S_h) return kUnsupported;
  if (p.start_w < 0 || p.start_w > imax(p.new_w, S_w) - S_w) return kUnsupported;
  const int64_t px = (int64_t)p.h * p.w;
  if (p.image_off < 0 || p.image_off > packed_bytes - 3 * px) return kUnsupported;
  if (p.sem_off < 0 || p.sem_off > packed_bytes - px) return kUnsupported;
  if (p.inst_off < 0 || p.inst_off > packed_bytes - px) return kUnsupported;
  if (p.blur && (S_h <= kHalo || S_w <= kHalo)) return kUnsupported;      // one reflection per side
  return p.blur ? kBlur : kPlain;
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

struct Rgb { float c[3]; };

// The cropped, padded, grey-or-not, not yet normalised image at crop coordinates (y, x), 0 <= y < S_h, 0 <= x < S_w.
__device__ __forceinline__ Rgb pre_blur(const spml_augment_params& p, const unsigned char* __restrict__ rgb, double sy,
                                        double sx, const float (&mean)[3], int y, int x) {
  const int Y = y + p.start_h, X = x + p.start_w;
  Rgb v;
  if (Y < p.new_h && X < p.new_w) {
    int y0, x0;
    float fy, fx;
    linear_tap(Y, sy, p.h, y0, fy);
    linear_tap(X, sx, p.w, x0, fx);
    const int y1 = y0 + 1 < p.h ? y0 + 1 : y0, x1 = x0 + 1 < p.w ? x0 + 1 : x0;      // (weight 0 where clamped)
    const int c0 = p.flip ? p.w - 1 - x0 : x0, c1 = p.flip ? p.w - 1 - x1 : x1;
    const unsigned char* r0 = rgb + (size_t)y0 * p.w * 3;
    const unsigned char* r1 = rgb + (size_t)y1 * p.w * 3;
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = (float)r0[c0 * 3 + c] / 255.f, v01 = (float)r0[c1 * 3 + c] / 255.f;
      const float v10 = (float)r1[c0 * 3 + c] / 255.f, v11 = (float)r1[c1 * 3 + c] / 255.f;
      v.c[c] = b0 * (a0 * v00 + a1 * v01) + b1 * (a0 * v10 + a1 * v11);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v.c[c] = mean[c];
  }
  if (p.gray) {
    const float g = (v.c[0] * 0.3f + v.c[1] * 0.59f) + v.c[2] * 0.11f;
    v.c[0] = v.c[1] = v.c[2] = g;
  }
  return v;
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(kTileW * kTileH) void augment_batch(
    const unsigned char* __restrict__ packed, int64_t packed_bytes, const spml_augment_params* __restrict__ params,
    const float* __restrict__ mean_dev, const float* __restrict__ std_dev, const unsigned char* __restrict__ remap,
    int S_h, int S_w, float* __restrict__ image, int64_t* __restrict__ sem_out, int64_t* __restrict__ inst_out) {
  __shared__ float stage[3][kStageH][kStageW + 1];
  const int b = blockIdx.z;
  const spml_augment_params p = params[b];
  const Path path = record_path(p, packed_bytes, S_h, S_w);
  if (path == kUnsupported) return;                          // (the host entry refused it already: never reached)
  const float mean[3] = {mean_dev[0], mean_dev[1], mean_dev[2]};
  const double sy = axis_scale(p.h, p.new_h), sx = axis_scale(p.w, p.new_w);
  const unsigned char* rgb = packed + p.image_off;
  const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < S_w && y < S_h;

  Rgb v;
  if (path == kBlur) {                                       // (workgroup-uniform)
    for (int i = threadIdx.x; i < kStageH * kStageW; i += kTileW * kTileH) {
      const int ly = i / kStageW, lx = i - ly * kStageW;
      const int gy = y0 + ly - kHalo, gx = x0 + lx - kHalo;
      // positions past the crop's far edge by more than the halo are read by no pixel that is stored
      if (gy < S_h + kHalo && gx < S_w + kHalo) {
        const Rgb s = pre_blur(p, rgb, sy, sx, mean, reflect101(gy, S_h), reflect101(gx, S_w));
        stage[0][ly][lx] = s.c[0];
        stage[1][ly][lx] = s.c[1];
        stage[2][ly][lx] = s.c[2];
      }
    }
    __syncthreads();
    if (inside) {
      v.c[0] = v.c[1] = v.c[2] = 0.f;
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const float wgt = p.weights[i * 5 + j];
#pragma unroll
          for (int c = 0; c < 3; ++c) v.c[c] = fmaf(wgt, stage[c][ty + i][tx + j], v.c[c]);
        }
    }
  } else if (inside) {
    v = pre_blur(p, rgb, sy, sx, mean, y, x);
  }
  if (!inside) return;

  const size_t plane = (size_t)S_h * S_w, at = (size_t)y * S_w + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) image[((size_t)b * 3 + c) * plane + at] = (v.c[c] - mean[c]) / std_dev[c];

  const int Y = y + p.start_h, X = x + p.start_w;
  int64_t sem = 255, inst = 255;
  if (Y < p.new_h && X < p.new_w) {
    const int r = nearest_tap(Y, sy, p.h), s = nearest_tap(X, sx, p.w);
    const size_t src = (size_t)r * p.w + (p.flip ? p.w - 1 - s : s);
    const unsigned char a = packed[p.sem_off + src];
    sem = p.flip ? remap[a] : a;
    inst = packed[p.inst_off + src];
  }
  sem_out[(size_t)b * plane + at] = sem;
  inst_out[(size_t)b * plane + at] = inst;
}

// 256 flags per workgroup in LDS, then plain stores of 1 (the entry zeroes `tags` on the stream first; several
// workgroups of an image may store the same 1)
__global__ __launch_bounds__(256) void tag_flags(const unsigned char* __restrict__ packed, int64_t packed_bytes,
                                                 const spml_augment_params* __restrict__ params,
                                                 int64_t* __restrict__ tags) {
  __shared__ int flag[256];
  const int b = blockIdx.y;
  const spml_augment_params p = params[b];
  const int64_t px = (int64_t)p.h * p.w;
  if (p.h < 1 || p.w < 1 || p.h > kMaxSide || p.w > kMaxSide || p.sem_off < 0 || p.sem_off > packed_bytes - px) return;
  flag[threadIdx.x] = 0;
  __syncthreads();
  const unsigned char* sem = packed + p.sem_off;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (int64_t)kTagBlocks * 256) flag[sem[i]] = 1;
  __syncthreads();
  if (flag[threadIdx.x]) tags[(size_t)b * 256 + threadIdx.x] = 1;
}

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_augment_params_bytes(void) { return sizeof(spml_augment_params); }

extern "C" const char* spml_augment_path_name(const spml_augment_params* record, int64_t packed_bytes, int S_h,
                                              int S_w) {
  if (!record) return "unsupported";
  const Path path = record_path(*record, packed_bytes, S_h, S_w);
  return path == kBlur ? "blur" : (path == kPlain ? "plain" : "unsupported");
}

extern "C" int spml_augment_batch_u8(const unsigned char* packed, int64_t packed_bytes,
                                     const spml_augment_params* params_host, const spml_augment_params* params_dev,
                                     int B, const float* mean, const float* std, const unsigned char* remap, int S_h,
                                     int S_w, float* image, int64_t* semantic_label, int64_t* instance_label,
                                     void* stream) {
  if (!packed || packed_bytes < 0 || !params_host || !params_dev || B < 1 || !mean || !std || !remap || !image ||
      !semantic_label || !instance_label)
    return SPML_ERR_INVALID_ARG;
  if (((uintptr_t)params_dev & 7) != 0 || ((uintptr_t)image & 3) != 0 || ((uintptr_t)semantic_label & 7) != 0 ||
      ((uintptr_t)instance_label & 7) != 0 || ((uintptr_t)mean & 3) != 0 || ((uintptr_t)std & 3) != 0)
    return SPML_ERR_INVALID_ARG;
  if (B > 65535) return SPML_ERR_UNSUPPORTED;                  // gridDim.z
  for (int b = 0; b < B; ++b)
    if (record_path(params_host[b], packed_bytes, S_h, S_w) == kUnsupported) return SPML_ERR_UNSUPPORTED;
  const size_t plane = (size_t)S_h * S_w;
  const void* written[3] = {image, semantic_label, instance_label};
  const size_t written_bytes[3] = {(size_t)B * 3 * plane * sizeof(float), (size_t)B * plane * sizeof(int64_t),
                                   (size_t)B * plane * sizeof(int64_t)};
  for (int i = 0; i < 3; ++i) {
    if (overlap(written[i], written_bytes[i], packed, (size_t)packed_bytes) ||
        overlap(written[i], written_bytes[i], params_dev, (size_t)B * sizeof(spml_augment_params)) ||
        overlap(written[i], written_bytes[i], remap, 256) || overlap(written[i], written_bytes[i], mean, 12) ||
        overlap(written[i], written_bytes[i], std, 12))
      return SPML_ERR_INVALID_ARG;
    for (int j = i + 1; j < 3; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return SPML_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)((S_w + kTileW - 1) / kTileW), (unsigned)((S_h + kTileH - 1) / kTileH), (unsigned)B);
  hipLaunchKernelGGL(augment_batch, grid, dim3(kTileW * kTileH), 0, (hipStream_t)stream, packed, packed_bytes,
                     params_dev, mean, std, remap, S_h, S_w, image, semantic_label, instance_label);
  return launch_status();
}

extern "C" int spml_augment_tags_u8(const unsigned char* packed, int64_t packed_bytes,
                                    const spml_augment_params* params_host, const spml_augment_params* params_dev,
                                    int B, int64_t* semantic_tag, void* stream) {
  if (!packed || packed_bytes < 0 || !params_host || !params_dev || B < 1 || !semantic_tag) return SPML_ERR_INVALID_ARG;
  if (((uintptr_t)params_dev & 7) != 0 || ((uintptr_t)semantic_tag & 7) != 0) return SPML_ERR_INVALID_ARG;
  if (B > 65535) return SPML_ERR_UNSUPPORTED;                  // gridDim.y
  for (int b = 0; b < B; ++b) {
    const spml_augment_params& p = params_host[b];
    if (p.h < 1 || p.w < 1 || p.h > kMaxSide || p.w > kMaxSide || p.sem_off < 0 ||
        p.sem_off > packed_bytes - (int64_t)p.h * p.w)
      return SPML_ERR_UNSUPPORTED;
  }
  const size_t tag_bytes = (size_t)B * 256 * sizeof(int64_t);
  if (overlap(semantic_tag, tag_bytes, packed, (size_t)packed_bytes) ||
      overlap(semantic_tag, tag_bytes, params_dev, (size_t)B * sizeof(spml_augment_params)))
    return SPML_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(semantic_tag, 0, tag_bytes, s) != hipSuccess) return SPML_ERR_LAUNCH;
  hipLaunchKernelGGL(tag_flags, dim3(kTagBlocks, (unsigned)B), dim3(256), 0, s, packed, packed_bytes, params_dev,
                     semantic_tag);
  return launch_status();
}
