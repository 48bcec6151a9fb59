// Full-resolution softmax inference (the label-map end of every recipe):
// pyscripts/inference/inference_softmax.py:105-148 with spml/models/predictions/softmax_classifier.py:37-90
// in eval mode.  Per sliding-window crop the reference runs, as framework ops, a channel normalisation, a 3x3
// convolution C -> 2C, batch norm, ReLU, a 1x1 convolution 2C -> num_classes and
// `outputs[..., sh:eh, sw:ew] += crop_out`; after the last crop an arg-max over the canvas; and
// pyscripts/benchmark/benchmark_by_mIoU.py:25-53 counts the label map against the ground truth.  Here:
//
//   unit_hl8_from_nchw    embedding NCHW fp32 -> x / |x| as the split-f16 A operand of the convolution (one pass)
//   (spml_conv_hl8_affine_f32 of conv.hip: 3x3 + folded batch norm + ReLU -> hidden [pixels][2C] fp32)
//   class_head_accumulate hidden x W^T + bias on the fp32-input matrix cores, added into the canvas window
//   argmax_channels       canvas -> int64 label map of the un-padded region
//   iou_counts            (TP+FN, TP+FP, TP) per class, integer atomics
#include "common.hpp"

#include <algorithm>

namespace spml {
namespace {

// ---------------------------------------------------------------------------------------
// x [n][C][hw] fp32 -> hl8 [n*hw][C] of x / |x|_2 over the channels.  A unit row is bounded by 1, so the scale of the
// split is fixed: S = 2^13, what conv.hip's pow2_scale gives for *bound == 1.0f (the caller hands that bound over).
// Workgroup = 64 consecutive pixels of one image x all channels: plane reads are 256-B runs per wave instruction, the
// tile is transposed through LDS ([C][65] floats), the hl8 rows of the 64 pixels are one contiguous run of the output.
constexpr float kUnitScale = 8192.0f;
constexpr int kUnitPix = 64;

__global__ __launch_bounds__(256) void unit_hl8_from_nchw(const float* __restrict__ x, int C, int64_t hw,
                                                          uint4* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* tile = reinterpret_cast<float*>(lds);              // [C][65]
  double* part = reinterpret_cast<double*>(tile + (size_t)C * (kUnitPix + 1));   // [4][64] partial sums of squares, [64] 1/norm
  const int img = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * kUnitPix;
  const int px = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const bool live = p0 + px < hw;
  const float* src = x + (size_t)img * C * hw + p0 + px;
  // the norm in double (exact squares, one rounding in 1 / sqrt): the unit value is then ONE fp32 rounding away from
  // x / |x|, which leaves the 2^-22 of the split format to the split (the kernel is bound by its HBM traffic)
  double ss = 0.0;
  for (int c = grp; c < C; c += 4) {
    const float v = live ? src[(size_t)c * hw] : 0.f;
    tile[c * (kUnitPix + 1) + px] = v;
    ss += (double)v * (double)v;
  }
  part[grp * 64 + px] = ss;
  __syncthreads();
  if (grp == 0) {
    const double s2 = (part[px] + part[64 + px]) + (part[128 + px] + part[192 + px]);
    // softmax_classifier.py:53-54 divides without an epsilon; a zero-norm pixel (NaN there) is written as zeros
    part[256 + px] = s2 > 0.0 ? (double)kUnitScale / sqrt(s2) : 0.0;
  }
  __syncthreads();
  const int upp = C >> 3;                                     // 8-channel units per pixel
  const int64_t row0 = (int64_t)img * hw + p0;
  for (int i = threadIdx.x; i < kUnitPix * upp; i += 256) {
    const int p = i / upp, u = i - p * upp;
    if (p0 + p >= hw) break;                                  // (p grows with i)
    const double inv = part[256 + p];
    union { half8 h; uint4 q; } hh, ll;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = (float)((double)tile[(u * 8 + e) * (kUnitPix + 1) + p] * inv);
      const _Float16 hj = (_Float16)v;
      hh.h[e] = hj;
      ll.h[e] = (_Float16)(v - (float)hj);
    }
    const size_t unit = ((size_t)(row0 + p) * upp + u) * 2;
    out[unit] = hh.q;
    out[unit + 1] = ll.q;
  }
}

// ---------------------------------------------------------------------------------------
// canvas[c][sh + y][sw + x] += sum_k hidden[y * w + x][k] * wgt[c][k] + bias[c]
// v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate) with A = weights (rows = classes), B = hidden^T
// (columns = pixels): the 32x32 result has the PIXEL on the lane (col = lane & 31) and the class in the registers
// (row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)), so that every register is two 128-byte runs of one class plane of
// the canvas -- the read-modify-write is coalesced along W as the accumulator stands, without a transpose.
// Wave = one tile of 32 consecutive crop pixels: its 32 * Ch floats are ONE contiguous run of `hidden`, read once
// with 16-byte loads into the wave's own LDS rows (stride Ch + 4 floats: the b128 fragment reads of 16 consecutive
// pixels fall into 16 different 16-byte slots).  A lane's fragment read is 4 consecutive k: MFMA j of k-block t sums
// k = 8t + j (lanes 0..31) and k = 8t + 4 + j (lanes 32..63); the weights are read from LDS with the same map.
// The weights ([NT * 32][Ch + 4], zero rows above ncls) stay in LDS for the whole launch.
constexpr int kHeadTile = 32;
constexpr int kHeadPre = 16;

template <int NT>
__global__ __launch_bounds__(512) void class_head_accumulate(const float* __restrict__ hidden, int Ch, int h, int w,
                                                            const float* __restrict__ wgt,
                                                            const float* __restrict__ bias, int ncls,
                                                            float* __restrict__ canvas, int Hp, int Wp, int sh,
                                                            int sw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int ld = Ch + 4;
  float* wl = reinterpret_cast<float*>(lds);                          // [NT * 32][ld]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  float* xl = wl + (size_t)NT * 32 * ld + (size_t)wave * kHeadTile * ld;   // [32][ld], this wave's
  const int c4 = Ch >> 2;
  for (int i = threadIdx.x; i < NT * 32 * c4; i += blockDim.x) {
    const int row = i / c4, col = (i - row * c4) * 4;
    float4v v = {0.f, 0.f, 0.f, 0.f};
    if (row < ncls) v = *reinterpret_cast<const float4v*>(wgt + (size_t)row * Ch + col);
    *reinterpret_cast<float4v*>(wl + row * ld + col) = v;
  }
  __syncthreads();

  const int64_t P = (int64_t)h * w;
  const int64_t tiles = (P + kHeadTile - 1) / kHeadTile;
  const size_t plane = (size_t)Hp * Wp;
  const int pl = lane & 31, half = lane >> 5;
  // Up to kHeadPre 16-byte loads per lane (Ch <= 128, ncls <= 32) are issued one tile AHEAD into registers, and the canvas values of
  // the current tile before its MFMAs: the HBM latency of both runs under the matrix-core work instead of in front of it.
  const int nld = kHeadTile * c4;                                      // float4s of a tile
  const bool ahead = NT == 1 && nld <= kHeadPre * 64;                  // wave-uniform (NT == 2 has no registers to spare)
  const int64_t step = (int64_t)gridDim.x * nwave;
  float4v pre[kHeadPre];
  auto fetch = [&](int64_t tile) {
    const int64_t left = (P - tile * kHeadTile) * c4;                  // float4s of `hidden` from the tile's start to its end
    const float4v* src = reinterpret_cast<const float4v*>(hidden + (size_t)tile * kHeadTile * Ch);
#pragma unroll
    for (int j = 0; j < kHeadPre; ++j) {
      const int i = j * 64 + lane;
      pre[j] = float4v{0.f, 0.f, 0.f, 0.f};
      if (i < nld && i < left) pre[j] = src[i];
    }
  };
  int64_t t = (int64_t)blockIdx.x * nwave + wave;
  if (ahead && t < tiles) fetch(t);
  for (; t < tiles; t += step) {
    const int64_t p0 = t * kHeadTile;
    if (ahead) {
#pragma unroll
      for (int j = 0; j < kHeadPre; ++j) {
        const int i = j * 64 + lane;
        if (i < nld) {
          const int row = i / c4, col = (i - row * c4) * 4;
          *reinterpret_cast<float4v*>(xl + row * ld + col) = pre[j];
        }
      }
    } else {
      const int64_t left = (P - p0) * c4;
      const float4v* src = reinterpret_cast<const float4v*>(hidden + (size_t)p0 * Ch);
      for (int i = lane; i < nld; i += 64) {
        const int row = i / c4, col = (i - row * c4) * 4;
        float4v v = {0.f, 0.f, 0.f, 0.f};
        if (i < left) v = src[i];
        *reinterpret_cast<float4v*>(xl + row * ld + col) = v;
      }
    }
    // the wave reads back what its own lanes wrote: LDS operations of one wave complete in order, the wave barriers
    // only keep the compiler from moving accesses across them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (ahead && t + step < tiles) fetch(t + step);
    const int64_t p = p0 + pl;
    const bool live = p < P;
    const int y = live ? (int)(p / w) : 0, x = live ? (int)(p - (int64_t)y * w) : 0;
    float* dst = canvas + (size_t)(sh + y) * Wp + (sw + x);           // (dead lanes: the window's first pixel, never accessed)
    float old[NT][16];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = n * 32 + acc_row(r, lane);
        old[n][r] = live && c < ncls ? dst[(size_t)c * plane] : 0.f;
      }
    float16v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const float* xb = xl + pl * ld + 4 * half;
    const float* wb = wl + pl * ld + 4 * half;
    for (int k = 0; k < Ch; k += 8) {
      const float4v b = *reinterpret_cast<const float4v*>(xb + k);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float4v a = *reinterpret_cast<const float4v*>(wb + (size_t)n * 32 * ld + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc[n], 0, 0, 0);
      }
    }
    // the LDS tile is free for the next iteration's stores once these reads were issued (in order within the wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (live) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = n * 32 + acc_row(r, lane);
          if (c < ncls) dst[(size_t)c * plane] = old[n][r] + (acc[n][r] + bias[c]);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------
// thread = one pixel of the top-left h x w region; the class planes are read along W (coalesced)
__global__ __launch_bounds__(256) void argmax_channels(const float* __restrict__ canvas, int ncls, int Hp, int Wp,
                                                       int h, int w, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)h * w) return;
  const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
  const float* src = canvas + (size_t)y * Wp + x;
  const size_t plane = (size_t)Hp * Wp;
  float best = src[0];
  int arg = 0;
  for (int c0 = 1; c0 < ncls; c0 += 8) {
    float v[8];                                  // eight planes in flight before the first comparison
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c0 + j < ncls ? src[(size_t)(c0 + j) * plane] : -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // strict '>' keeps the lowest index of a tie (the -inf fillers never win); a NaN wins over every number and
      // the first NaN is kept (what torch.argmax returns)
      if (v[j] > best || (v[j] != v[j] && best == best)) {
        best = v[j];
        arg = c0 + j;
      }
    }
  }
  out[i] = arg;
}

// ---------------------------------------------------------------------------------------
// per-workgroup LDS histograms [3][ncls] (32-bit: a workgroup sees fewer than 2^31 pixels), then one 64-bit integer
// atomic per non-zero bin: integer sums do not depend on the arrival order
__global__ __launch_bounds__(256) void iou_counts(const int64_t* __restrict__ pred, const int64_t* __restrict__ target,
                                                  int64_t n, int ncls, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned* hist = reinterpret_cast<unsigned*>(lds);
  for (int i = threadIdx.x; i < 3 * ncls; i += 256) hist[i] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i], p = pred[i];
    if (t < 0 || t >= ncls) continue;
    atomicAdd(hist + (int)t, 1u);
    if (p >= 0 && p < ncls) atomicAdd(hist + ncls + (int)p, 1u);
    if (p == t) atomicAdd(hist + 2 * ncls + (int)t, 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * ncls; i += 256)
    if (hist[i]) atomicAdd(out + i, (unsigned long long)hist[i]);
}

constexpr size_t kLdsLimit = 160 * 1024;

size_t head_lds_bytes(int nt, int waves, int Ch) {
  return (size_t)(nt * 32 + waves * kHeadTile) * (Ch + 4) * sizeof(float);
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" int spml_unit_hl8_from_nchw_f32(const float* x, int n, int C, int h, int w, void* out, void* stream) {
  if (!x || !out || n <= 0 || C <= 0 || h <= 0 || w <= 0) return SPML_ERR_INVALID_ARG;
  const size_t lds = (size_t)C * (kUnitPix + 1) * sizeof(float) + 5 * 64 * sizeof(double);
  if ((C & 15) || C > 512 || lds > kLdsLimit || n > 65535 || !al16(out)) return SPML_ERR_UNSUPPORTED;
  const int64_t hw = (int64_t)h * w;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(unit_hl8_from_nchw),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(unit_hl8_from_nchw, dim3((unsigned)((hw + kUnitPix - 1) / kUnitPix), (unsigned)n), dim3(256),
                     lds, (hipStream_t)stream, x, C, hw, static_cast<uint4*>(out));
  return launch_status();
}

extern "C" int spml_class_head_supported(int Ch, int ncls) {
  if (Ch <= 0 || (Ch & 31) || ncls <= 0 || ncls > 64) return 0;
  return head_lds_bytes(ncls > 32 ? 2 : 1, 1, Ch) <= kLdsLimit;
}

extern "C" int spml_class_head_accumulate_f32(const float* hidden, int Ch, int h, int w, const float* weight,
                                              const float* bias, int ncls, float* canvas, int Hp, int Wp, int sh,
                                              int sw, void* stream) {
  if (!hidden || !weight || !bias || !canvas || Ch <= 0 || ncls <= 0 || h <= 0 || w <= 0 || Hp <= 0 || Wp <= 0)
    return SPML_ERR_INVALID_ARG;
  if (sh < 0 || sw < 0 || (int64_t)sh + h > Hp || (int64_t)sw + w > Wp) return SPML_ERR_INVALID_ARG;
  if (!spml_class_head_supported(Ch, ncls) || !al16(hidden) || !al16(weight)) return SPML_ERR_UNSUPPORTED;
  const int nt = ncls > 32 ? 2 : 1;
  int waves = 8;                                        // two per SIMD where the LDS holds their tiles
  while (waves > 1 && head_lds_bytes(nt, waves, Ch) > kLdsLimit) waves >>= 1;
  const size_t lds = head_lds_bytes(nt, waves, Ch);
  const int64_t tiles = ((int64_t)h * w + kHeadTile - 1) / kHeadTile;
  const unsigned grid = (unsigned)std::min<int64_t>((tiles + waves - 1) / waves, 256);     // one workgroup per CU
  auto kern = nt == 2 ? class_head_accumulate<2> : class_head_accumulate<1>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * waves), lds, (hipStream_t)stream, hidden, Ch, h, w, weight, bias,
                     ncls, canvas, Hp, Wp, sh, sw);
  return launch_status();
}

extern "C" int spml_argmax_channels_i64(const float* canvas, int ncls, int Hp, int Wp, int h, int w, int64_t* out,
                                        void* stream) {
  if (!canvas || !out || ncls <= 0 || Hp <= 0 || Wp <= 0 || h <= 0 || w <= 0 || h > Hp || w > Wp)
    return SPML_ERR_INVALID_ARG;
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(argmax_channels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, canvas,
                     ncls, Hp, Wp, h, w, out);
  return launch_status();
}

extern "C" int spml_iou_counts_i64(const int64_t* pred, const int64_t* target, int64_t n, int ncls, int64_t* counts,
                                   void* stream) {
  if (!pred || !target || !counts || n <= 0 || ncls <= 0) return SPML_ERR_INVALID_ARG;
  if (ncls > 4096) return SPML_ERR_UNSUPPORTED;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(iou_counts, dim3(grid), dim3(256), 3 * (size_t)ncls * sizeof(unsigned), (hipStream_t)stream,
                     pred, target, n, ncls, reinterpret_cast<unsigned long long*>(counts));
  return launch_status();
}
