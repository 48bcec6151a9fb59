// N17: the picture of a training summary -- pyscripts/train/train.py:222-258 of the reference with
// spml/utils/general/vis.py:23-31,41-48,62-101 and common.py:29-73,101-120 -- without the embedding leaving the device:
//
//   pca_moments      embedding [N, C, H, W] fp32 -> mean[C], cov[C][C] fp64 of its L2-normalised pixels
//                    (column sums, then the Gram matrix of the CENTRED rows on the f32-input matrix instruction)
//   pca_project      embedding, V [C][3] -> proj [N, H, W, 3] = normalised row . V (un-centred, common.py:68) and the
//                    per-image, per-channel minimum and maximum of proj
//   summary_panels   labels, proj, extrema, colour table -> the finished uint8 picture, one launch
//
// Operand map of v_mfma_f32_32x32x2_f32: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], one fp32
// register each.  With i, j = channel and k = pixel, lane l holds channel c0 + (l & 31) of pixel p + (l >> 5) for both
// operands: in the channels-last layout a step of two pixels is one 256-byte load per 32 channels, straight from global
// memory.  The pixel's norm is a reduction over the 32 lanes of a half-wave, the mean one register per lane.
// NCHW-contiguous input is staged per 64-pixel tile through LDS (read along the pixels, consumed along the channels)
// into the same map.  A pixel past the end is masked to zero AFTER the centring: it adds nothing to the Gram matrix.
//
// No float atomics, no ticket, no inline assembly: every workgroup writes its partial to the workspace, a finishing
// kernel adds the partials in index order in fp64.  The results are bit-identical from call to call, in either
// deterministic mode.
#include "common.hpp"

#include <math.h>

#pragma clang fp contract(off)

namespace spml {
namespace {

constexpr int kTilePx = 64;             // pixels of a workgroup's tile: 32 operand steps, 8 per wave
constexpr int kPairs = kTilePx / 2 / 4; // operand steps per wave and tile
constexpr int kMaxGroups = 256;         // workgroups of a moment pass = partials the finishing kernel adds
constexpr int kMaxProjGroups = 64;      // workgroups of the projection per image
constexpr int kMaxSide = 16384;         // of a label map, a panel and the picture

enum { kLayoutNone = 0, kLayoutNhwc = 1, kLayoutNchw = 2 };

// The one expression that decides the route -- spml_pca_path_name and the two entries read it.
inline int pca_layout(int C, int64_t pixel_stride, int64_t channel_stride) {
  if (C != 32 && C != 64) return kLayoutNone;
  if (pixel_stride == C && channel_stride == 1) return kLayoutNhwc;
  if (pixel_stride == 1 && channel_stride >= 1) return kLayoutNchw;
  return kLayoutNone;
}

// P = N * H * W where it lies in [1, 2^31), else 0
inline int64_t pixel_count(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const int64_t lim = (int64_t)1 << 31;
  const int64_t hw = (int64_t)H * W;
  if (hw >= lim) return 0;
  const int64_t p = hw * N;
  return p < lim ? p : 0;
}

inline int moment_groups(int64_t P) {
  const int64_t g = ((P + kTilePx - 1) / kTilePx + 3) / 4;
  return (int)(g < 1 ? 1 : (g > kMaxGroups ? kMaxGroups : g));
}

inline int project_groups(int64_t hw) {
  const int64_t g = ((hw + kTilePx - 1) / kTilePx + 3) / 4;
  return (int)(g < 1 ? 1 : (g > kMaxProjGroups ? kMaxProjGroups : g));
}

// Workspace, in floats: mean32 [64] | column-sum partials [G][C] | Gram partials [G][C][C]; the projection uses its
// head as [N][Gp][3][2].
struct SummaryWs {
  size_t mean32, sums, gram, total;
};

inline SummaryWs summary_ws(int N, int C, int H, int W) {
  SummaryWs l = {0, 0, 0, 0};
  const int64_t P = pixel_count(N, H, W);
  if (P == 0 || (C != 32 && C != 64)) return l;
  const size_t G = (size_t)moment_groups(P);
  l.mean32 = 0;
  l.sums = 64;
  l.gram = l.sums + G * C;
  const size_t moments = l.gram + G * C * C;
  const size_t project = (size_t)N * project_groups((int64_t)H * W) * 6;
  l.total = (moments > project ? moments : project) * sizeof(float);
  return l;
}

// NCHW: one 64-pixel tile, read along the pixels (coalesced), stored [pixel][channel] with one float of padding per row.
template <int C>
__device__ __forceinline__ void stage_tile(const float* __restrict__ x, int64_t hw, float* tile, int64_t p0,
                                           int64_t limit) {
  const int px = threadIdx.x & (kTilePx - 1);
  const int64_t pix = p0 + px;
  const bool valid = pix < limit;
  const int64_t n = valid ? pix / hw : 0, s = valid ? pix - n * hw : 0;
  const float* src = x + (n * C) * hw + s;
#pragma unroll 4
  for (int c = threadIdx.x / kTilePx; c < C; c += 256 / kTilePx)
    tile[px * (C + 1) + c] = valid ? src[(int64_t)c * hw] : 0.f;
}

// The operand registers of step `pair` of the tile at p0: v[j] = channel 32 j + (lane & 31) of pixel
// p0 + 2 pair + (lane >> 5), zero past `limit`.  Returns whether this lane's pixel exists.
template <int C, bool kNchw>
__device__ __forceinline__ bool load_pair(const float* __restrict__ x, const float* tile, int64_t p0, int64_t limit,
                                          int pair, int lane, float (&v)[C / 32]) {
  const int px = 2 * pair + (lane >> 5);
  const int64_t pix = p0 + px;
  const bool valid = pix < limit;
#pragma unroll
  for (int j = 0; j < C / 32; ++j) {
    if (kNchw)
      v[j] = tile[px * (C + 1) + 32 * j + (lane & 31)];
    else
      v[j] = valid ? x[pix * C + 32 * j + (lane & 31)] : 0.f;
  }
  return valid;
}

__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// common.normalize_embedding: x / max(||x||, 1e-12); an all-zero pixel stays zero
template <int J>
__device__ __forceinline__ void normalize_pixel(float (&v)[J]) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) ss += v[j] * v[j];
  float norm = sqrtf(half_wave_sum(ss));
  norm = norm >= kEps ? norm : kEps;
#pragma unroll
  for (int j = 0; j < J; ++j) v[j] = v[j] / norm;
}

// kGram = false: partial[g][C] = this workgroup's column sums of the normalised rows.
// kGram = true:  partial[g][C][C] = its Gram matrix of the rows minus mean32.
template <int C, bool kNchw, bool kGram>
__global__ __launch_bounds__(256) void pca_moments(const float* __restrict__ x, int64_t P, int64_t hw,
                                                   const float* __restrict__ mean32, float* __restrict__ partial) {
  constexpr int J = C / 32;
  __shared__ float smem[kGram ? C * C : 4 * C];
  __shared__ float tile[kNchw ? kTilePx * (C + 1) : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m[J], s[J];
  float16v acc[J][J];
#pragma unroll
  for (int a = 0; a < J; ++a) {
    m[a] = kGram ? mean32[32 * a + (lane & 31)] : 0.f;
    s[a] = 0.f;
#pragma unroll
    for (int b = 0; b < J; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  }
  const int64_t tiles = (P + kTilePx - 1) / kTilePx;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {     // (the trip count is the workgroup's: barriers are safe)
    const int64_t p0 = t * kTilePx;
    if (kNchw) {
      __syncthreads();
      stage_tile<C>(x, hw, tile, p0, P);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < kPairs; ++i) {
      const int pair = wave + 4 * i;
      if (p0 + 2 * pair >= P) continue;                         // (wave-uniform)
      float v[J];
      const bool valid = load_pair<C, kNchw>(x, tile, p0, P, pair, lane, v);
      normalize_pixel<J>(v);
      if (kGram) {
#pragma unroll
        for (int a = 0; a < J; ++a) v[a] = valid ? v[a] - m[a] : 0.f;
#pragma unroll
        for (int a = 0; a < J; ++a)
#pragma unroll
          for (int b = 0; b < J; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[a], v[b], acc[a][b], 0, 0, 0);
      } else {
#pragma unroll
        for (int a = 0; a < J; ++a) s[a] += v[a];
      }
    }
  }
  if (kGram) {
    // the four waves, in wave order: D[row = channel of A][col = channel of B]
    for (int w = 0; w < 4; ++w) {
      if (wave == w) {
#pragma unroll
        for (int a = 0; a < J; ++a)
#pragma unroll
          for (int b = 0; b < J; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int at = (32 * a + acc_row(r, lane)) * C + 32 * b + (lane & 31);
              smem[at] = w == 0 ? acc[a][b][r] : smem[at] + acc[a][b][r];
            }
      }
      __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.x * C * C;
    for (int i = threadIdx.x; i < C * C; i += 256) out[i] = smem[i];
  } else {
#pragma unroll
    for (int a = 0; a < J; ++a) {
      s[a] += __shfl_xor(s[a], 32, kWave);
      if (lane < 32) smem[wave * C + 32 * a + lane] = s[a];
    }
    __syncthreads();
    if (threadIdx.x < C) {
      const int c = threadIdx.x;
      partial[(size_t)blockIdx.x * C + c] = ((smem[c] + smem[C + c]) + smem[2 * C + c]) + smem[3 * C + c];
    }
  }
}

__global__ __launch_bounds__(64) void pca_finish_mean(const float* __restrict__ partial, int G, int C, int64_t P,
                                                      double* __restrict__ mean, float* __restrict__ mean32) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += (double)partial[(size_t)g * C + c];
  const double m = s / (double)P;
  mean[c] = m;
  mean32[c] = (float)m;
}

__global__ __launch_bounds__(256) void pca_finish_cov(const float* __restrict__ partial, int G, int CC, double denom,
                                                     double* __restrict__ cov) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= CC) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += (double)partial[(size_t)g * CC + i];
  cov[i] = s / denom;
}

// blockIdx.y = image.  partial[(image * gridDim.x + blockIdx.x)][3][2] = (min, max) of this workgroup's pixels.
template <int C, bool kNchw>
__global__ __launch_bounds__(256) void pca_project(const float* __restrict__ x, int64_t hw, const float* __restrict__ V,
                                                   float* __restrict__ proj, float* __restrict__ partial) {
  constexpr int J = C / 32;
  __shared__ float smem[4 * 6];
  __shared__ float tile[kNchw ? kTilePx * (C + 1) : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float vv[J][3], mn[3], mx[3];
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) vv[j][k] = V[(32 * j + (lane & 31)) * 3 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mn[k] = INFINITY;
    mx[k] = -INFINITY;
  }
  const int64_t base = (int64_t)blockIdx.y * hw, limit = base + hw;
  const int64_t tiles = (hw + kTilePx - 1) / kTilePx;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t p0 = base + t * kTilePx;
    if (kNchw) {
      __syncthreads();
      stage_tile<C>(x, hw, tile, p0, limit);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < kPairs; ++i) {
      const int pair = wave + 4 * i;
      if (p0 + 2 * pair >= limit) continue;                     // (wave-uniform)
      float v[J];
      const bool valid = load_pair<C, kNchw>(x, tile, p0, limit, pair, lane, v);
      normalize_pixel<J>(v);
      float d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float dk = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) dk += v[j] * vv[j][k];
        d[k] = half_wave_sum(dk);
      }
      if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          mn[k] = fminf(mn[k], d[k]);
          mx[k] = fmaxf(mx[k], d[k]);
        }
        const int k = lane & 31;
        if (k < 3) proj[(p0 + 2 * pair + (lane >> 5)) * 3 + k] = k == 0 ? d[0] : (k == 1 ? d[1] : d[2]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mn[k] = fminf(mn[k], __shfl_xor(mn[k], 32, kWave));
    mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], 32, kWave));
    if (lane == 0) {
      smem[wave * 6 + 2 * k] = mn[k];
      smem[wave * 6 + 2 * k + 1] = mx[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int e = threadIdx.x;
    float r = smem[e];
    for (int w = 1; w < 4; ++w) r = (e & 1) ? fmaxf(r, smem[w * 6 + e]) : fminf(r, smem[w * 6 + e]);
    partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6 + e] = r;
  }
}

__global__ __launch_bounds__(256) void pca_finish_minmax(const float* __restrict__ partial, int groups, int N,
                                                         float* __restrict__ minmax) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= N * 6) return;
  const int img = id / 6, e = id - img * 6;
  float r = partial[(size_t)img * groups * 6 + e];
  for (int g = 1; g < groups; ++g) {
    const float o = partial[((size_t)img * groups + g) * 6 + e];
    r = (e & 1) ? fmaxf(r, o) : fminf(r, o);
  }
  minmax[id] = r;
}

// F.interpolate(mode='nearest') as ATen forms it: scale = (float)in / out, source = min((int)floorf(dst * scale), in - 1)
__device__ __forceinline__ int nearest_source(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

__host__ __device__ inline bool panels_ok(int N, int Hl, int Wl, int h, int w, int pad, int out_h, int out_w, bool grid) {
  if (N < 1 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return false;
  if ((int64_t)N * h * w >= ((int64_t)1 << 31)) return false;
  if (!grid) return true;
  if (Hl < 1 || Wl < 1 || Hl > kMaxSide || Wl > kMaxSide) return false;
  if (pad != 2 && !(pad == 0 && N == 1)) return false;
  if ((int64_t)out_h != (int64_t)N * (h + pad) + pad || (int64_t)out_w != 3 * (int64_t)w + 2 * pad) return false;
  if (out_h > 8 * 65535) return false;                          // (rows of 8 are gridDim.y)
  return 3 * (int64_t)out_h * out_w < ((int64_t)1 << 31);
}

// vis.py:92-95 in fp32, in that order, truncated; a constant channel gives 0 (the reference divides 0 by 0)
__device__ __forceinline__ unsigned char stretch_byte(float v, float mn, float mx) {
  const float range = mx - mn;
  if (!(range > 0.f)) return 0;
  const float t = ((v - mn) / range) * 255.f;
  return (unsigned char)(int)t;
}

// kGrid: thread = one pixel of the picture uint8 [3][out_h][out_w] (make_grid(nrow=1): image i at row pad + i (h + pad),
// column pad; per image semantic colour | instance colour | embedding, each h x w; everything else 0).
// !kGrid: blockIdx.z = image, out = uint8 [N][3][h][w], the embedding panel alone.
template <bool kGrid>
__global__ __launch_bounds__(256) void summary_panels(const int64_t* __restrict__ semantic,
                                                      const int64_t* __restrict__ instance, int N, int Hl, int Wl,
                                                      const float* __restrict__ proj, const float* __restrict__ minmax,
                                                      int h, int w, const unsigned char* __restrict__ color_map,
                                                      int pad, int out_h, int out_w, unsigned char* __restrict__ out) {
  if (!panels_ok(N, Hl, Wl, h, w, pad, out_h, out_w, kGrid)) return;
  const int X = blockIdx.x * 32 + (threadIdx.x & 31), Y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (!kGrid) {
    const int i = blockIdx.z;
    if (X >= w || Y >= h || i >= N) return;
    const size_t px = ((size_t)i * h + Y) * w + X;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[(((size_t)i * 3 + c) * h + Y) * w + X] = stretch_byte(proj[px * 3 + c], minmax[(i * 3 + c) * 2],
                                                              minmax[(i * 3 + c) * 2 + 1]);
    return;
  }
  if (X >= out_w || Y >= out_h) return;
  const size_t plane = (size_t)out_h * out_w, at = (size_t)Y * out_w + X;
  const int y = Y - pad, x = X - pad, cell = h + pad;
  const int i = y >= 0 ? y / cell : N, ry = y - i * cell;
  unsigned char rgb[3] = {0, 0, 0};
  if (i < N && ry < h && x >= 0 && x < 3 * w) {
    const int panel = x / w, cx = x - panel * w;
    if (panel < 2) {
      const int64_t* lab = (panel == 0 ? semantic : instance) + (size_t)i * Hl * Wl;
      const int sy = nearest_source(ry, Hl, h), sx = nearest_source(cx, Wl, w);
      const int entry = (int)(lab[(size_t)sy * Wl + sx] & 255);
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = color_map[entry * 3 + c];
    } else {
      const size_t px = ((size_t)i * h + ry) * w + cx;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        rgb[c] = stretch_byte(proj[px * 3 + c], minmax[(i * 3 + c) * 2], minmax[(i * 3 + c) * 2 + 1]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c * plane + at] = rgb[c];
}

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the checks the two embedding entries share: status, and the layout and pixel count where it is SPML_OK
inline int embedding_args(const float* emb, int N, int C, int H, int W, int64_t pixel_stride, int64_t channel_stride,
                          const void* ws, size_t ws_bytes, int& layout, int64_t& P) {
  if (!emb || misaligned(emb, 16)) return SPML_ERR_INVALID_ARG;
  layout = pca_layout(C, pixel_stride, channel_stride);
  P = pixel_count(N, H, W);
  if (layout == kLayoutNone || P == 0) return SPML_ERR_UNSUPPORTED;
  if (layout == kLayoutNchw && channel_stride != (int64_t)H * W) return SPML_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < summary_ws(N, C, H, W).total) return SPML_ERR_WORKSPACE;
  if (misaligned(ws, 16)) return SPML_ERR_INVALID_ARG;
  return SPML_OK;
}

template <int C, bool kNchw>
void launch_moments(const float* emb, int64_t P, int64_t hw, int G, const SummaryWs& l, float* ws, double* mean,
                    double* cov, hipStream_t s) {
  hipLaunchKernelGGL((pca_moments<C, kNchw, false>), dim3(G), dim3(256), 0, s, emb, P, hw, (const float*)nullptr,
                     ws + l.sums);
  hipLaunchKernelGGL(pca_finish_mean, dim3(1), dim3(64), 0, s, ws + l.sums, G, C, P, mean, ws + l.mean32);
  hipLaunchKernelGGL((pca_moments<C, kNchw, true>), dim3(G), dim3(256), 0, s, emb, P, hw, ws + l.mean32, ws + l.gram);
  hipLaunchKernelGGL(pca_finish_cov, dim3((C * C + 255) / 256), dim3(256), 0, s, ws + l.gram, G, C * C,
                     (double)(P > 1 ? P - 1 : 1), cov);
}

template <int C, bool kNchw>
void launch_project(const float* emb, int N, int64_t hw, int groups, const float* V, float* proj, float* minmax,
                    float* ws, hipStream_t s) {
  hipLaunchKernelGGL((pca_project<C, kNchw>), dim3(groups, N), dim3(256), 0, s, emb, hw, V, proj, ws);
  hipLaunchKernelGGL(pca_finish_minmax, dim3((N * 6 + 255) / 256), dim3(256), 0, s, ws, groups, N, minmax);
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_train_summary_workspace_bytes(int N, int C, int H, int W) { return summary_ws(N, C, H, W).total; }

extern "C" const char* spml_pca_path_name(int C, int64_t pixel_stride, int64_t channel_stride) {
  const int layout = pca_layout(C, pixel_stride, channel_stride);
  if (layout == kLayoutNone) return "unsupported";
  if (layout == kLayoutNhwc) return C == 32 ? "gram_mfma_f32_c32" : "gram_mfma_f32_c64";
  return C == 32 ? "gram_mfma_f32_c32_nchw" : "gram_mfma_f32_c64_nchw";
}

extern "C" int spml_pca_moments_f32(const float* emb, int N, int C, int H, int W, int64_t pixel_stride,
                                    int64_t channel_stride, double* mean, double* cov, void* ws, size_t ws_bytes,
                                    void* stream) {
  if (!mean || !cov || misaligned(mean, 16) || misaligned(cov, 16)) return SPML_ERR_INVALID_ARG;
  int layout;
  int64_t P;
  const int rc = embedding_args(emb, N, C, H, W, pixel_stride, channel_stride, ws, ws_bytes, layout, P);
  if (rc != SPML_OK) return rc;
  const SummaryWs l = summary_ws(N, C, H, W);
  const int G = moment_groups(P);
  const int64_t hw = (int64_t)H * W;
  hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  if (C == 32) {
    if (layout == kLayoutNchw) launch_moments<32, true>(emb, P, hw, G, l, w, mean, cov, s);
    else launch_moments<32, false>(emb, P, hw, G, l, w, mean, cov, s);
  } else {
    if (layout == kLayoutNchw) launch_moments<64, true>(emb, P, hw, G, l, w, mean, cov, s);
    else launch_moments<64, false>(emb, P, hw, G, l, w, mean, cov, s);
  }
  return launch_status();
}

extern "C" int spml_pca_project_minmax_f32(const float* emb, int N, int C, int H, int W, int64_t pixel_stride,
                                           int64_t channel_stride, const float* V, float* proj, float* minmax, void* ws,
                                           size_t ws_bytes, void* stream) {
  if (!V || !proj || !minmax || misaligned(V, 4) || misaligned(proj, 16) || misaligned(minmax, 4))
    return SPML_ERR_INVALID_ARG;
  int layout;
  int64_t P;
  const int rc = embedding_args(emb, N, C, H, W, pixel_stride, channel_stride, ws, ws_bytes, layout, P);
  if (rc != SPML_OK) return rc;
  if (N > 65535) return SPML_ERR_UNSUPPORTED;                   // (the image is gridDim.y)
  const int64_t hw = (int64_t)H * W;
  const int groups = project_groups(hw);
  hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  if (C == 32) {
    if (layout == kLayoutNchw) launch_project<32, true>(emb, N, hw, groups, V, proj, minmax, w, s);
    else launch_project<32, false>(emb, N, hw, groups, V, proj, minmax, w, s);
  } else {
    if (layout == kLayoutNchw) launch_project<64, true>(emb, N, hw, groups, V, proj, minmax, w, s);
    else launch_project<64, false>(emb, N, hw, groups, V, proj, minmax, w, s);
  }
  return launch_status();
}

extern "C" int spml_summary_panels_u8(const int64_t* semantic, const int64_t* instance, int N, int Hl, int Wl,
                                      const float* proj, const float* minmax, int h, int w,
                                      const unsigned char* color_map, int pad, int out_h, int out_w,
                                      unsigned char* out, void* stream) {
  const bool grid = semantic != nullptr;
  if ((semantic != nullptr) != (instance != nullptr) || (grid && !color_map)) return SPML_ERR_INVALID_ARG;
  if (!proj || !minmax || !out || misaligned(proj, 16) || misaligned(minmax, 4) || misaligned(semantic, 8) ||
      misaligned(instance, 8))
    return SPML_ERR_INVALID_ARG;
  if (!panels_ok(N, Hl, Wl, h, w, pad, out_h, out_w, grid)) return SPML_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (grid) {
    const dim3 g((unsigned)((out_w + 31) / 32), (unsigned)((out_h + 7) / 8));
    hipLaunchKernelGGL(summary_panels<true>, g, dim3(256), 0, s, semantic, instance, N, Hl, Wl, proj, minmax, h, w,
                       color_map, pad, out_h, out_w, out);
  } else {
    if (N > 65535) return SPML_ERR_UNSUPPORTED;                 // (the image is gridDim.z)
    const dim3 g((unsigned)((w + 31) / 32), (unsigned)((h + 7) / 8), (unsigned)N);
    hipLaunchKernelGGL(summary_panels<false>, g, dim3(256), 0, s, semantic, instance, N, Hl, Wl, proj, minmax, h, w,
                       color_map, pad, out_h, out_w, out);
  }
  return launch_status();
}
