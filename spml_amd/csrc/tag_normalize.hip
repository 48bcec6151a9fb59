// N11: the tag-specific tail of the kNN pseudo labels -- pyscripts/inference/pseudo_inference_crf_msc.py
// :252-263 and the arg-max of :275.  The reference takes the mean of the stacked vote maps over the views (:254), the
// maximum of every class over the whole image (:259), floors it at 0.15 (:260), replaces it by 1 for the classes the
// image does not carry (:262), divides the map by it (:263) and, after the CRF, takes the arg-max over the classes (:275):
// seven passes over an [ncls][h * w] tensor as framework ops.  Here it is two launches on the caller's stream:
//
//   class_peak_parts    acc [ncls][n] (read once) -> parts [ncls][B]: the maximum of every class over one of B chunks
//                       of its plane.  grid (B, ncls), B = parts_per_class(n) <= 16.
//   normalize_argmax    prologue: every workgroup finishes the B parts of every class (<= 4 KiB out of L2) into
//                       div[c] = tags[c] ? max(peak[c] / V, floor) : 1 in LDS; then a thread owns one pixel, consecutive
//                       lanes own consecutive pixels (the layout of view_votes, knn_msc.hip): every class plane is read
//                       coalesced, acc / V / div[c] is formed with two IEEE divisions, written to prob when asked, and
//                       the first class that attains the maximum is the label.
//
// The kernel boundary between the two is the only ordering between workgroups: no grid-wide wait (the per-XCD L2s are
// not coherent inside a launch), no atomics, no host read.  Every part is written by the first launch before the second
// reads it, so the content of the workspace before the call does not matter, and max is exact in any order: results are
// bit-identical from call to call, with or without the deterministic mode.  fp32 division is monotone, so
// max_p(acc[c][p] / V) = (max_p acc[c][p]) / V and the first launch reads acc as it is.  The maximum makes no assumption
// on the sign of acc (fmaxf from -inf).  The divisions are the compiler's correctly rounded fp32 `/` (no fast-math
// flag in spml_amd/_build.py): the same bits as numpy's and ATen's CPU division.
#include <math.h>

#include "common.hpp"

namespace spml {
namespace {

constexpr int kMaxClasses = 64;
constexpr int kBlock = 256;
constexpr int kMaxParts = 16;                     // 64 classes x 16 parts = 1024 floats: four per thread of the prologue
constexpr int64_t kPartPixels = 2048;             // below that a plane is not split further
constexpr int64_t kMaxPixels = (int64_t)1 << 30;  // as view_votes (a pixel index fits an int; offsets are size_t)

inline int parts_per_class(int64_t n) {
  const int64_t b = (n + kPartPixels - 1) / kPartPixels;
  return b < 1 ? 1 : b > kMaxParts ? kMaxParts : (int)b;
}

// the pixels of one part: a multiple of the block size with parts * chunk >= n.  The rounding can leave the last parts
// without a pixel, so the launch uses ceil(n / chunk) <= parts of them and the rows of `parts` are that long.
inline int64_t chunk_pixels(int64_t n, int parts) {
  return ((n + parts - 1) / parts + kBlock - 1) / kBlock * kBlock;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// block (b, c): the maximum of acc[c][b * chunk .. min((b + 1) * chunk, n)).  A plane starts at any 4-byte address
// (n may be odd), so up to three head elements are read alone, the aligned middle as float4s, up to three tail elements
// alone.  b * chunk < n for every b < gridDim.x = ceil(n / chunk).
__global__ __launch_bounds__(kBlock) void class_peak_parts(const float* __restrict__ acc, int64_t n, int64_t chunk,
                                                           float* __restrict__ parts) {
  __shared__ float wave_part[kBlock / kWave];
  const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int64_t lo = (int64_t)b * chunk;
  const int64_t len = (lo + chunk < n ? lo + chunk : n) - lo;
  const float* p = acc + (size_t)c * (size_t)n + (size_t)lo;
  int64_t head = (int64_t)(((0 - reinterpret_cast<uintptr_t>(p)) >> 2) & 3);
  if (head > len) head = len;
  float m = -INFINITY;
  if (tid < head) m = p[tid];
  const float4v* q = reinterpret_cast<const float4v*>(p + head);
  const int64_t nv = (len - head) >> 2;
#pragma unroll 4
  for (int64_t j = tid; j < nv; j += kBlock) {
    const float4v v = q[j];
    m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  const int64_t done = head + 4 * nv;
  if (done + tid < len) m = fmaxf(m, p[done + tid]);
  m = wave_max(m);
  if ((tid & (kWave - 1)) == 0) wave_part[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    float t = wave_part[0];
#pragma unroll
    for (int i = 1; i < kBlock / kWave; ++i) t = fmaxf(t, wave_part[i]);
    parts[(size_t)c * gridDim.x + b] = t;
  }
}

// thread = pixel i of [ncls][n].  Prologue: thread t finishes class t / 4 from the parts t % 4, t % 4 + 4, ... (at most
// four independent loads), two shuffles join the four threads of a class.  The classes are walked eight at a time: the
// eight loads of a pixel are issued before the first division needs one.
template <bool kProb>
__global__ __launch_bounds__(kBlock) void normalize_argmax(const float* __restrict__ acc, int ncls, int64_t n,
                                                           float views, const unsigned char* __restrict__ tags,
                                                           float floor_value, const float* __restrict__ parts,
                                                           int nparts, int64_t* __restrict__ labels,
                                                           float* __restrict__ prob, float* __restrict__ divisor) {
  __shared__ float div[kMaxClasses];
  {
    const int c = threadIdx.x >> 2, q = threadIdx.x & 3;
    float m = -INFINITY;
    if (c < ncls) {
#pragma unroll
      for (int j = 0; j < kMaxParts / 4; ++j) {
        const int part = q + 4 * j;
        if (part < nparts) m = fmaxf(m, parts[c * nparts + part]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 1, kWave));
    m = fmaxf(m, __shfl_xor(m, 2, kWave));
    if (c < ncls && q == 0) {
      const float d = tags[c] ? fmaxf(m / views, floor_value) : 1.0f;
      div[c] = d;
      if (divisor != nullptr && blockIdx.x == 0) divisor[c] = d;
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float* src = acc + i;
  float best = 0.f;
  int best_c = 0;
  for (int c0 = 0; c0 < ncls; c0 += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c0 + j < ncls ? src[(size_t)(c0 + j) * (size_t)n] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c0 + j < ncls) {                                    // (block-uniform)
        const float p = (v[j] / views) / div[c0 + j];
        if (kProb) prob[(size_t)(c0 + j) * (size_t)n + (size_t)i] = p;
        if (c0 + j == 0 || p > best) {                        // strict: the lowest class that attains the maximum
          best = p;
          best_c = c0 + j;
        }
      }
    }
  }
  labels[i] = (int64_t)best_c;
}

inline bool overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return pn != 0 && qn != 0 && p0 < q0 + qn && q0 < p0 + pn;
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_tag_normalize_workspace_bytes(int ncls, int64_t n) {
  if (ncls <= 0 || ncls > kMaxClasses || n <= 0 || n > kMaxPixels) return 0;
  return (size_t)ncls * parts_per_class(n) * sizeof(float);
}

extern "C" int spml_tag_normalize_argmax_f32(const float* acc, int ncls, int64_t n, int num_views,
                                             const unsigned char* tags, float floor, int64_t* labels, float* prob,
                                             float* divisor, void* ws, size_t ws_bytes, void* stream) {
  if (!acc || !tags || !labels || n < 1 || ncls < 1 || num_views < 1 || !(floor > 0.f) || !isfinite(floor) ||
      ((uintptr_t)acc & 3) != 0)
    return SPML_ERR_INVALID_ARG;
  if (ncls > kMaxClasses || n > kMaxPixels) return SPML_ERR_UNSUPPORTED;
  const int nparts = parts_per_class(n);
  const size_t need = (size_t)ncls * nparts * sizeof(float);
  if (!ws || ws_bytes < need || ((uintptr_t)ws & 3) != 0) return SPML_ERR_WORKSPACE;
  const size_t map_bytes = (size_t)ncls * (size_t)n * sizeof(float);
  // what is written (ws, labels, prob, divisor) may alias neither an input nor each other
  const void* written[4] = {ws, labels, prob, divisor};
  const size_t written_bytes[4] = {need, (size_t)n * sizeof(int64_t), prob ? map_bytes : 0,
                                   divisor ? (size_t)ncls * sizeof(float) : 0};
  for (int i = 0; i < 4; ++i) {
    if (overlap(written[i], written_bytes[i], acc, map_bytes) || overlap(written[i], written_bytes[i], tags, (size_t)ncls))
      return SPML_ERR_INVALID_ARG;
    for (int j = i + 1; j < 4; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return SPML_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  float* parts = static_cast<float*>(ws);
  const int64_t chunk = chunk_pixels(n, nparts);
  const int used = (int)((n + chunk - 1) / chunk);            // <= nparts: the parts that hold a pixel
  hipLaunchKernelGGL(class_peak_parts, dim3((unsigned)used, (unsigned)ncls), dim3(kBlock), 0, s, acc, n, chunk, parts);
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  if (prob)
    hipLaunchKernelGGL(normalize_argmax<true>, grid, block, 0, s, acc, ncls, n, (float)num_views, tags, floor, parts, used,
                       labels, prob, divisor);
  else
    hipLaunchKernelGGL(normalize_argmax<false>, grid, block, 0, s, acc, ncls, n, (float)num_views, tags, floor, parts,
                       used, labels, prob, divisor);
  return launch_status();
}
