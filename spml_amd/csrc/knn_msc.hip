// N9: multi-scale + flip kNN inference -- the per-view tail of pyscripts/inference/inference_msc.py:223-234
// and the sum of :237-239 (without the final division).  Per view the reference gathers the retrieved labels of every
// pixel (`topk[clu]`, [rh * rw, k] int64), one-hots them to [rh * rw, k, ncls], means over k (:223-226), copies the
// result to the host, `cv2.resize`s it to the image (:230-231), un-flips (:232-233) and stacks the views for a mean
// (:237-239).  All of that is a function of a [m][ncls] table (m segments, at most 144 with the largest k-means grid
// here) and of one segment id per pixel:
//
//   votes_table      topk [m][k] -> votes [m][NC], votes[s][c] = #{ j < k : topk[s][j] == c } / k
//   view_votes<NC>   clu [rh][rw] (read once) -> acc [ncls][h][w] += bilinear(votes[clu[.]][c])
//
// view_votes follows view_probs<NC> of msc_inference.hip: a thread owns one output pixel, consecutive lanes own
// consecutive x, so the read-modify-write of acc is perfectly coalesced and the four tap ids are near-coalesced 8-byte
// runs (reversed for a flipped view).  NC = the class count padded to 8, 16, 24, 32 or 64: a table row is NC floats
// (the columns from ncls on are zero), 32-byte aligned, and is read as float4s -- four classes per load, every loop
// unrolls.  The table is read straight through the cache: the lanes of a wave hold one or two distinct ids nearly
// everywhere (segments are thousands of pixels), so a tap's load touches one or two lines, and a 144 x 24 table is 13.5
// KiB.  The alternative -- every workgroup stages the table in LDS first (row stride NC + 4) -- costs each 256-thread
// workgroup a copy of the whole table (3.4 float4 loads + stores per thread at 144 x 24, against 12 table loads per
// thread of real work) and is compiled with -DSPML_VIEW_VOTES_LDS=1 for the A/B of tools/bench_knn_msc.py only; the
// two have NOT been timed against each other yet (profiles/knn_msc.md).
// No atomics: two calls on equal inputs are bit-identical, with or without the deterministic mode.
//
// Bilinear taps: bilinear.hpp (ATen's rule) with in = rh / rw;
// value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
#include "bilinear.hpp"
#include "common.hpp"

#ifndef SPML_VIEW_VOTES_LDS
#define SPML_VIEW_VOTES_LDS 0
#endif

namespace spml {
namespace {

constexpr int kMaxClasses = 64;
#if SPML_VIEW_VOTES_LDS
constexpr int kRowPad = 4;             // LDS row stride NC + 4 floats: rows stay 16-byte aligned, and the rows s and s + 1
                                       // start 4 * (NC + 4) bytes apart -- never a multiple of the 256-byte bank row
constexpr int kMaxSegments = 240;      // 240 * (64 + 4) * 4 B = 65 280 B of the 64 KiB a workgroup gets without opting in
#else
constexpr int kMaxSegments = 4096;     // a 1-MiB table at 64 classes: resident in L2, and ids * NC stay far inside an int
#endif

__host__ __device__ constexpr int padded_classes(int ncls) {
  return ncls <= 8 ? 8 : ncls <= 16 ? 16 : ncls <= 24 ? 24 : ncls <= 32 ? 32 : 64;
}

// block = segment s, thread = class c < nc: the count is an exact small integer, divided once by (float)k -- what
// one_hot(...).float().mean(1) gives (a sum of k zeros and ones, then one division).  A label outside [0, ncls)
// matches no column; the columns from ncls on are written as zeros.
__global__ __launch_bounds__(64) void votes_table(const int64_t* __restrict__ topk, int k, int ncls, int nc,
                                                  float* __restrict__ votes) {
  const int s = blockIdx.x, c = threadIdx.x;
  if (c >= nc) return;
  const int64_t* row = topk + (size_t)s * k;
  int count = 0;
  for (int j = 0; j < k; ++j) count += row[j] == (int64_t)c;
  votes[(size_t)s * nc + c] = c < ncls ? (float)count / (float)k : 0.f;
}

__device__ __forceinline__ int segment_of(int64_t id, int m) {
  return id < 0 ? 0 : id >= (int64_t)m ? m - 1 : (int)id;
}

// thread = output pixel i = y * w + x of acc [ncls][h * w].  The mapping is evaluated at xd = flip ? w - 1 - x : x and
// the result stored at x: the reference resizes the still-flipped view and flips the result (:230-233).
// An id outside [0, m) is outside the contract; it is clamped, so that nothing is read out of bounds.
template <int NC>
__global__ __launch_bounds__(256) void view_votes(const int64_t* __restrict__ clu, int rh, int rw,
                                                  const float* __restrict__ votes, int m, int ncls, int flip, int h,
                                                  int w, float scale_h, float scale_w, float* __restrict__ acc) {
#if SPML_VIEW_VOTES_LDS
  constexpr int kStride = NC + kRowPad;
  extern __shared__ float4v table4[];
  float* table = reinterpret_cast<float*>(table4);
  for (int e = threadIdx.x; e < m * (NC / 4); e += 256) {
    const int s = e / (NC / 4), q = e - s * (NC / 4);
    *reinterpret_cast<float4v*>(table + s * kStride + 4 * q) = reinterpret_cast<const float4v*>(votes)[e];
  }
  __syncthreads();
#else
  constexpr int kStride = NC;
  const float* table = votes;
#endif
  const int n = h * w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int y = i / w, x = i - y * w;
  const Tap ty = make_tap(y, scale_h, rh), tx = make_tap(flip ? w - 1 - x : x, scale_w, rw);
  const int s00 = segment_of(clu[ty.i0 * rw + tx.i0], m), s01 = segment_of(clu[ty.i0 * rw + tx.i1], m);
  const int s10 = segment_of(clu[ty.i1 * rw + tx.i0], m), s11 = segment_of(clu[ty.i1 * rw + tx.i1], m);
  const float4v* r00 = reinterpret_cast<const float4v*>(table + s00 * kStride);
  const float4v* r01 = reinterpret_cast<const float4v*>(table + s01 * kStride);
  const float4v* r10 = reinterpret_cast<const float4v*>(table + s10 * kStride);
  const float4v* r11 = reinterpret_cast<const float4v*>(table + s11 * kStride);
  float* dst = acc + i;
#pragma unroll
  for (int c0 = 0; c0 < NC; c0 += 8) {
    if (c0 >= ncls) break;                                  // (block-uniform)
    float4v a[2], b[2], c[2], d[2];
    float old[8];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      a[q] = r00[c0 / 4 + q]; b[q] = r01[c0 / 4 + q]; c[q] = r10[c0 / 4 + q]; d[q] = r11[c0 / 4 + q];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) old[j] = c0 + j < ncls ? dst[(size_t)(c0 + j) * n] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = ty.l0 * (tx.l0 * a[j / 4][j % 4] + tx.l1 * b[j / 4][j % 4]) +
                      ty.l1 * (tx.l0 * c[j / 4][j % 4] + tx.l1 * d[j / 4][j % 4]);
      if (c0 + j < ncls) dst[(size_t)(c0 + j) * n] = old[j] + v;
    }
  }
}

inline bool overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 < q0 + qn && q0 < p0 + pn;
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_view_votes_workspace_bytes(int m, int ncls) {
  if (m <= 0 || ncls <= 0 || ncls > kMaxClasses || m > kMaxSegments) return 0;
  return (size_t)m * padded_classes(ncls) * sizeof(float);
}

extern "C" int spml_view_votes_accumulate_f32(const int64_t* clu, int rh, int rw, const int64_t* topk, int m, int k,
                                              int ncls, int flip, int h, int w, float* acc, void* ws, size_t ws_bytes,
                                              void* stream) {
  if (!clu || !topk || !acc || rh <= 0 || rw <= 0 || m <= 0 || k <= 0 || ncls <= 0 || h <= 0 || w <= 0)
    return SPML_ERR_INVALID_ARG;
  if (ncls > kMaxClasses || m > kMaxSegments || (int64_t)rh * rw > (1 << 30) || (int64_t)h * w > (1 << 30))
    return SPML_ERR_UNSUPPORTED;
  const int nc = padded_classes(ncls);
  const size_t need = (size_t)m * nc * sizeof(float);
  if (!ws || ws_bytes < need) return SPML_ERR_WORKSPACE;
  if (((uintptr_t)ws & 15) != 0) return SPML_ERR_INVALID_ARG;         // the rows are read as float4s
  const int n = h * w;
  const size_t clu_bytes = (size_t)rh * rw * sizeof(int64_t), topk_bytes = (size_t)m * k * sizeof(int64_t);
  const size_t acc_bytes = (size_t)ncls * n * sizeof(float);
  // acc may alias none of the inputs, nor may the workspace (both are written)
  if (overlap(acc, acc_bytes, clu, clu_bytes) || overlap(acc, acc_bytes, topk, topk_bytes) ||
      overlap(acc, acc_bytes, ws, need) || overlap(ws, need, clu, clu_bytes) || overlap(ws, need, topk, topk_bytes))
    return SPML_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* votes = static_cast<float*>(ws);
  hipLaunchKernelGGL(votes_table, dim3((unsigned)m), dim3(64), 0, s, topk, k, ncls, nc, votes);
  const float sh = (float)rh / (float)h, sw = (float)rw / (float)w;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#if SPML_VIEW_VOTES_LDS
  const size_t lds = (size_t)m * (nc + kRowPad) * sizeof(float);
#else
  const size_t lds = 0;
#endif
#define SPML_VIEW(NC) \
  hipLaunchKernelGGL(view_votes<NC>, grid, block, lds, s, clu, rh, rw, votes, m, ncls, flip, h, w, sh, sw, acc)
  if (nc == 8) SPML_VIEW(8);
  else if (nc == 16) SPML_VIEW(16);
  else if (nc == 24) SPML_VIEW(24);
  else if (nc == 32) SPML_VIEW(32);
  else SPML_VIEW(64);
#undef SPML_VIEW
  return launch_status();
}
