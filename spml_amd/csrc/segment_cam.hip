// N13: the class maps of the DensePose pseudo-label program from propagated segment tags --
// pyscripts/inference/pseudo_denseposerw_crf.py:159-182.  The reference one-hots the label of every pixel's nearest
// labelled prototype to [N, ncls + 1] int64, scatter-adds it by the segment id twice (segment_mean), divides every row by
// its sum, gathers the rows back per pixel, transposes and resamples to 1/8 of the image: about a dozen passes over
// [N, ncls + 1] tensors.  The information is a [S][ncls] table of small integers and a four-tap gather:
//
//   count_lds / count_global   nn_index, nn_value, cluster_index [N], proto_label [M] -> table [S][ncls] (uint32)
//                              table[s][c] = #{p : cluster_index[p] = s, class(p) = c}
//   segment_probs              table -> probs [S][ncls] = table[s][c] / sum_c table[s][c] (0 for a row without a count)
//   gather_resample            cluster_index [h2][w2], probs -> acc [ncls][oh][ow], bilinear over probs[cluster_index]
//
// class(p) = proto_label[nn_index[p]], or none where nn_value[p] < threshold, nn_index[p] is outside [0, M) or the label
// is outside [0, ncls).  The counting body is segment_count.hpp (shared with segment_majority.hip): integer atomics only,
// so the table, and with it every output, is bit-identical from call to call and the same in both modes of the library.
// The reference's row is segment_mean's (count / pixels of the segment) divided by its sum; the pixel count cancels, and
// count / sum_c count is that quotient rounded once instead of three times.
// gather_resample has the layout of the view kernels of pseudo_label.hip: 16 lanes per output pixel with a class slice
// each (a 46 x 62 map is 716 waves and not 45), the four segment ids are loaded once per pixel, the four table rows are
// gathered before the first use; taps and blend are bilinear.hpp's.  The half-resolution map is never formed.
// No kernel forms an address from an id outside its range: such a pixel counts nowhere, such a tap contributes 0.
#include "bilinear.hpp"
#include "common.hpp"
#include "segment_count.hpp"

namespace spml {
namespace {

using segcount::kBlock;
using segcount::kLdsEntries;
using segcount::overlap;

constexpr int kMaxSegments = 4096;
constexpr int kMaxClasses = 64;
constexpr int kSlices = 16;            // lanes per output pixel in gather_resample
constexpr int kGatherPix = 16;         // output pixels per 256-thread workgroup there
constexpr int kOwn = kMaxClasses / kSlices;      // classes a lane owns (slice, +16, +32, +48)

// the bin of pixel p, or -1 when the pixel counts nowhere
struct TagBin {
  const int64_t* __restrict__ nn_index;
  const float* __restrict__ nn_value;
  const int64_t* __restrict__ proto_label;
  const int64_t* __restrict__ cluster_index;
  int64_t M;
  float threshold;
  int S, ncls;
  __device__ __forceinline__ int operator()(int64_t p, int64_t end) const {
    if (p >= end) return -1;
    const int64_t s = cluster_index[p], j = nn_index[p];
    if (s < 0 || s >= (int64_t)S || j < 0 || j >= M || nn_value[p] < threshold) return -1;
    const int64_t c = proto_label[j];
    if (c < 0 || c >= (int64_t)ncls) return -1;
    return (int)s * ncls + (int)c;            // < 4096 * 64
  }
};

__global__ __launch_bounds__(kBlock) void count_lds(TagBin bin, int64_t N, int64_t chunk,
                                                    unsigned* __restrict__ table) {
  __shared__ unsigned local[kLdsEntries];
  segcount::count_lds(bin, N, chunk, bin.S * bin.ncls, local, table);
}

__global__ __launch_bounds__(kBlock) void count_global(TagBin bin, int64_t N, int64_t chunk,
                                                       unsigned* __restrict__ table) {
  segcount::count_global(bin, N, chunk, table);
}

// wave = segment s, lane = class (ncls <= 64): the row's sum is an exact integer, every quotient one fp32 division
__global__ __launch_bounds__(kBlock) void segment_probs(const unsigned* __restrict__ table, int S, int ncls,
                                                        float* __restrict__ probs, int* __restrict__ counts_out,
                                                        float* __restrict__ probs_out) {
  const int s = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (s >= S) return;                                        // (wave-uniform)
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned v = lane < ncls ? table[(size_t)s * ncls + lane] : 0u;
  unsigned total = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, kWave);
  if (lane >= ncls) return;
  const float q = total != 0u ? (float)v / (float)total : 0.f;
  probs[(size_t)s * ncls + lane] = q;
  if (counts_out) counts_out[(size_t)s * ncls + lane] = (int)v;
  if (probs_out) probs_out[(size_t)s * ncls + lane] = q;
}

__global__ __launch_bounds__(256) void gather_resample(const int64_t* __restrict__ cluster_index,
                                                       const float* __restrict__ probs, int S, int ncls, int h2, int w2,
                                                       int oh, int ow, float scale_h, float scale_w,
                                                       float* __restrict__ acc) {
  const int slice = threadIdx.x & (kSlices - 1);
  const int n = oh * ow;
  const int p = blockIdx.x * kGatherPix + (threadIdx.x >> 4);
  const bool live = p < n;
  const Taps4 t = make_taps(live ? p : 0, ow, scale_h, scale_w, h2, w2, 0, w2, 1);
  // (the 16 lanes of a pixel load the same four words: one request each)
  const int64_t s00 = cluster_index[t.o00], s01 = cluster_index[t.o01], s10 = cluster_index[t.o10],
                s11 = cluster_index[t.o11];
  const bool k00 = s00 >= 0 && s00 < (int64_t)S, k01 = s01 >= 0 && s01 < (int64_t)S, k10 = s10 >= 0 && s10 < (int64_t)S,
             k11 = s11 >= 0 && s11 < (int64_t)S;
  const float* r00 = probs + (k00 ? (size_t)s00 * ncls : 0);
  const float* r01 = probs + (k01 ? (size_t)s01 * ncls : 0);
  const float* r10 = probs + (k10 ? (size_t)s10 * ncls : 0);
  const float* r11 = probs + (k11 ? (size_t)s11 * ncls : 0);
  float a[kOwn], b[kOwn], c[kOwn], d[kOwn];
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int ch = kSlices * j + slice;
    const bool ok = live && ch < ncls;
    a[j] = ok && k00 ? r00[ch] : 0.f;
    b[j] = ok && k01 ? r01[ch] : 0.f;
    c[j] = ok && k10 ? r10[ch] : 0.f;
    d[j] = ok && k11 ? r11[ch] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int ch = kSlices * j + slice;
    if (live && ch < ncls) acc[(size_t)ch * n + p] = blend(t, a[j], b[j], c[j], d[j]);
  }
}

inline bool supported(int64_t N, int S, int ncls) {
  return S <= kMaxSegments && ncls <= kMaxClasses && N < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace spml

using namespace spml;

// [table: S * ncls uint32][probs: S * ncls fp32]
extern "C" size_t spml_segment_tag_cam_workspace_bytes(int S, int ncls) {
  if (S <= 0 || ncls <= 0 || S > kMaxSegments || ncls > kMaxClasses) return 0;
  return (size_t)S * ncls * (sizeof(unsigned) + sizeof(float));
}

extern "C" const char* spml_segment_tag_cam_path_name(int64_t N, int S, int ncls) {
  if (N < 1 || S <= 0 || ncls <= 0) return "invalid";
  if (!supported(N, S, ncls)) return "unsupported";
  return S * ncls <= kLdsEntries ? "lds_table" : "global_table";
}

extern "C" int spml_segment_tag_cam_f32(const int64_t* nn_index, const float* nn_value, const int64_t* proto_label,
                                        int64_t M, float threshold, const int64_t* cluster_index, int S, int ncls,
                                        int h2, int w2, int oh, int ow, float* acc, int* counts, float* probs, void* ws,
                                        size_t ws_bytes, void* stream) {
  if (!nn_index || !nn_value || !proto_label || !cluster_index || !acc || M < 1 || S <= 0 || ncls <= 0 || h2 < 1 ||
      w2 < 1 || oh < 1 || ow < 1 || threshold != threshold)
    return SPML_ERR_INVALID_ARG;
  const int64_t N = (int64_t)h2 * w2;
  if (!supported(N, S, ncls) || (int64_t)oh * ow > (1 << 24)) return SPML_ERR_UNSUPPORTED;
  const int entries = S * ncls;
  const size_t need = spml_segment_tag_cam_workspace_bytes(S, ncls);
  if (!ws || ws_bytes < need) return SPML_ERR_WORKSPACE;
  if (((uintptr_t)ws & 3) != 0) return SPML_ERR_INVALID_ARG;
  // what is written (ws, acc, counts, probs) may alias neither an input nor each other
  const size_t map_bytes = (size_t)N * sizeof(int64_t);
  const void* read[4] = {nn_index, nn_value, proto_label, cluster_index};
  const size_t read_bytes[4] = {map_bytes, (size_t)N * sizeof(float), (size_t)M * sizeof(int64_t), map_bytes};
  const void* written[4] = {ws, acc, counts, probs};
  const size_t written_bytes[4] = {need, (size_t)ncls * oh * ow * sizeof(float),
                                   counts ? (size_t)entries * sizeof(int) : 0,
                                   probs ? (size_t)entries * sizeof(float) : 0};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j)
      if (overlap(written[i], written_bytes[i], read[j], read_bytes[j])) return SPML_ERR_INVALID_ARG;
    for (int j = i + 1; j < 4; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return SPML_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned* table = static_cast<unsigned*>(ws);
  float* table_probs = reinterpret_cast<float*>(table + entries);
  if (hipMemsetAsync(table, 0, (size_t)entries * sizeof(unsigned), s) != hipSuccess) return SPML_ERR_LAUNCH;
  const TagBin bin{nn_index, nn_value, proto_label, cluster_index, M, threshold, S, ncls};
  const segcount::Chunks g = segcount::plan_chunks(N);
  if (entries <= kLdsEntries)
    hipLaunchKernelGGL(count_lds, dim3((unsigned)g.blocks), dim3(kBlock), 0, s, bin, N, g.chunk, table);
  else
    hipLaunchKernelGGL(count_global, dim3((unsigned)g.blocks), dim3(kBlock), 0, s, bin, N, g.chunk, table);
  const int rows_per_block = kBlock / kWave;
  hipLaunchKernelGGL(segment_probs, dim3((unsigned)((S + rows_per_block - 1) / rows_per_block)), dim3(kBlock), 0, s,
                     table, S, ncls, table_probs, counts, probs);
  const int n = oh * ow;
  hipLaunchKernelGGL(gather_resample, dim3((unsigned)((n + kGatherPix - 1) / kGatherPix)), dim3(256), 0, s,
                     cluster_index, table_probs, S, ncls, h2, w2, oh, ow, (float)h2 / (float)oh, (float)w2 / (float)ow,
                     acc);
  return launch_status();
}
