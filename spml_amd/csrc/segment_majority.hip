// N10: the majority label per segment -- the tail of the memory-bank pass,
// spml/utils/segsort/common.py:221-267 as pyscripts/inference/prototype.py:200-203 and prototype_msc.py:189-192 use it
// (the labels; the list of agreeing pixels that function also returns is thrown away there).  The reference one-hots
// the label map to [P, ncls] int64 and scatter-adds it by the segment id; the information is a [m][ncls] table of small
// integers made from two int64 maps read once (16 bytes per pixel):
//
//   count_lds / count_global   clu [P], sem [P] -> table [m][ncls] (uint32)   table[s][c] = #{p : clu[p] = s, sem[p] = c}
//   row_argmax                 table -> major [m] (int64), and hist [m][ncls] (int64) when asked for
//
// The counting body (a contiguous run of pixels per workgroup, an LDS table where m * ncls fits 8192 entries and the
// global one where it does not -- m = 144 segments x 256 classes = 147 KiB: the case of a label map that holds the ignore
// value 255 --, equal keys merged inside a wave before the atomic) is segment_count.hpp, shared with segment_cam.hip.
// Only integer atomics: integer adds commute, so the result does not depend on the arrival order -- two calls are
// bit-identical, with or without the deterministic mode.  Counters are 32 bits wide: P < 2^31 bounds every bin.
// A pixel whose id is outside [0, m) or whose label is outside [0, ncls) counts nowhere and forms no address.
// SPML_MAJORITY_WAVE_COMBINE=0 compiles the plain form (one atomic per counted pixel); tools/bench_prototype_msc.py times
// the two: on the global table the merged form takes 0.46 - 0.83 x the plain form's time, on the LDS table 0.88 - 1.02 x
// (profiles/prototype_msc.md).
#include "common.hpp"
#include "segment_count.hpp"

namespace spml {
namespace {

using segcount::kBlock;
using segcount::kLdsEntries;
using segcount::overlap;

constexpr int kMaxSegments = 4096;
constexpr int kMaxClasses = 256;

// the bin of pixel p, or -1 when the pixel counts nowhere
struct LabelBin {
  const int64_t* __restrict__ clu;
  const int64_t* __restrict__ sem;
  int m, ncls;
  __device__ __forceinline__ int operator()(int64_t p, int64_t end) const {
    if (p >= end) return -1;
    const int64_t s = clu[p], c = sem[p];
    if (s < 0 || s >= (int64_t)m || c < 0 || c >= (int64_t)ncls) return -1;
    return (int)s * ncls + (int)c;            // < 4096 * 256
  }
};

__global__ __launch_bounds__(kBlock) void count_lds(const int64_t* __restrict__ clu, const int64_t* __restrict__ sem,
                                                    int64_t P, int64_t chunk, int m, int ncls,
                                                    unsigned* __restrict__ table) {
  __shared__ unsigned local[kLdsEntries];
  segcount::count_lds(LabelBin{clu, sem, m, ncls}, P, chunk, m * ncls, local, table);
}

__global__ __launch_bounds__(kBlock) void count_global(const int64_t* __restrict__ clu,
                                                       const int64_t* __restrict__ sem, int64_t P, int64_t chunk,
                                                       int m, int ncls, unsigned* __restrict__ table) {
  segcount::count_global(LabelBin{clu, sem, m, ncls}, P, chunk, table);
}

// wave = segment s: the lanes stride over the classes, each keeps its best (count, class) -- a later class replaces an
// earlier one only with a LARGER count --, then the wave keeps the larger count and, between equal counts, the lower
// class: the first maximum, torch.argmax's rule on the CPU.  An all-zero row gives class 0.
__global__ __launch_bounds__(kBlock) void row_argmax(const unsigned* __restrict__ table, int m, int ncls,
                                                     int64_t* __restrict__ major, int64_t* __restrict__ hist) {
  const int s = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (s >= m) return;                                        // (wave-uniform)
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned* row = table + (size_t)s * ncls;
  unsigned best = 0u;
  int best_c = kMaxClasses;                                  // "no class yet": loses every tie
  for (int c = lane; c < ncls; c += kWave) {
    const unsigned v = row[c];
    if (hist) hist[(size_t)s * ncls + c] = (int64_t)v;
    if (best_c == kMaxClasses || v > best) { best = v; best_c = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned v = __shfl_xor(best, o, kWave);
    const int c = __shfl_xor(best_c, o, kWave);
    if (v > best || (v == best && c < best_c)) { best = v; best_c = c; }
  }
  if (lane == 0) major[s] = (int64_t)best_c;
}

inline bool supported(int64_t P, int m, int ncls) {
  return m <= kMaxSegments && ncls <= kMaxClasses && P < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_segment_majority_workspace_bytes(int m, int ncls) {
  if (m <= 0 || ncls <= 0 || m > kMaxSegments || ncls > kMaxClasses) return 0;
  return (size_t)m * ncls * sizeof(unsigned);
}

extern "C" const char* spml_segment_majority_path_name(int64_t P, int m, int ncls) {
  if (P < 0 || m <= 0 || ncls <= 0) return "invalid";
  if (!supported(P, m, ncls)) return "unsupported";
#if SPML_MAJORITY_WAVE_COMBINE
  return m * ncls <= kLdsEntries ? "lds_table" : "global_table";
#else
  return m * ncls <= kLdsEntries ? "lds_table_per_pixel_atomics" : "global_table_per_pixel_atomics";
#endif
}

extern "C" int spml_segment_majority_i64(const int64_t* clu, const int64_t* sem, int64_t P, int m, int ncls,
                                         int64_t* major, int64_t* hist, void* ws, size_t ws_bytes, void* stream) {
  if (P < 0 || m <= 0 || ncls <= 0 || !major || (P > 0 && (!clu || !sem))) return SPML_ERR_INVALID_ARG;
  if (!supported(P, m, ncls)) return SPML_ERR_UNSUPPORTED;
  const int entries = m * ncls;
  const size_t need = (size_t)entries * sizeof(unsigned);
  if (!ws || ws_bytes < need) return SPML_ERR_WORKSPACE;
  if (((uintptr_t)ws & 3) != 0) return SPML_ERR_INVALID_ARG;
  const size_t map_bytes = (size_t)P * sizeof(int64_t), major_bytes = (size_t)m * sizeof(int64_t);
  const size_t hist_bytes = hist ? (size_t)entries * sizeof(int64_t) : 0;
  // what is written (ws, major, hist) may alias neither an input nor each other
  const void* written[3] = {ws, major, hist};
  const size_t written_bytes[3] = {need, major_bytes, hist_bytes};
  for (int i = 0; i < 3; ++i) {
    if (overlap(written[i], written_bytes[i], clu, map_bytes) || overlap(written[i], written_bytes[i], sem, map_bytes))
      return SPML_ERR_INVALID_ARG;
    for (int j = i + 1; j < 3; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return SPML_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned* table = static_cast<unsigned*>(ws);
  if (hipMemsetAsync(table, 0, need, s) != hipSuccess) return SPML_ERR_LAUNCH;
  if (P > 0) {
    const segcount::Chunks g = segcount::plan_chunks(P);
    if (entries <= kLdsEntries)
      hipLaunchKernelGGL(count_lds, dim3((unsigned)g.blocks), dim3(kBlock), 0, s, clu, sem, P, g.chunk, m, ncls, table);
    else
      hipLaunchKernelGGL(count_global, dim3((unsigned)g.blocks), dim3(kBlock), 0, s, clu, sem, P, g.chunk, m, ncls,
                         table);
  }
  const int rows_per_block = kBlock / kWave;
  hipLaunchKernelGGL(row_argmax, dim3((unsigned)((m + rows_per_block - 1) / rows_per_block)), dim3(kBlock), 0, s, table,
                     m, ncls, major, hist);
  return launch_status();
}
