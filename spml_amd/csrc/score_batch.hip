// N16: scoring label files against ground truth -- the per-file arithmetic of the reference's
// pyscripts/benchmark/benchmark_by_mIoU.py:25-53 (iou_stats) and benchmark_by_instance.py:97-108 (instances per class),
// numpy on the host there, for a whole batch of decoded files in two launches:
//
//   count_lds / count_global   packed uint8 planes (pred, gt, inst) of B files -> per file two tables of uint32
//                                pair [ncls][ncls+2]   pair[g][q] = #{i : gt = g < ncls, bin(pred) = q}
//                                inst [256][ncls+1]    inst[s][c] = #{i : id = s, gt = c < ncls, or c = ncls: "outside"}
//   finish                     tables -> stats int64 [B][4][ncls] = TP+FN, TP+FP, TP, instances per class
//
// bin(p) = min(p, ncls + 1): the column ncls holds the predictions of exactly ncls, which np.histogram counts for the
// LAST class of TP+FP (it closes its last bin on the right) though they are no true positive of it (`pred == target`),
// the column ncls + 1, "no bin", anything larger.  TP+FN is the row sum of `pair`, TP+FP the column sum (the last class
// takes the column ncls as well), TP the diagonal: one add per counted pixel.  An id occurs when its row of `inst` is
// not all zero (the column "outside" is what makes an id of uncounted pixels occur); its class is the first maximum over
// the row's first ncls columns (class 0 for an all-zero histogram, the arg-max of numpy); when all 256 ids occur, id 255
// counts nowhere (`if i < 255` over the sorted unique ids).
//
// Each workgroup owns one run of kRun contiguous pixels of ONE file; the grid is the sum of the files' runs, and a
// workgroup finds its file by a prefix sum over the records' run counts (B <= 256 = one record per thread), so a batch of
// mixed sizes leaves no workgroup idle.  A thread loads 16 pixels of every plane as one 16-byte vector: plane offsets
// are multiples of 16 and planes are padded to 16 bytes inside `packed`; the padding is loaded, never counted.  The
// counting is segment_count.hpp's: tables in LDS where both fit its 8192 entries (ncls * (ncls + 2) + 256 * (ncls + 1):
// up to 27 classes), flushed once per workgroup (non-zero bins only) into the file's global tables; the global tables
// directly beyond that; equal keys merged inside a wave before the atomic.  Only integer atomics: integer adds commute,
// so two calls are bit-identical, with or without the deterministic mode.  Counters are 32 bits wide: n < 2^31 bounds
// every bin.
#include "common.hpp"
#include "segment_count.hpp"

#include <algorithm>

namespace spml {
namespace {

using segcount::kBlock;
using segcount::kLdsEntries;
using segcount::overlap;

constexpr int kMaxFiles = 256;                       // one record per thread of a workgroup
constexpr int kMaxClasses = 64;
constexpr int kIds = 256;                            // instance masks are 8-bit
constexpr int kVec = 16;                             // pixels of one 16-byte load
constexpr int kVecsPerThread = 2;
constexpr int kRun = kBlock * kVec * kVecsPerThread; // 8192 pixels per workgroup
constexpr int64_t kMaxPixels = (int64_t)1 << 31;     // exclusive

static_assert(kMaxFiles == kBlock, "the prefix over the records is one record per thread");

__host__ __device__ inline int pair_entries(int ncls) { return ncls * (ncls + 2); }
__host__ __device__ inline int file_entries(int ncls) { return pair_entries(ncls) + kIds * (ncls + 1); }
__host__ __device__ inline int64_t padded(int64_t n) { return (n + (kVec - 1)) / kVec * kVec; }

__host__ __device__ inline bool plane_ok(int64_t off, int64_t n, int64_t packed_bytes) {
  return off >= 0 && (off & (kVec - 1)) == 0 && off <= packed_bytes - padded(n);
}

// The one expression that decides whether a record runs -- the host entry (before anything is launched), the kernels
// (a record that fails counts nothing and forms no address) and spml_score_batch_path_name read it.
__host__ __device__ inline bool record_ok(const spml_score_params& p, int64_t packed_bytes) {
  if (p.n < 1 || p.n >= kMaxPixels) return false;
  if (!plane_ok(p.pred_off, p.n, packed_bytes) || !plane_ok(p.gt_off, p.n, packed_bytes)) return false;
  return p.inst_off == -1 || plane_ok(p.inst_off, p.n, packed_bytes);
}

__host__ __device__ inline int runs_of(int64_t n) { return (int)((n + kRun - 1) / kRun); }   // <= 2^18

inline bool limits_ok(int B, int ncls) { return B >= 1 && B <= kMaxFiles && ncls >= 1 && ncls <= kMaxClasses; }

// ... and whether the whole call runs: B, ncls, every record, no two planes overlapping (sorted by offset: neighbours)
inline bool batch_ok(const spml_score_params* p, int B, int64_t packed_bytes, int ncls) {
  if (!p || !limits_ok(B, ncls) || packed_bytes < 0) return false;
  struct Span { int64_t off, bytes; };
  Span spans[3 * kMaxFiles];
  int count = 0;
  for (int b = 0; b < B; ++b) {
    if (!record_ok(p[b], packed_bytes)) return false;
    const int64_t bytes = padded(p[b].n);
    spans[count++] = {p[b].pred_off, bytes};
    spans[count++] = {p[b].gt_off, bytes};
    if (p[b].inst_off >= 0) spans[count++] = {p[b].inst_off, bytes};
  }
  std::sort(spans, spans + count, [](const Span& a, const Span& b) { return a.off < b.off; });
  for (int i = 1; i < count; ++i)
    if (spans[i].off < spans[i - 1].off + spans[i - 1].bytes) return false;
  return true;
}

// The file and the run of this workgroup: thread t holds record t's run count, an inclusive scan over the workgroup
// (Hillis-Steele in LDS), and the one thread whose interval holds blockIdx.x publishes (file, first pixel).  Returns
// false for a workgroup beyond the records' total (the host sized the grid from the same records).
__device__ __forceinline__ bool find_run(const spml_score_params* __restrict__ params, int B, int64_t packed_bytes,
                                         int* scan, int* found, spml_score_params& rec, int& file, int64_t& begin) {
  const int t = threadIdx.x;
  int mine = 0;
  if (t < B) {
    const spml_score_params p = params[t];
    mine = record_ok(p, packed_bytes) ? runs_of(p.n) : 0;
  }
  scan[t] = mine;
  if (t == 0) found[0] = -1;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    const int add = t >= o ? scan[t - o] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const int last = scan[t], first = last - mine;             // (B * 2^18 runs at most: no overflow)
  if ((int)blockIdx.x >= first && (int)blockIdx.x < last) {
    found[0] = t;
    found[1] = (int)blockIdx.x - first;
  }
  __syncthreads();
  file = found[0];
  if (file < 0) return false;
  rec = params[file];
  begin = (int64_t)found[1] * kRun;
  return true;
}

__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) {
  const unsigned word = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
  return (word >> (8 * (j & 3))) & 0xffu;
}

// the run [begin, min(n, begin + kRun)) of one file into `table` (LDS or global: pair table, then the id table)
template <bool kInst>
__device__ __forceinline__ void count_run(const unsigned char* __restrict__ packed, const spml_score_params& rec,
                                          int64_t begin, int ncls, unsigned* table) {
  const int pair_cols = ncls + 2, cols = ncls + 1, id_base = pair_entries(ncls);
#pragma unroll 1
  for (int v = 0; v < kVecsPerThread; ++v) {
    const int64_t at = begin + ((int64_t)v * kBlock + threadIdx.x) * kVec;      // (wave-uniform trip count)
    const bool live = at < rec.n;                            // a vector that starts inside n lies inside the padded plane
    uint4 pv = {0u, 0u, 0u, 0u}, gv = pv, sv = pv;
    if (live) {
      pv = *reinterpret_cast<const uint4*>(packed + rec.pred_off + at);
      gv = *reinterpret_cast<const uint4*>(packed + rec.gt_off + at);
      if (kInst) sv = *reinterpret_cast<const uint4*>(packed + rec.inst_off + at);
    }
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const bool counted = live && at + j < rec.n;           // (the padding bytes are never counted)
      const int g = (int)byte_of(gv, j), p = (int)byte_of(pv, j);
      const bool in_gt = g < ncls;
      const int q = p < ncls + 1 ? p : ncls + 1;
      segcount::add_one(table, counted && in_gt ? g * pair_cols + q : -1);
      if (kInst) segcount::add_one(table, counted ? id_base + (int)byte_of(sv, j) * cols + (in_gt ? g : ncls) : -1);
    }
  }
}

template <bool kLds>
__global__ __launch_bounds__(kBlock) void count(const unsigned char* __restrict__ packed, int64_t packed_bytes,
                                                const spml_score_params* __restrict__ params, int B, int ncls,
                                                unsigned* __restrict__ tables) {
  __shared__ int scan[kBlock];
  __shared__ int found[2];
  __shared__ unsigned local[kLds ? kLdsEntries : 1];
  spml_score_params rec;
  int file;
  int64_t begin;
  if (!find_run(params, B, packed_bytes, scan, found, rec, file, begin)) return;       // (workgroup-uniform)
  const bool inst = rec.inst_off >= 0;
  const int entries = inst ? file_entries(ncls) : pair_entries(ncls);
  unsigned* table = tables + (size_t)file * file_entries(ncls);
  if (kLds) {
    for (int e = threadIdx.x; e < entries; e += kBlock) local[e] = 0u;
    __syncthreads();
    if (inst) count_run<true>(packed, rec, begin, ncls, local);
    else count_run<false>(packed, rec, begin, ncls, local);
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += kBlock) {
      const unsigned v = local[e];
      if (v != 0u) atomicAdd(table + e, v);
    }
  } else {
    if (inst) count_run<true>(packed, rec, begin, ncls, table);
    else count_run<false>(packed, rec, begin, ncls, table);
  }
}

// workgroup = file.  Thread s = instance id s (its row's first maximum, whether it occurs), then thread c = class c
// (row sum, column sum and diagonal of the pair table).  Every element of stats[file] is written.
__global__ __launch_bounds__(kIds) void finish(const spml_score_params* __restrict__ params, int64_t packed_bytes,
                                               int ncls, const unsigned* __restrict__ tables,
                                               int64_t* __restrict__ stats) {
  __shared__ int per_class[kMaxClasses];
  const int file = blockIdx.x, t = threadIdx.x, cols = ncls + 1, pair_cols = ncls + 2;
  const spml_score_params rec = params[file];
  const bool ok = record_ok(rec, packed_bytes), inst = ok && rec.inst_off >= 0;
  const unsigned* pair = tables + (size_t)file * file_entries(ncls);
  if (t < ncls) per_class[t] = 0;
  bool occurs = false;
  int best_c = 0;
  if (inst) {
    const unsigned* row = pair + pair_entries(ncls) + (size_t)t * cols;
    unsigned best = 0u;
    for (int c = 0; c < ncls; ++c) {
      const unsigned v = row[c];
      if (v > best) { best = v; best_c = c; }                // a later class only with a LARGER count: the first maximum
    }
    occurs = best != 0u || row[ncls] != 0u;
  }
  const int present = __syncthreads_count(occurs ? 1 : 0);   // (also orders the zeroing of per_class)
  if (occurs && !(present == kIds && t == kIds - 1)) atomicAdd(per_class + best_c, 1);
  __syncthreads();
  if (t < ncls) {
    unsigned tp_fn = 0u, tp_fp = 0u, tp = 0u;
    if (ok) {
      for (int q = 0; q < pair_cols; ++q) tp_fn += pair[t * pair_cols + q];
      for (int g = 0; g < ncls; ++g) tp_fp += pair[g * pair_cols + t] + (t == ncls - 1 ? pair[g * pair_cols + ncls] : 0u);
      tp = pair[t * pair_cols + t];
    }
    int64_t* out = stats + (size_t)file * 4 * ncls;
    out[t] = (int64_t)tp_fn;
    out[ncls + t] = (int64_t)tp_fp;
    out[2 * ncls + t] = (int64_t)tp;
    out[3 * ncls + t] = (int64_t)per_class[t];
  }
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_score_params_bytes(void) { return sizeof(spml_score_params); }

extern "C" size_t spml_score_batch_workspace_bytes(int B, int ncls) {
  if (!limits_ok(B, ncls)) return 0;
  return (size_t)B * file_entries(ncls) * sizeof(unsigned);
}

extern "C" const char* spml_score_batch_path_name(const spml_score_params* records, int B, int64_t packed_bytes,
                                                  int ncls) {
  if (!batch_ok(records, B, packed_bytes, ncls)) return "unsupported";
  return file_entries(ncls) <= kLdsEntries ? "lds_table" : "global_table";
}

extern "C" int spml_score_batch_u8(const unsigned char* packed, int64_t packed_bytes,
                                   const spml_score_params* params_host, const spml_score_params* params_dev, int B,
                                   int ncls, int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!packed || !params_host || !params_dev || !stats || packed_bytes < 0) return SPML_ERR_INVALID_ARG;
  if (((uintptr_t)packed & (kVec - 1)) != 0 || ((uintptr_t)params_dev & 7) != 0 || ((uintptr_t)stats & 7) != 0)
    return SPML_ERR_INVALID_ARG;
  if (!batch_ok(params_host, B, packed_bytes, ncls)) return SPML_ERR_UNSUPPORTED;
  const size_t need = spml_score_batch_workspace_bytes(B, ncls);
  if (!ws || ws_bytes < need) return SPML_ERR_WORKSPACE;
  if (((uintptr_t)ws & 3) != 0) return SPML_ERR_INVALID_ARG;
  const size_t stats_bytes = (size_t)B * 4 * ncls * sizeof(int64_t), params_bytes = (size_t)B * sizeof(spml_score_params);
  // what is written (stats, ws) may overlap neither an input nor each other
  if (overlap(stats, stats_bytes, packed, (size_t)packed_bytes) || overlap(stats, stats_bytes, params_dev, params_bytes) ||
      overlap(ws, need, packed, (size_t)packed_bytes) || overlap(ws, need, params_dev, params_bytes) ||
      overlap(stats, stats_bytes, ws, need))
    return SPML_ERR_INVALID_ARG;
  int64_t runs = 0;
  for (int b = 0; b < B; ++b) runs += runs_of(params_host[b].n);                       // <= 256 * 2^18
  hipStream_t s = (hipStream_t)stream;
  unsigned* tables = static_cast<unsigned*>(ws);
  if (hipMemsetAsync(tables, 0, need, s) != hipSuccess) return SPML_ERR_LAUNCH;
  hipLaunchKernelGGL(file_entries(ncls) <= kLdsEntries ? count<true> : count<false>, dim3((unsigned)runs), dim3(kBlock),
                     0, s, packed, packed_bytes, params_dev, B, ncls, tables);
  hipLaunchKernelGGL(finish, dim3((unsigned)B), dim3(kIds), 0, s, params_dev, packed_bytes, ncls,
                     (const unsigned*)tables, stats);
  return launch_status();
}
