// Counting pixels into a [segments][classes] table of 32-bit integers: the body segment_majority.hip and segment_cam.hip
// share.  A workgroup owns a contiguous run of pixels (segments are spatially coherent: a run touches few bins).  Where
// the table fits kLdsEntries it is counted in LDS (ds_add_u32) and flushed once per workgroup, skipping the bins that
// stayed zero; otherwise the adds go to the global table directly.  kLdsEntries = 8192 (32 KiB): five workgroups of a CU
// keep their tables in its 160 KiB of LDS at once, and zeroing plus scanning the table (32 entries per thread) stays in
// proportion to the 8 pixels a thread counts.
// Only integer atomics: integer adds commute, so the result does not depend on the arrival order.  Counters are 32 bits
// wide: P < 2^31 bounds every bin.
//
// Equal keys are merged inside a wave before the atomic: groups of equal keys are peeled off the wave (ballot, shuffle of
// the first pending lane's key, one add of the group's size by that lane).  SPML_MAJORITY_WAVE_COMBINE=0 compiles the
// plain form (one atomic per counted pixel); tools/bench_prototype_msc.py times the two (profiles/prototype_msc.md).
//
// The caller's `bin(p, end)` gives the table entry of pixel p, or -1 when the pixel counts nowhere (p >= end included).
#pragma once

#include "common.hpp"

#ifndef SPML_MAJORITY_WAVE_COMBINE
#define SPML_MAJORITY_WAVE_COMBINE 1
#endif

namespace spml {
namespace segcount {

constexpr int kLdsEntries = 8192;          // 32 KiB of uint32 counters per workgroup
constexpr int kBlock = 256;
constexpr int kPixelsPerThread = 8;
constexpr int kMaxBlocks = 2048;

// one count per lane with key >= 0.  Every lane of the wave calls this (the loop bounds of the callers are
// wave-uniform), so the ballots see the whole wave.
__device__ __forceinline__ void add_one(unsigned* table, int key) {
#if SPML_MAJORITY_WAVE_COMBINE
  const int lane = threadIdx.x & (kWave - 1);
  bool pending = key >= 0;
  for (;;) {
    const unsigned long long todo = __ballot(pending);
    if (todo == 0) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int lead_key = __shfl(key, leader, kWave);
    const bool mine = pending && key == lead_key;
    const unsigned long long group = __ballot(mine);
    if (lane == leader) atomicAdd(table + lead_key, (unsigned)__popcll(group));
    if (mine) pending = false;
  }
#else
  if (key >= 0) atomicAdd(table + key, 1u);
#endif
}

// workgroup b counts the pixels [b * chunk, min(P, (b + 1) * chunk)); chunk is a multiple of kBlock.  `local`: the
// workgroup's kLdsEntries counters in LDS.
template <typename Bin>
__device__ __forceinline__ void count_lds(const Bin& bin, int64_t P, int64_t chunk, int entries, unsigned* local,
                                          unsigned* __restrict__ table) {
  for (int e = threadIdx.x; e < entries; e += kBlock) local[e] = 0u;
  __syncthreads();
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < P ? begin + chunk : P;
  for (int64_t base = begin; base < end; base += kBlock) add_one(local, bin(base + threadIdx.x, end));
  __syncthreads();
  for (int e = threadIdx.x; e < entries; e += kBlock) {
    const unsigned v = local[e];
    if (v != 0u) atomicAdd(table + e, v);
  }
}

template <typename Bin>
__device__ __forceinline__ void count_global(const Bin& bin, int64_t P, int64_t chunk, unsigned* __restrict__ table) {
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < P ? begin + chunk : P;
  for (int64_t base = begin; base < end; base += kBlock) add_one(table, bin(base + threadIdx.x, end));
}

// the grid of a count launch over P > 0 pixels: `blocks` workgroups of kBlock threads, `chunk` pixels each
struct Chunks {
  int64_t blocks, chunk;
};

inline Chunks plan_chunks(int64_t P) {
  int64_t blocks = (P + (int64_t)kBlock * kPixelsPerThread - 1) / ((int64_t)kBlock * kPixelsPerThread);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const int64_t chunk = ((P + blocks - 1) / blocks + kBlock - 1) / kBlock * kBlock;
  return {(P + chunk - 1) / chunk, chunk};
}

inline bool overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return pn != 0 && qn != 0 && p0 < q0 + qn && q0 < p0 + pn;
}

}  // namespace segcount
}  // namespace spml
