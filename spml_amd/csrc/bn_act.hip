// Training-mode batch normalisation fused with the ReLU and the residual add around it, for
// channels-last (NHWC) fp32 activations [R = N*H*W, C].
//
// The reference's ResNet bottleneck (spml/models/backbones/resnet.py:42-63) runs
//   bn(conv(x)) -> relu        (twice)      and      bn(conv(x)) + identity -> relu
// as separate framework ops: per unit 3 batch norms (two passes over the tensor each), 3 ReLUs
// and 1 add -- 20 % of the GPU time of the training step once the convolutions are tuned
// (profiles/r02_train_step_steady_state.md).  Here one statistics pass + one apply pass do
// normalise + scale/shift (+ residual) (+ ReLU), and the backward is one reduction pass + one
// apply pass that also yields the gradient of the residual branch.  HBM-bound, float4 accesses.
//
// Four kernels carry every pass:
//   bn_partial<MODE, MASK>  per chunk of rows and channel: MODE 0 mean and sum of squared deviations (+ max / min),
//                           MODE 1 sum(dz), sum(dz * (x - mean)) (+ max |dz|)   with dz = dy * (y > 0)
//   bn_merge<MODE>          the chunks pooled in a fixed order (Chan's formula: no E[x^2] - E[x]^2 cancellation);
//                           single-rank calls finalise (invstd, running statistics) and bound the output tensor here
//   bn_apply<HAS_RES>       y = act((x - mean) * invstd * gamma + beta [+ residual]) as fp32, hl8 and / or ReLU mask
//   bn_bwd_apply<MASK>      dx = gamma * invstd * (dz - sum_dz/n - xhat * sum_dz_xhat/n) as fp32 and / or hl8; dres = dz
// Entry points (the host side at the end of the file; include/spml_hip.h has the contracts):
//   spml_bn_stats_f32 / _act_apply_f32 / _act_bwd_reduce_f32 / _act_bwd_apply_f32   one pass each: SyncBatchNorm
//       combines the ranks' statistics between the halves (spml_bn_finalize_f32, spml_bn_finalize_ranks_f32)
//   spml_bn_act_fwd_f32 / _act_bwd_f32                                              single rank: one call per direction
//   spml_bn_stats_ext_f32 / _act_apply_hl8_f32 / _act_bwd_reduce_ext_f32 / _act_bwd_apply_hl8_f32, spml_bn_fwd_hl8_f32 /
//       _bwd_hl8_f32                the same two families with the split-f16 (hl8) copies, bounds and mask bytes that
//                                   the matrix-core convolutions consume (C % 8 == 0)
//   spml_bn_*_chunks_f32            ... pooled from the chunk statistics a convolution's epilogue left: no partial pass
#include "common.hpp"

namespace spml {
namespace {


// hl8 = split-f16 copy of a tensor (csrc/conv.hip): 16-byte units ((row*C/8 + c/8)*2 + part) of
// 8 channels; a channel quad q is half a unit.
// ReLU mask: one byte per (row, channel quad), bit e = (y[4q+e] > 0) -- 0.25 B per element for the
// backward passes instead of re-reading y.
__device__ __forceinline__ float4v relu_mask_bits(float4v dz, const unsigned char* __restrict__ mask, size_t row,
                                                  int C, int q) {
  const unsigned m = mask[row * (size_t)(C >> 2) + q];
#pragma unroll
  for (int e = 0; e < 4; ++e) dz[e] = (m >> e) & 1u ? dz[e] : 0.f;
  return dz;
}

// S = 2^(14 - e) for the smallest e with bound < 2^e (same rule as csrc/conv.hip)
__device__ __forceinline__ float bn_pow2_scale(float bound) {
  if (!(bound > 0.f) || bound > 1e38f) return 1.f;
  int e;
  (void)frexpf(bound, &e);
  e = 14 - e;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  return ldexpf(1.f, e);
}

// One channel quad (4 values) of row `row` into the hl8 tensor.  A 16-byte unit holds 8 channels of one part: the two
// lanes of a quad pair (q, q ^ 1: adjacent lanes, same row) exchange halves so that the even lane stores the whole h
// unit and the odd lane the whole l unit -- one contiguous kilobyte per wave store instead of two instructions that
// each fill every other 8 bytes (bn_bwd_apply ran at 3 TB/s with those).  Every lane of the pair must call it.
__device__ __forceinline__ void store_hl8_quad(uint2* __restrict__ out, size_t row, int C, int q, float4v v,
                                               float s) {
  union { uint2 u; _Float16 h[4]; } hh, ll;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = v[e] * s;
    const _Float16 h = (_Float16)x;
    hh.h[e] = h;
    ll.h[e] = (_Float16)(x - (float)h);
  }
  const bool odd = (q & 1) != 0;
  const uint2 send = odd ? hh.u : ll.u;            // the even lane needs the partner's h half, the odd lane its l half
  uint2 recv;
  recv.x = (unsigned)__shfl_xor((int)send.x, 1, kWave);
  recv.y = (unsigned)__shfl_xor((int)send.y, 1, kWave);
  uint4 unit;
  if (odd) { unit.x = recv.x; unit.y = recv.y; unit.z = ll.u.x; unit.w = ll.u.y; }
  else { unit.x = hh.u.x; unit.y = hh.u.y; unit.z = recv.x; unit.w = recv.y; }
  reinterpret_cast<uint4*>(out)[(row * (size_t)(C >> 3) + (q >> 1)) * 2 + (odd ? 1 : 0)] = unit;
}

// block = 256 threads = CQ channel quads x (256 / CQ) row lanes; grid (C / (4*CQ), chunks)
// MODE 0: (sum, sumsq) of x -> (mean, M2) of the chunk;  MODE 1: (sum dz, sum dz * (x - mean))
template <int MODE, int MASK>
__global__ __launch_bounds__(256) void bn_partial(const float* __restrict__ x, const float* __restrict__ dy,
                                                  const float* __restrict__ y, const float* __restrict__ mean,
                                                  int64_t R, int C, int cq, int chunk_rows,
                                                  float* __restrict__ pa, float* __restrict__ pb,
                                                  const unsigned char* __restrict__ yh, float* __restrict__ pc,
                                                  float* __restrict__ pd, float* __restrict__ zero_me) {
  // zero_me: the tensor-bound slot the following bn_merge max-reduces into (single-rank calls)
  if (zero_me && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *zero_me = 0.f;
  // pc / pd (optional): MODE 0 per-channel max / min of x, MODE 1 max |dz| (the bounds that fix
  // the power-of-two scale of the split-f16 copies, csrc/conv.hip); yh (MASK 2): the ReLU mask
  // bytes written by bn_apply instead of an fp32 y
  __shared__ float4v sa[256], sb[256];
  const int tx = threadIdx.x % cq, ty = threadIdx.x / cq, nty = 256 / cq;
  const int q = blockIdx.x * cq + tx;                       // channel quad
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
  const int nrows = (int)min((int64_t)chunk_rows, R - r0);
  const int cquads = C >> 2;
  float4v a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
  float4v mu = {0.f, 0.f, 0.f, 0.f};
  float4v hi = {-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f}, lo = {3.4e38f, 3.4e38f, 3.4e38f, 3.4e38f};
  if (MODE == 1) hi = a;
  if (q < cquads) {
    // MODE 0: sums are taken relative to the mean of the chunk's first four rows (a per-channel shift), so that
    // sumsq - n * mean^2 does not cancel when |mean| >> std.  The rounding of the accumulated sumsq is magnified by
    // 1 + ((shift - chunk mean) / std)^2 in M2: with the first row alone as the shift that was ~10 for the unluckiest
    // of a few hundred channels (3 sigma), and a whole-tensor M2 4e-6 off where one chunk dominates
    // (profiles/bn_branch_parity.md); four rows halve the sigma.  1, 2 or 4 rows: a constant channel keeps an exact
    // shift (pairwise sums, power-of-two count) and M2 = 0.  MODE 1: the batch mean
    if (MODE == 1) {
      mu = *reinterpret_cast<const float4v*>(mean + 4 * q);
    } else {
      const float* xs = x + (size_t)r0 * C + 4 * q;
      const float4v s0 = *reinterpret_cast<const float4v*>(xs);
      const float4v s1 = nrows >= 2 ? *reinterpret_cast<const float4v*>(xs + C) : s0;
      const float4v s2 = nrows >= 4 ? *reinterpret_cast<const float4v*>(xs + 2 * (size_t)C) : s0;
      const float4v s3 = nrows >= 4 ? *reinterpret_cast<const float4v*>(xs + 3 * (size_t)C) : s1;
      mu = ((s0 + s1) + (s2 + s3)) * 0.25f;
    }
#pragma unroll 4
    for (int r = ty; r < nrows; r += nty) {
      const size_t o = (size_t)(r0 + r) * C + 4 * q;
      const float4v xv = *reinterpret_cast<const float4v*>(x + o);
      if (MODE == 0) {
        const float4v d = xv - mu;
        a += d;
        b += d * d;
#pragma unroll
        for (int e = 0; e < 4; ++e) { hi[e] = fmaxf(hi[e], xv[e]); lo[e] = fminf(lo[e], xv[e]); }
      } else {
        float4v dz = *reinterpret_cast<const float4v*>(dy + o);
        if (MASK == 1) {
          const float4v yv = *reinterpret_cast<const float4v*>(y + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) dz[e] = yv[e] > 0.f ? dz[e] : 0.f;
        } else if (MASK == 2) {
          dz = relu_mask_bits(dz, yh, (size_t)(r0 + r), C, q);
        }
        a += dz;
        b += dz * (xv - mu);
#pragma unroll
        for (int e = 0; e < 4; ++e) hi[e] = fmaxf(hi[e], fabsf(dz[e]));
      }
    }
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  if (ty == 0 && q < cquads) {
    for (int i = 1; i < nty; ++i) { a += sa[i * cq + tx]; b += sb[i * cq + tx]; }
    if (MODE == 0) {
      const float inv = 1.0f / (float)nrows;
      const float4v m = a * inv;          // mean of the shifted values
      b = b - m * m * (float)nrows;       // chunk M2 (shift invariant)
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = fmaxf(b[e], 0.f);
      a = m + mu;                         // chunk mean
    }
    *reinterpret_cast<float4v*>(pa + (size_t)blockIdx.y * C + 4 * q) = a;
    *reinterpret_cast<float4v*>(pb + (size_t)blockIdx.y * C + 4 * q) = b;
  }
  if (pc) {                                  // block-uniform
    __syncthreads();
    sa[threadIdx.x] = hi;
    sb[threadIdx.x] = lo;
    __syncthreads();
    if (ty == 0 && q < cquads) {
      for (int i = 1; i < nty; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hi[e] = fmaxf(hi[e], sa[i * cq + tx][e]);
          lo[e] = fminf(lo[e], sb[i * cq + tx][e]);
        }
      }
      *reinterpret_cast<float4v*>(pc + (size_t)blockIdx.y * C + 4 * q) = hi;
      if (MODE == 0) *reinterpret_cast<float4v*>(pd + (size_t)blockIdx.y * C + 4 * q) = lo;
    }
  }
}

// Merge of the chunk partials: block = 16 channels x 64 chunk lanes, fixed summation order
// (deterministic).  MODE 0 extras (single-rank batch norm: everything in this kernel, no
// framework ops in between): fin != 0 -> out_b receives invstd = rsqrt(M2 / R + eps) instead of M2
// and the running statistics are updated (momentum, unbiased variance).
struct BnFinal { int fin; float eps, momentum; float* running_mean; float* running_var; };
// single-rank calls: the tensor bound (csrc/conv.hip) is max-reduced here instead of a launch of
// its own.  MODE 0: max_c |bn(x)_c| (+ *res_bound) from this kernel's mean / invstd / extremes;
// MODE 1: the bound of |dx| from the sums of this kernel and the forward's extremes.
struct BnBound {
  float* bound;
  const float* res_bound;
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* cmax;
  const float* cmin;
  float inv_count;
};
// 256-thread workgroups (one wave per SIMD): a 1024-thread one needs four free wave slots on every SIMD of
// a CU at once and queued behind the side stream's weight-gradient workgroups in the backward pass
// (median 57 us against 12 us for the same merge in the forward pass)
constexpr int kMergeLanes = 64, kMergeCh = 4;

__device__ inline float merge_lanes(float v, float* sh, int tx, int ty) {
  __syncthreads();
  sh[ty * kMergeCh + tx] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll 16
  for (int i = 0; i < kMergeLanes; ++i) t += sh[i * kMergeCh + tx];
  return t;
}

template <int MODE>
__global__ __launch_bounds__(kMergeCh * kMergeLanes) void bn_merge(
    const float* __restrict__ pa, const float* __restrict__ pb, int64_t R, int C, int chunks, int chunk_rows,
    const float* __restrict__ invstd, float* __restrict__ out_a, float* __restrict__ out_b, BnFinal f,
    const float* __restrict__ pc, const float* __restrict__ pd, float* __restrict__ out_c,
    float* __restrict__ out_d, BnBound bb) {
  __shared__ float sh[kMergeCh * kMergeLanes];
  __shared__ float sh_bound[kMergeCh];      // the block's (up to) four bound candidates: ONE atomicMax per block
  const int tx = threadIdx.x % kMergeCh, ty = threadIdx.x / kMergeCh;
  // (the live threads of a block are lanes 0 .. 3 of its first wave: they meet wave-synchronously through sh_bound;
  // every channel used to send its own atomicMax to the ONE bound word -- C same-address atomics in a row)
  const int n_live = min(kMergeCh, C - (int)blockIdx.x * kMergeCh);
  auto publish_bound = [&](float v) {
    sh_bound[tx] = v;
    __builtin_amdgcn_wave_barrier();
    if (tx == 0) {
      unsigned m = __float_as_uint(v);       // (bit patterns, as the atomic itself compares them: a NaN stays the maximum)
      for (int i = 1; i < n_live; ++i) m = max(m, __float_as_uint(sh_bound[i]));
      atomicMax(reinterpret_cast<unsigned*>(bb.bound), m);
    }
  };
  const int c = min(blockIdx.x * kMergeCh + tx, C - 1);
  const bool live = blockIdx.x * kMergeCh + tx < C && ty == 0;
  float hi = -3.4e38f, lo = 3.4e38f;
  // Up to kMergeRegs x kMergeLanes chunks: every value this thread folds is requested up front -- pa, pb and the
  // extremes, all loads in flight together -- and the three reductions below run on registers.  The loops they replace
  // waited for a batch of four loads at a time, three dependent phases in a row: ~12 memory round trips per call, and
  // ~200 calls sit on the critical path of a training step (12-14 us each; the same arithmetic in the same order).
  constexpr int kMergeRegs = 16;
  const bool in_regs = chunks <= kMergeRegs * kMergeLanes;
  const bool ext = pc && out_c;
  float ra[kMergeRegs], rb[kMergeRegs], rc[kMergeRegs], rd[kMergeRegs];
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < kMergeRegs; ++j) {
      const int i = ty + j * kMergeLanes;
      const bool ok = i < chunks;
      const size_t o = (size_t)(ok ? i : 0) * C + c;
      ra[j] = ok ? pa[o] : 0.f;
      rb[j] = ok ? pb[o] : 0.f;
      rc[j] = (ok && ext) ? pc[o] : -3.4e38f;
      rd[j] = (ok && ext && MODE == 0) ? pd[o] : 3.4e38f;
    }
  }
  // the per-channel coefficients the epilogue of a live thread needs (gamma / beta / residual bound / running statistics;
  // MODE 1: invstd, mean, extremes, gamma) are requested here, with the chunk values: behind the reductions they were
  // one more dependent round trip per call
  float p_gamma = 0.f, p_beta = 0.f, p_res = 0.f, p_rm = 0.f, p_rv = 0.f, p_is = 0.f, p_mu = 0.f, p_cmax = 0.f, p_cmin = 0.f;
  const float p_ref = MODE == 0 ? pa[c] : 0.f;      // chunk 0's mean (every thread of the channel: the shift of the pooled mean)
  if (live) {
    if (MODE == 0) {
      if (f.fin && bb.bound) { p_gamma = bb.gamma[c]; p_beta = bb.beta[c]; p_res = bb.res_bound ? *bb.res_bound : 0.f; }
      if (f.fin && f.running_mean) { p_rm = f.running_mean[c]; p_rv = f.running_var[c]; }
    } else {
      p_is = invstd[c];
      if (bb.bound) { p_mu = bb.mean[c]; p_cmax = bb.cmax[c]; p_cmin = bb.cmin[c]; p_gamma = bb.gamma[c]; }
    }
  }
  if (ext) {                               // extremes of the chunks (max / min; MODE 1: max only)
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < kMergeRegs; ++j) {
        hi = fmaxf(hi, rc[j]);
        if (MODE == 0) lo = fminf(lo, rd[j]);
      }
    } else {
#pragma unroll 4
      for (int i = ty; i < chunks; i += kMergeLanes) {
        hi = fmaxf(hi, pc[(size_t)i * C + c]);
        if (MODE == 0) lo = fminf(lo, pd[(size_t)i * C + c]);
      }
    }
    __syncthreads();
    sh[ty * kMergeCh + tx] = hi;
    __syncthreads();
    for (int i = 0; i < kMergeLanes; ++i) hi = fmaxf(hi, sh[i * kMergeCh + tx]);
    if (MODE == 0) {
      __syncthreads();
      sh[ty * kMergeCh + tx] = lo;
      __syncthreads();
      for (int i = 0; i < kMergeLanes; ++i) lo = fminf(lo, sh[i * kMergeCh + tx]);
    }
    if (live) {
      out_c[c] = hi;
      if (MODE == 0) out_d[c] = lo;
    }
  }
  if (MODE == 0) {
    // pooled mean first, then the M2 terms (Chan): two independent sums, no division in the loops.  The means are
    // pooled relative to chunk 0's: the sum of mean_i * n_i itself rounds at |mean|, which left the mean of a
    // constant channel one ulp off its value -- M2 > 0 and y = beta + gamma * ulp / sqrt(eps) instead of beta
    float sm = 0.f;
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < kMergeRegs; ++j) {
        const int i = ty + j * kMergeLanes;
        if (i < chunks) {
          const float nb = (float)min((int64_t)chunk_rows, R - (int64_t)i * chunk_rows);
          sm += (ra[j] - p_ref) * nb;
        }
      }
    } else {
#pragma unroll 4
      for (int i = ty; i < chunks; i += kMergeLanes) {
        const float nb = (float)min((int64_t)chunk_rows, R - (int64_t)i * chunk_rows);
        sm += (pa[(size_t)i * C + c] - p_ref) * nb;
      }
    }
    const float m = p_ref + merge_lanes(sm, sh, tx, ty) / (float)R;
    float m2 = 0.f;
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < kMergeRegs; ++j) {
        const int i = ty + j * kMergeLanes;
        if (i < chunks) {
          const float nb = (float)min((int64_t)chunk_rows, R - (int64_t)i * chunk_rows);
          const float d = ra[j] - m;
          m2 += rb[j] + d * d * nb;
        }
      }
    } else {
#pragma unroll 4
      for (int i = ty; i < chunks; i += kMergeLanes) {
        const float nb = (float)min((int64_t)chunk_rows, R - (int64_t)i * chunk_rows);
        const float d = pa[(size_t)i * C + c] - m;
        m2 += pb[(size_t)i * C + c] + d * d * nb;
      }
    }
    m2 = merge_lanes(m2, sh, tx, ty);
    if (!live) return;
    out_a[c] = m;
    if (f.fin) {
      const float is = 1.0f / sqrtf(m2 / (float)R + f.eps);
      out_b[c] = is;
      if (bb.bound) {
        const float sc = p_gamma * is, b = p_beta;
        const float v = fmaxf(fabsf((hi - m) * sc + b), fabsf((lo - m) * sc + b)) * 1.0001f + p_res;
        publish_bound(v);
      }
      if (f.running_mean) {
        f.running_mean[c] = (1.f - f.momentum) * p_rm + f.momentum * m;
        f.running_var[c] = (1.f - f.momentum) * p_rv +
                           f.momentum * (m2 / (float)(R > 1 ? R - 1 : 1));
      }
    } else {
      out_b[c] = m2;
    }
  } else {
    float s0 = 0.f, s1 = 0.f;
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < kMergeRegs; ++j)
        if (ty + j * kMergeLanes < chunks) { s0 += ra[j]; s1 += rb[j]; }
    } else {
      for (int i = ty; i < chunks; i += kMergeLanes) { s0 += pa[(size_t)i * C + c]; s1 += pb[(size_t)i * C + c]; }
    }
    s0 = merge_lanes(s0, sh, tx, ty);
    s1 = merge_lanes(s1, sh, tx, ty);
    if (!live) return;
    out_a[c] = s0;                        // sum dz
    out_b[c] = s1 * p_is;                 // sum dz * xhat
    if (bb.bound) {
      const float is = p_is, mu = p_mu;
      const float xh = fmaxf(fabsf(p_cmax - mu), fabsf(p_cmin - mu)) * is;
      const float v = fabsf(p_gamma * is) *
                      (hi + fabsf(s0) * bb.inv_count + xh * fabsf(s1 * is) * bb.inv_count) * 1.0001f;
      publish_bound(v);
    }
  }
}

// apply kernels: block = cq channel quads x (256 / cq) row lanes, grid (C / (4*cq), row tiles);
// a thread keeps its channel quad's coefficients in registers and walks down the rows of its
// tile (BnGeom::apply_rows: ~4096 blocks per launch, at most 256 rows each)

template <bool HAS_RES>
__global__ __launch_bounds__(256) void bn_apply(const float* __restrict__ x, const float* __restrict__ res,
                                                int64_t R, int C, int cq, int apply_rows,
                                                const float* __restrict__ mean,
                                                const float* __restrict__ invstd,
                                                const float* __restrict__ gamma,
                                                const float* __restrict__ beta, int relu,
                                                float* __restrict__ y, uint2* __restrict__ yh,
                                                const float* __restrict__ ybound,
                                                unsigned char* __restrict__ mask) {
  const int tx = threadIdx.x % cq, ty = threadIdx.x / cq, nty = 256 / cq;
  const int q = blockIdx.x * cq + tx;
  if (q >= (C >> 2)) return;
  const float ys = yh ? bn_pow2_scale(*ybound) : 1.f;
  const float4v mu = *reinterpret_cast<const float4v*>(mean + 4 * q);
  const float4v sc = *reinterpret_cast<const float4v*>(invstd + 4 * q) *
                     *reinterpret_cast<const float4v*>(gamma + 4 * q);
  const float4v sh = *reinterpret_cast<const float4v*>(beta + 4 * q);
  const int64_t r0 = (int64_t)blockIdx.y * apply_rows;
  const int64_t r1 = min(R, r0 + apply_rows);
#pragma unroll 4
  for (int64_t r = r0 + ty; r < r1; r += nty) {
    const size_t o = (size_t)r * C + 4 * q;
    float4v v = (*reinterpret_cast<const float4v*>(x + o) - mu) * sc + sh;
    if (HAS_RES) v += *reinterpret_cast<const float4v*>(res + o);
    if (relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    if (y) *reinterpret_cast<float4v*>(y + o) = v;
    if (yh) store_hl8_quad(yh, (size_t)r, C, q, v, ys);
    if (mask)
      mask[(size_t)r * (C >> 2) + q] = (unsigned char)((v[0] > 0.f) | ((v[1] > 0.f) << 1) | ((v[2] > 0.f) << 2) |
                                                       ((v[3] > 0.f) << 3));
  }
}

template <int MASK>
__global__ __launch_bounds__(256) void bn_bwd_apply(const float* __restrict__ dy, const float* __restrict__ y,
                                                    const float* __restrict__ x, int64_t R, int C, int cq,
                                                    int apply_rows, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma,
                                                    const float* __restrict__ sum_dz,
                                                    const float* __restrict__ sum_dz_xhat, float inv_count,
                                                    const float* __restrict__ count_dev,
                                                    float* __restrict__ dx, float* __restrict__ dres,
                                                    const unsigned char* __restrict__ yh, uint2* __restrict__ dxh,
                                                    const float* __restrict__ dxbound) {
  const int tx = threadIdx.x % cq, ty = threadIdx.x / cq, nty = 256 / cq;
  const int q = blockIdx.x * cq + tx;
  if (q >= (C >> 2)) return;
  if (count_dev) inv_count = 1.f / count_dev[0];      // pooled row count of all ranks (SyncBatchNorm)
  const float ds = dxh ? bn_pow2_scale(*dxbound) : 1.f;
  float4v mu = {0.f, 0.f, 0.f, 0.f}, is = mu, gi = mu, c0 = mu, c1 = mu;
  if (dx || dxh) {
    mu = *reinterpret_cast<const float4v*>(mean + 4 * q);
    is = *reinterpret_cast<const float4v*>(invstd + 4 * q);
    gi = *reinterpret_cast<const float4v*>(gamma + 4 * q) * is;
    c0 = *reinterpret_cast<const float4v*>(sum_dz + 4 * q) * inv_count;
    c1 = *reinterpret_cast<const float4v*>(sum_dz_xhat + 4 * q) * inv_count;
  }
  const int64_t r0 = (int64_t)blockIdx.y * apply_rows;
  const int64_t r1 = min(R, r0 + apply_rows);
#pragma unroll 4
  for (int64_t r = r0 + ty; r < r1; r += nty) {
    const size_t o = (size_t)r * C + 4 * q;
    float4v dz = *reinterpret_cast<const float4v*>(dy + o);
    if (MASK == 1) {
      const float4v yv = *reinterpret_cast<const float4v*>(y + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) dz[e] = yv[e] > 0.f ? dz[e] : 0.f;
    } else if (MASK == 2) {
      dz = relu_mask_bits(dz, yh, (size_t)r, C, q);
    }
    if (dres) *reinterpret_cast<float4v*>(dres + o) = dz;
    if (dx || dxh) {
      const float4v xh = (*reinterpret_cast<const float4v*>(x + o) - mu) * is;
      const float4v g = gi * (dz - c0 - xh * c1);
      if (dx) *reinterpret_cast<float4v*>(dx + o) = g;
      if (dxh) store_hl8_quad(dxh, (size_t)r, C, q, g, ds);
    }
  }
}

// upper bounds of |y| and |dx| over the whole tensor from the per-channel extremes (one block)
__device__ __forceinline__ float block_max_256(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__global__ __launch_bounds__(256) void bn_bound_fwd(int C, const float* __restrict__ cmax,
                                                    const float* __restrict__ cmin,
                                                    const float* __restrict__ mean,
                                                    const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma,
                                                    const float* __restrict__ beta,
                                                    const float* __restrict__ res_bound, float* __restrict__ out) {
  __shared__ float sh[4];
  float m = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float sc = gamma[c] * invstd[c];
    m = fmaxf(m, fmaxf(fabsf((cmax[c] - mean[c]) * sc + beta[c]), fabsf((cmin[c] - mean[c]) * sc + beta[c])));
  }
  m = block_max_256(m, sh);
  if (threadIdx.x == 0) out[0] = m * 1.0001f + (res_bound ? res_bound[0] : 0.f);
}

__global__ __launch_bounds__(256) void bn_bound_bwd(int C, const float* __restrict__ max_dz,
                                                    const float* __restrict__ cmax,
                                                    const float* __restrict__ cmin,
                                                    const float* __restrict__ mean,
                                                    const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma,
                                                    const float* __restrict__ sum_dz,
                                                    const float* __restrict__ sum_dz_xhat, float inv_count,
                                                    const float* __restrict__ count_dev,
                                                    float* __restrict__ out) {
  __shared__ float sh[4];
  float m = 0.f;
  if (count_dev) inv_count = 1.f / count_dev[0];
  for (int c = threadIdx.x; c < C; c += 256) {
    const float xh = fmaxf(fabsf(cmax[c] - mean[c]), fabsf(cmin[c] - mean[c])) * invstd[c];
    m = fmaxf(m, fabsf(gamma[c] * invstd[c]) *
                     (max_dz[c] + fabsf(sum_dz[c]) * inv_count + xh * fabsf(sum_dz_xhat[c]) * inv_count));
  }
  m = block_max_256(m, sh);
  if (threadIdx.x == 0) out[0] = m * 1.0001f;
}

__global__ __launch_bounds__(256) void bn_finalize(int C, const float* __restrict__ mean,
                                                   const float* __restrict__ m2, float count, float eps,
                                                   float momentum, float* __restrict__ running_mean,
                                                   float* __restrict__ running_var, float* __restrict__ invstd) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  invstd[c] = 1.0f / sqrtf(m2[c] / count + eps);
  if (running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean[c];
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (m2[c] / (count > 1.f ? count - 1.f : 1.f));
  }
}

// SyncBatchNorm: pooled statistics of `world` ranks (Chan) + finalisation in one launch.
// stats [world][3][C] = per-rank (count, mean, M2) as gathered by the caller.
__global__ __launch_bounds__(256) void bn_finalize_ranks(int C, int world, const float* __restrict__ stats,
                                                         float eps, float momentum,
                                                         float* __restrict__ running_mean,
                                                         float* __restrict__ running_var,
                                                         float* __restrict__ mean_out,
                                                         float* __restrict__ invstd,
                                                         float* __restrict__ total_out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float total = 0.f, sm = 0.f;
  for (int r = 0; r < world; ++r) {
    const float n = stats[((size_t)r * 3 + 0) * C + c];
    total += n;
    sm += n * stats[((size_t)r * 3 + 1) * C + c];
  }
  const float m = sm / total;
  float m2 = 0.f;
  for (int r = 0; r < world; ++r) {
    const float n = stats[((size_t)r * 3 + 0) * C + c];
    const float d = stats[((size_t)r * 3 + 1) * C + c] - m;
    m2 += stats[((size_t)r * 3 + 2) * C + c] + d * d * n;
  }
  mean_out[c] = m;
  invstd[c] = 1.0f / sqrtf(m2 / total + eps);
  if (total_out && c == 0) total_out[0] = total;
  if (running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (m2 / (total > 1.f ? total - 1.f : 1.f));
  }
}

// ---- Host side.  bn_geom fixes the launch geometry of an [R, C] tensor once per call: the workspace size, every grid
// and every kernel argument read it.  One launcher per kernel takes the geometry, the stream, R and C, and a record of
// the kernel's pointers in which what a call does not pass stays null; a function returns the template variant.
// cq channel quads per 256-thread block (256 / cq row lanes), col_blocks = grid.x of the partial and apply kernels;
// chunks of chunk_rows rows for the partial statistics (grid.y of bn_partial, depth of the merge): enough to fill the
// chip (~1024 blocks), at most 1024, at least 128 rows each; apply_rows per block of the apply kernels (~4096 blocks)
struct BnGeom { int cq, col_blocks, chunks, chunk_rows, apply_rows; };
inline BnGeom bn_geom(int64_t R, int C) {
  BnGeom g;
  const int q = C >> 2;
  g.cq = q >= 64 ? 64 : (q >= 32 ? 32 : (q >= 16 ? 16 : (q >= 8 ? 8 : 4)));
  g.col_blocks = (q + g.cq - 1) / g.cq;
  const int64_t target = std::min<int64_t>(1024, std::max<int64_t>(1, 1024 / std::max(g.col_blocks, 1)));
  g.chunk_rows = (int)std::max<int64_t>(128, (R + target - 1) / target);
  g.chunks = (int)((R + g.chunk_rows - 1) / g.chunk_rows);
  const int nty = 256 / g.cq;
  const int64_t rows = (R * g.col_blocks + 4095) / 4096;
  g.apply_rows = (int)std::min<int64_t>(256, std::max<int64_t>(nty, (rows + nty - 1) / nty * nty));
  return g;
}
// ... with the chunks a producer left (the epilogue of a convolution, csrc/conv.hip) in place of its own
inline BnGeom with_chunks(BnGeom g, int chunks, int rows) { g.chunks = chunks; g.chunk_rows = rows; return g; }
// such chunks cover the R rows exactly: the last one holds at least one row
inline bool chunks_cover(int chunks, int chunk_rows, int64_t R) {
  return chunks > 0 && chunk_rows > 0 && (int64_t)chunks * chunk_rows >= R && (int64_t)(chunks - 1) * chunk_rows < R;
}

// The [chunks][C] planes of a workspace (four) or of a producer's chunk_stats (four forward, three backward).
// MODE 0: a = chunk mean, b = chunk M2, c = max, d = min.  MODE 1: a = sum dz, b = sum dz * (x - mean), c = max |dz|;
// no kernel takes d there, and spml_bn_bwd_hl8_f32 keeps the merged max_dz [C] in that quarter of the workspace.
template <typename T>
struct BnPlanes {
  T *a, *b, *c, *d;
  // the first n of them: what the kernels are handed by a call that has no use for the rest
  BnPlanes first(int n) const { return {a, b, n > 2 ? c : nullptr, n > 3 ? d : nullptr}; }
};
template <typename T>
inline BnPlanes<T> bn_planes(T* base, const BnGeom& g, int C) {
  const size_t n = (size_t)g.chunks * C;
  return {base, base + n, base + 2 * n, base + 3 * n};
}
inline size_t bn_ws_bytes(const BnGeom& g, int C) { return (size_t)4 * g.chunks * C * 4 + 256; }

// the kernel variant by where dz = dy * (y > 0) comes from (1 an fp32 y, 2 the mask bytes, 0 no ReLU): no test per row
inline int mask_kind(const float* y, const unsigned char* relu_mask) { return y ? 1 : (relu_mask ? 2 : 0); }
inline dim3 apply_grid(const BnGeom& g, int64_t R) {
  return dim3(g.col_blocks, (unsigned)((R + g.apply_rows - 1) / g.apply_rows));
}

struct PartialArgs {
  const float* x;
  const float *dy = nullptr, *mean = nullptr, *y = nullptr;      // MODE 1: dy, batch mean; y or the mask bytes if ReLU
  const unsigned char* relu_mask = nullptr;
  float* zero_me = nullptr;                                      // the bound slot the next merge max-reduces into
};
template <int MODE>
inline auto partial_kernel(int mask) {
  using K = decltype(&bn_partial<0, 0>);
  if (MODE == 0) return K(bn_partial<0, 0>);
  return select_int<0, 1, 2>(mask, K(nullptr), [](auto M_) -> K { return bn_partial<1, decltype(M_)::value>; });
}
template <int MODE>
inline void launch_partial(const BnGeom& g, hipStream_t s, int64_t R, int C, const PartialArgs& a, BnPlanes<float> p) {
  hipLaunchKernelGGL(partial_kernel<MODE>(mask_kind(a.y, a.relu_mask)), dim3(g.col_blocks, g.chunks), dim3(256), 0, s,
                     a.x, a.dy, a.y, a.mean, R, C, g.cq, g.chunk_rows, p.a, p.b, a.relu_mask, p.c, p.d, a.zero_me);
}

struct MergeArgs {
  float *out_a, *out_b;                  // MODE 0: mean, M2 (invstd where fin.fin);  MODE 1: sum dz, sum dz * xhat
  const float* invstd = nullptr;         // MODE 1
  float *out_c = nullptr, *out_d = nullptr;      // merged extremes of p.c / p.d: max and min of x, or max |dz| alone
  BnBound bound = {};
  BnFinal fin = {0, 0.f, 0.f, nullptr, nullptr};
};
template <int MODE, typename T>
inline void launch_merge(const BnGeom& g, hipStream_t s, int64_t R, int C, BnPlanes<T> p, const MergeArgs& a) {
  hipLaunchKernelGGL(bn_merge<MODE>, dim3((C + kMergeCh - 1) / kMergeCh), dim3(kMergeCh * kMergeLanes), 0, s, p.a, p.b,
                     R, C, g.chunks, g.chunk_rows, a.invstd, a.out_a, a.out_b, a.fin, p.c, p.d, a.out_c, a.out_d,
                     a.bound);
}

struct ApplyArgs {
  const float *x, *residual, *mean, *invstd, *gamma, *beta;      // residual may be null
  int relu;
  float *y = nullptr, *y_bound = nullptr;      // y_bound fixes the scale of y_hl8 (a single-rank merge writes it)
  uint2* y_hl8 = nullptr;
  unsigned char* relu_mask = nullptr;
};
inline auto apply_kernel(bool has_res) { return has_res ? bn_apply<true> : bn_apply<false>; }
inline void launch_apply(const BnGeom& g, hipStream_t s, int64_t R, int C, const ApplyArgs& a) {
  hipLaunchKernelGGL(apply_kernel(a.residual != nullptr), apply_grid(g, R), dim3(256), 0, s, a.x, a.residual, R, C,
                     g.cq, g.apply_rows, a.mean, a.invstd, a.gamma, a.beta, a.relu, a.y, a.y_hl8, a.y_bound,
                     a.relu_mask);
}

struct BwdApplyArgs {
  const float *dy, *y;                   // y or relu_mask or neither (mask_kind)
  const unsigned char* relu_mask;
  const float *x, *mean, *invstd, *gamma, *sum_dz, *sum_dz_xhat;      // read for dx / dx_hl8 only
  const float* count_dev;                // the row count of all ranks on the device, or null: 1 / count in inv_count
  float inv_count;
  float *dx, *d_residual;
  uint2* dx_hl8 = nullptr;               // with dx_bound, which fixes its scale (and which a single-rank merge writes)
  float* dx_bound = nullptr;
};
inline auto bwd_apply_kernel(int mask) {
  using K = decltype(&bn_bwd_apply<0>);
  return select_int<0, 1, 2>(mask, K(nullptr), [](auto M_) -> K { return bn_bwd_apply<decltype(M_)::value>; });
}
inline void launch_bwd_apply(const BnGeom& g, hipStream_t s, int64_t R, int C, const BwdApplyArgs& a) {
  hipLaunchKernelGGL(bwd_apply_kernel(mask_kind(a.y, a.relu_mask)), apply_grid(g, R), dim3(256), 0, s, a.dy, a.y, a.x,
                     R, C, g.cq, g.apply_rows, a.mean, a.invstd, a.gamma, a.sum_dz, a.sum_dz_xhat, a.inv_count,
                     a.count_dev, a.dx, a.d_residual, a.relu_mask, a.dx_hl8, a.dx_bound);
}

// statistics of x: the chunk partials into the planes p of the workspace, then their merge
inline void stats_pass(const BnGeom& g, hipStream_t s, const float* x, int64_t R, int C, BnPlanes<float> p,
                       const MergeArgs& m) {
  launch_partial<0>(g, s, R, C, {x}, p);
  launch_merge<0>(g, s, R, C, p, m);
}
// tail of the two single-rank hl8 forwards: merge with finalisation and the bound of y (reset with p), then the apply
template <typename T>
inline void merge_final_apply(const BnGeom& g, hipStream_t s, int64_t R, int C, BnPlanes<T> p, const BnFinal& fin,
                              const float* residual_bound, float* mean, float* invstd, float* cmax, float* cmin,
                              const ApplyArgs& ap) {
  const BnBound bound{ap.y_bound, ap.residual ? residual_bound : nullptr, ap.gamma, ap.beta};
  launch_merge<0>(g, s, R, C, p, {mean, invstd, nullptr, cmax, cmin, bound, fin});
  launch_apply(g, s, R, C, ap);
}
// tail of the two single-rank hl8 backwards: merge with the bound of dx (if dx_hl8), then the apply if it has an output
template <typename T>
inline void merge_bound_bwd_apply(const BnGeom& g, hipStream_t s, int64_t R, int C, BnPlanes<T> p, float* d_beta,
                                  float* d_gamma, float* max_dz, const float* cmax, const float* cmin,
                                  const BwdApplyArgs& ba) {
  const BnBound bound{ba.dx_hl8 ? ba.dx_bound : nullptr, nullptr, ba.gamma, nullptr, ba.mean, cmax, cmin, ba.inv_count};
  launch_merge<1>(g, s, R, C, p, {d_beta, d_gamma, ba.invstd, max_dz, nullptr, bound});
  if (!ba.dx && !ba.dx_hl8 && !ba.d_residual) return;
  launch_bwd_apply(g, s, R, C, ba);
}
// the pointers every forward entry point reads or writes with float4 accesses (absent outputs pass)
inline bool fwd_aligned(const float* x, const float* residual, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, const float* y, const void* y_hl8) {
  return al16(x) && (!y || al16(y)) && (!y_hl8 || al16(y_hl8)) && (!residual || al16(residual)) && al16(mean) &&
         al16(invstd) && al16(gamma) && al16(beta);
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_bn_workspace_bytes(int64_t R, int C) {
  return R <= 0 || C <= 0 ? 0 : bn_ws_bytes(bn_geom(R, C), C);
}

extern "C" int spml_bn_stats_f32(const float* x, int64_t R, int C, float* mean, float* m2, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (!x || !mean || !m2 || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  if ((C & 3) || !al16(x) || !al16(mean) || !al16(m2)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  stats_pass(g, (hipStream_t)stream, x, R, C, bn_planes(static_cast<float*>(ws), g, C).first(2), {mean, m2});
  return launch_status();
}

extern "C" int spml_bn_act_apply_f32(const float* x, const float* residual, int64_t R, int C, const float* mean,
                                     const float* invstd, const float* gamma, const float* beta, int relu, float* y,
                                     void* stream) {
  if (!x || !mean || !invstd || !gamma || !beta || !y || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  if ((C & 3) || !fwd_aligned(x, residual, mean, invstd, gamma, beta, y, nullptr)) return SPML_ERR_UNSUPPORTED;
  launch_apply(bn_geom(R, C), (hipStream_t)stream, R, C, {x, residual, mean, invstd, gamma, beta, relu, y});
  return launch_status();
}

extern "C" int spml_bn_act_bwd_reduce_f32(const float* dy, const float* y, const float* x, int64_t R, int C,
                                          const float* mean, const float* invstd, float* sum_dz, float* sum_dz_xhat,
                                          void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !x || !mean || !invstd || !sum_dz || !sum_dz_xhat || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  if ((C & 3) || !al16(dy) || !al16(x) || (y && !al16(y)) || !al16(mean)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  const BnPlanes<float> p = bn_planes(static_cast<float*>(ws), g, C).first(2);
  launch_partial<1>(g, (hipStream_t)stream, R, C, {x, dy, mean, y}, p);
  launch_merge<1>(g, (hipStream_t)stream, R, C, p, {sum_dz, sum_dz_xhat, invstd});
  return launch_status();
}

extern "C" int spml_bn_act_bwd_apply_f32(const float* dy, const float* y, const float* x, int64_t R, int C,
                                         const float* mean, const float* invstd, const float* gamma,
                                         const float* sum_dz, const float* sum_dz_xhat, double count,
                                         const float* count_dev, float* dx, float* d_residual, void* stream) {
  if (!dy || R <= 0 || C <= 0 || (!dx && !d_residual) || (count <= 0 && !count_dev)) return SPML_ERR_INVALID_ARG;
  if (dx && (!x || !mean || !invstd || !gamma || !sum_dz || !sum_dz_xhat)) return SPML_ERR_INVALID_ARG;
  if ((C & 3) || !al16(dy) || (y && !al16(y)) || (dx && !al16(dx)) || (d_residual && !al16(d_residual)))
    return SPML_ERR_UNSUPPORTED;
  launch_bwd_apply(bn_geom(R, C), (hipStream_t)stream, R, C,
                   {dy, y, nullptr, x, mean, invstd, gamma, sum_dz, sum_dz_xhat, count_dev,
                    count > 0 ? (float)(1.0 / count) : 0.f, dx, d_residual});
  return launch_status();
}

// Single-rank batch norm: the whole forward / backward in one call each (three launches, no
// framework ops in between).
extern "C" int spml_bn_act_fwd_f32(const float* x, const float* residual, int64_t R, int C, const float* gamma,
                                   const float* beta, float* running_mean, float* running_var, float momentum,
                                   float eps, int relu, float* y, float* mean, float* invstd, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (!x || !gamma || !beta || !y || !mean || !invstd || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  if ((C & 3) || !fwd_aligned(x, residual, mean, invstd, gamma, beta, y, nullptr)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  stats_pass(g, (hipStream_t)stream, x, R, C, bn_planes(static_cast<float*>(ws), g, C).first(2),
             {mean, invstd, nullptr, nullptr, nullptr, {}, BnFinal{1, eps, momentum, running_mean, running_var}});
  launch_apply(g, (hipStream_t)stream, R, C, {x, residual, mean, invstd, gamma, beta, relu, y});
  return launch_status();
}

extern "C" int spml_bn_act_bwd_f32(const float* dy, const float* y, const float* x, int64_t R, int C,
                                   const float* mean, const float* invstd, const float* gamma, float* d_gamma,
                                   float* d_beta, float* dx, float* d_residual, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!dy || !x || !mean || !invstd || !gamma || !d_gamma || !d_beta || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  int rc = spml_bn_act_bwd_reduce_f32(dy, y, x, R, C, mean, invstd, d_beta, d_gamma, ws, ws_bytes, stream);
  if (rc != SPML_OK) return rc;
  if (!dx && !d_residual) return SPML_OK;
  return spml_bn_act_bwd_apply_f32(dy, y, x, R, C, mean, invstd, gamma, d_beta, d_gamma, (double)R, nullptr, dx,
                                   d_residual, stream);
}

// ---- variants that also produce the split-f16 ("hl8") copies the matrix-core convolutions
// consume (csrc/conv.hip), with the tensor bounds that fix their scales -----------------------
extern "C" int spml_bn_stats_ext_f32(const float* x, int64_t R, int C, float* mean, float* m2, float* cmax,
                                     float* cmin, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !mean || !m2 || !cmax || !cmin || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  if ((C & 3) || !al16(x) || !al16(mean) || !al16(m2)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  stats_pass(g, (hipStream_t)stream, x, R, C, bn_planes(static_cast<float*>(ws), g, C),
             {mean, m2, nullptr, cmax, cmin});
  return launch_status();
}

// The same statistics pooled from the chunk statistics a convolution's epilogue left
// (spml_conv_hl8_stats_f32): one launch, x is not read.  Any C: only the chunk members of the geometry are used.
extern "C" int spml_bn_stats_ext_chunks_f32(const float* chunk_stats, int chunks, int chunk_rows, int64_t R, int C,
                                            float* mean, float* m2, float* cmax, float* cmin, void* stream) {
  if (!chunk_stats || !mean || !m2 || !cmax || !cmin || R <= 0 || C <= 0 || !chunks_cover(chunks, chunk_rows, R))
    return SPML_ERR_INVALID_ARG;
  const BnGeom g = with_chunks(BnGeom{}, chunks, chunk_rows);
  launch_merge<0>(g, (hipStream_t)stream, R, C, bn_planes(chunk_stats, g, C), {mean, m2, nullptr, cmax, cmin});
  return launch_status();
}

extern "C" int spml_bn_finalize_f32(const float* mean, const float* m2, int C, double count, float eps,
                                    float momentum, float* running_mean, float* running_var, float* invstd,
                                    void* stream) {
  if (!mean || !m2 || !invstd || C <= 0 || count <= 0) return SPML_ERR_INVALID_ARG;
  hipLaunchKernelGGL(bn_finalize, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, C, mean, m2,
                     (float)count, eps, momentum, running_mean, running_var, invstd);
  return launch_status();
}

extern "C" int spml_bn_act_apply_hl8_f32(const float* x, const float* residual, const float* residual_bound,
                                         int64_t R, int C, const float* mean, const float* invstd,
                                         const float* gamma, const float* beta, const float* cmax,
                                         const float* cmin, int relu, float* y, void* y_hl8, float* y_bound,
                                         unsigned char* relu_mask, void* stream) {
  if (!x || !mean || !invstd || !gamma || !beta || (!y && !y_hl8) || R <= 0 || C <= 0) return SPML_ERR_INVALID_ARG;
  if ((y_hl8 || y_bound) && (!cmax || !cmin || !y_bound || (residual && !residual_bound))) return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !fwd_aligned(x, residual, mean, invstd, gamma, beta, y, y_hl8)) return SPML_ERR_UNSUPPORTED;
  if (y_bound)
    hipLaunchKernelGGL(bn_bound_fwd, dim3(1), dim3(256), 0, (hipStream_t)stream, C, cmax, cmin, mean, invstd, gamma,
                       beta, residual ? residual_bound : (const float*)nullptr, y_bound);
  launch_apply(bn_geom(R, C), (hipStream_t)stream, R, C,
               {x, residual, mean, invstd, gamma, beta, relu, y, y_bound, static_cast<uint2*>(y_hl8), relu_mask});
  return launch_status();
}

extern "C" int spml_bn_act_bwd_reduce_ext_f32(const float* dy, const float* y, const unsigned char* relu_mask,
                                              const float* x, int64_t R, int C, const float* mean,
                                              const float* invstd, float* sum_dz, float* sum_dz_xhat, float* max_dz,
                                              void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !x || !mean || !invstd || !sum_dz || !sum_dz_xhat || !max_dz || R <= 0 || C <= 0)
    return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !al16(dy) || !al16(x) || (y && !al16(y)) || !al16(mean)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  const BnPlanes<float> p = bn_planes(static_cast<float*>(ws), g, C).first(3);
  launch_partial<1>(g, (hipStream_t)stream, R, C, {x, dy, mean, y, relu_mask}, p);
  launch_merge<1>(g, (hipStream_t)stream, R, C, p, {sum_dz, sum_dz_xhat, invstd, max_dz});
  return launch_status();
}

extern "C" int spml_bn_act_bwd_apply_hl8_f32(const float* dy, const float* y, const unsigned char* relu_mask,
                                             const float* x, int64_t R, int C, const float* mean,
                                             const float* invstd, const float* gamma, const float* sum_dz,
                                             const float* sum_dz_xhat, const float* max_dz, const float* cmax,
                                             const float* cmin, double count, const float* count_dev, float* dx,
                                             void* dx_hl8, float* dx_bound, float* d_residual, void* stream) {
  if (!dy || R <= 0 || C <= 0 || (!dx && !dx_hl8 && !d_residual) || (count <= 0 && !count_dev))
    return SPML_ERR_INVALID_ARG;
  const float inv_count = count > 0 ? (float)(1.0 / count) : 0.f;
  if ((dx || dx_hl8) && (!x || !mean || !invstd || !gamma || !sum_dz || !sum_dz_xhat)) return SPML_ERR_INVALID_ARG;
  if (dx_hl8 && (!max_dz || !cmax || !cmin || !dx_bound)) return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !al16(dy) || (y && !al16(y)) || (dx && !al16(dx)) || (dx_hl8 && !al16(dx_hl8)) ||
      (d_residual && !al16(d_residual)))
    return SPML_ERR_UNSUPPORTED;
  if (dx_hl8)
    hipLaunchKernelGGL(bn_bound_bwd, dim3(1), dim3(256), 0, (hipStream_t)stream, C, max_dz, cmax, cmin, mean, invstd,
                       gamma, sum_dz, sum_dz_xhat, inv_count, count_dev, dx_bound);
  launch_bwd_apply(bn_geom(R, C), (hipStream_t)stream, R, C,
                   {dy, y, relu_mask, x, mean, invstd, gamma, sum_dz, sum_dz_xhat, count_dev, inv_count, dx, d_residual,
                    static_cast<uint2*>(dx_hl8), dx_bound});
  return launch_status();
}

// Single-rank forms of the two halves: statistics + finalisation + bound + apply (three launches),
// reduction + bound + apply (three launches).
extern "C" int spml_bn_fwd_hl8_f32(const float* x, const float* residual, const float* residual_bound, int64_t R,
                                   int C, const float* gamma, const float* beta, float* running_mean,
                                   float* running_var, float momentum, float eps, int relu, float* y, void* y_hl8,
                                   float* y_bound, unsigned char* relu_mask, float* mean, float* invstd,
                                   float* cmax, float* cmin, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !gamma || !beta || (!y && !y_hl8) || !y_bound || !mean || !invstd || !cmax || !cmin || R <= 0 || C <= 0 ||
      (residual && !residual_bound))
    return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !fwd_aligned(x, residual, mean, invstd, gamma, beta, y, y_hl8)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  const BnPlanes<float> p = bn_planes(static_cast<float*>(ws), g, C);
  launch_partial<0>(g, (hipStream_t)stream, R, C, {x, nullptr, nullptr, nullptr, nullptr, y_bound}, p);
  merge_final_apply(g, (hipStream_t)stream, R, C, p, BnFinal{1, eps, momentum, running_mean, running_var},
                    residual_bound, mean, invstd, cmax, cmin,
                    {x, residual, mean, invstd, gamma, beta, relu, y, y_bound, static_cast<uint2*>(y_hl8), relu_mask});
  return launch_status();
}

// The same forward when the producer of x (a matrix-core convolution, spml_conv_hl8_stats_f32) has already
// left the chunk statistics [4][chunks][C] (mean, M2, max, min per chunk of chunk_rows rows) and reset
// *y_bound: two launches, x is read once.
extern "C" int spml_bn_fwd_hl8_chunks_f32(const float* x, const float* chunk_stats, int chunks, int chunk_rows,
                                          const float* residual, const float* residual_bound, int64_t R, int C,
                                          const float* gamma, const float* beta, float* running_mean,
                                          float* running_var, float momentum, float eps, int relu, float* y,
                                          void* y_hl8, float* y_bound, unsigned char* relu_mask, float* mean,
                                          float* invstd, float* cmax, float* cmin, void* stream) {
  if (!x || !chunk_stats || !gamma || !beta || (!y && !y_hl8) || !y_bound || !mean || !invstd || !cmax || !cmin ||
      R <= 0 || C <= 0 || !chunks_cover(chunks, chunk_rows, R) || (residual && !residual_bound))
    return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !fwd_aligned(x, residual, mean, invstd, gamma, beta, y, y_hl8)) return SPML_ERR_UNSUPPORTED;
  const BnGeom g = with_chunks(bn_geom(R, C), chunks, chunk_rows);
  merge_final_apply(g, (hipStream_t)stream, R, C, bn_planes(chunk_stats, g, C),
                    BnFinal{1, eps, momentum, running_mean, running_var}, residual_bound, mean, invstd, cmax, cmin,
                    {x, residual, mean, invstd, gamma, beta, relu, y, y_bound, static_cast<uint2*>(y_hl8), relu_mask});
  return launch_status();
}

extern "C" int spml_bn_bwd_hl8_f32(const float* dy, const float* y, const unsigned char* relu_mask, const float* x,
                                   int64_t R, int C, const float* mean, const float* invstd, const float* gamma,
                                   const float* cmax, const float* cmin, float* d_gamma, float* d_beta, float* dx,
                                   void* dx_hl8, float* dx_bound, float* d_residual, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!dy || !x || !mean || !invstd || !gamma || !cmax || !cmin || !d_gamma || !d_beta || R <= 0 || C <= 0 ||
      (dx_hl8 && !dx_bound))
    return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !al16(dy) || !al16(x) || (y && !al16(y)) || (dx && !al16(dx)) || (dx_hl8 && !al16(dx_hl8)) ||
      (d_residual && !al16(d_residual)) || !al16(mean))
    return SPML_ERR_UNSUPPORTED;
  const BnGeom g = bn_geom(R, C);
  if (!ws || ws_bytes < bn_ws_bytes(g, C)) return SPML_ERR_WORKSPACE;
  const BnPlanes<float> ws4 = bn_planes(static_cast<float*>(ws), g, C);
  float* max_dz = ws4.d;                       // the fourth quarter of the workspace is free here
  launch_partial<1>(g, (hipStream_t)stream, R, C, {x, dy, mean, y, relu_mask, dx_hl8 ? dx_bound : nullptr},
                    ws4.first(3));
  merge_bound_bwd_apply(g, (hipStream_t)stream, R, C, ws4.first(3), d_beta, d_gamma, max_dz, cmax, cmin,
                        {dy, y, relu_mask, x, mean, invstd, gamma, d_beta, d_gamma, nullptr, (float)(1.0 / (double)R),
                         dx, d_residual, static_cast<uint2*>(dx_hl8), dx_bound});
  return launch_status();
}

// The same backward when the producer of dy (a data-gradient convolution, spml_conv_hl8_bwd_stats_f32) has already
// left the chunk sums [3][chunks][C] (sum dz, sum dz * (x - mean), max |dz| per chunk of chunk_rows rows) and reset
// *dx_bound: two launches, dy / x / the mask are read once.  max_dz [C] is scratch + output.
extern "C" int spml_bn_bwd_hl8_chunks_f32(const float* dy, const unsigned char* relu_mask, const float* x,
                                          const float* chunk_stats, int chunks, int chunk_rows, int64_t R, int C,
                                          const float* mean, const float* invstd, const float* gamma,
                                          const float* cmax, const float* cmin, float* d_gamma, float* d_beta,
                                          float* max_dz, float* dx, void* dx_hl8, float* dx_bound, float* d_residual,
                                          void* stream) {
  if (!dy || !x || !chunk_stats || !mean || !invstd || !gamma || !cmax || !cmin || !d_gamma || !d_beta || !max_dz ||
      R <= 0 || C <= 0 || !chunks_cover(chunks, chunk_rows, R) || (dx_hl8 && !dx_bound))
    return SPML_ERR_INVALID_ARG;
  if ((C & 7) || !al16(dy) || !al16(x) || (dx && !al16(dx)) || (dx_hl8 && !al16(dx_hl8)) ||
      (d_residual && !al16(d_residual)) || !al16(mean))
    return SPML_ERR_UNSUPPORTED;
  const BnGeom g = with_chunks(bn_geom(R, C), chunks, chunk_rows);
  merge_bound_bwd_apply(g, (hipStream_t)stream, R, C, bn_planes(chunk_stats, g, C).first(3), d_beta, d_gamma, max_dz,
                        cmax, cmin, {dy, nullptr, relu_mask, x, mean, invstd, gamma, d_beta, d_gamma, nullptr,
                                     (float)(1.0 / (double)R), dx, d_residual, static_cast<uint2*>(dx_hl8), dx_bound});
  return launch_status();
}

// spml_bn_act_bwd_reduce_ext_f32 pooled from the same chunk sums instead of a pass over dy and x -- the local half
// of SyncBatchNorm's backward for the matrix-core units (the caller all-reduces the sums before the apply pass).
extern "C" int spml_bn_act_bwd_reduce_ext_chunks_f32(const float* chunk_stats, int chunks, int chunk_rows, int64_t R,
                                                     int C, const float* invstd, float* sum_dz, float* sum_dz_xhat,
                                                     float* max_dz, void* stream) {
  if (!chunk_stats || !invstd || !sum_dz || !sum_dz_xhat || !max_dz || R <= 0 || C <= 0 ||
      !chunks_cover(chunks, chunk_rows, R))
    return SPML_ERR_INVALID_ARG;
  const BnGeom g = with_chunks(BnGeom{}, chunks, chunk_rows);
  launch_merge<1>(g, (hipStream_t)stream, R, C, bn_planes(chunk_stats, g, C).first(3),
                  {sum_dz, sum_dz_xhat, invstd, max_dz});
  return launch_status();
}

extern "C" int spml_bn_finalize_ranks_f32(const float* stats, int world, int C, float eps, float momentum,
                                          float* running_mean, float* running_var, float* mean, float* invstd,
                                          float* total_count, void* stream) {
  if (!stats || !mean || !invstd || world < 1 || C <= 0) return SPML_ERR_INVALID_ARG;
  hipLaunchKernelGGL(bn_finalize_ranks, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, C, world, stats, eps,
                     momentum, running_mean, running_var, mean, invstd, total_count);
  return launch_status();
}
