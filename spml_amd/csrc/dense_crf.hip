// N12: fully connected CRF refinement, spml/models/crf.py:23-41 -- the exact mean-field filter that
// pydensecrf's permutohedral lattice approximates, over all N x N pixel pairs of one image.
//
//   U = -log(clip(probmap, 1e-5, 1))                     Q_0 = softmax_c(-U)
//   K1[i,j] = exp(-|p_i - p_j|^2 / (2 pos_xy_std^2))
//   K2[i,j] = exp(-|p_i - p_j|^2 / (2 bi_xy_std^2) - |I_i - I_j|^2 / (2 bi_rgb_std^2))          (i = j included)
//   n_m = 1 / sqrt(K_m 1 + 1e-20)                        M_m(Q)[c,i] = n_m[i] sum_j K_m[i,j] n_m[j] Q[c,j]
//   Q <- softmax_c(-U + pos_w M_1(Q) + bi_w M_2(Q))      iter_max times
//
// The bilateral message is the hot path: N^2 exponentials per iteration.  crf_pairs is flash-style without the online
// maximum (the exponent is never positive).  A wave owns 32 pixels i and walks every 32-pixel tile of j:
//
//   D_xy[j][i], D_rgb[j][i]   two 32x32x16 f16 MFMAs.  Centred coordinates (|x'|, |y'| <= 1024) and uint8 colours are
//                             integers that f16 holds exactly, |f|^2 enters as two 11-bit pieces, every product and
//                             every partial sum is an integer below 2^24: |f_i - f_j|^2 = |f_j|^2 + |f_i|^2 - 2 f_j.f_i
//                             is formed with no rounding (and is exactly 0 for i = j).
//   K = exp2(a D_xy + b D_rgb)  in registers (v_exp_f32), split into hi + lo / 2048 (common.hpp).
//   Y[c][i] += Qn^T[c][j] K[j][i]   the accumulator tile has j in its 16 registers and i on the lane, which is the B
//                             operand of the next MFMA as it stands (no LDS, no lane movement); Qn = n_2[j] Q[c,j] is
//                             kept as split-f16 A fragments in that k order by whoever wrote Q.  Three MFMAs per k step
//                             and 32 classes: hi.hi, hi.lo, lo.hi -- fp32-class.
//   epilogue                  n_2[i], bi_w, + log p + the spatial message, softmax over the classes of a pixel (16
//                             registers x 2 lane halves x CT), the next Q in fp32 and as the next operand, the arg-max.
//
// The norms K_2 1 come from the same loop with a row of ones as the A operand (kNorm).  The spatial kernel is separable,
// K1 = g(dx) g(dy): two 1-D passes over n_1 Q with the taps cut at R = ceil(6 pos_xy_std) (the dropped tail is below
// 4e-9 of the kernel's mass), and n_1 in closed form from the same taps.  No atomics anywhere; Q is double-buffered;
// every launch is ordered by the stream alone: a call is bit-reproducible.
//
// the random-walk pseudo labels (pseudo_softmaxrw_crf.py:172-187, pseudo_camrw_crf.py:166-181) hand the CRF a
// 1/8-resolution map up-sampled to the image.  crf_init_upsampled forms the up-sampled values in registers (the taps of
// bilinear.hpp, as upsample_argmax of pseudo_label.hip) and writes what crf_init writes, plus the labels before the CRF:
// the [ncls][h][w] map is never stored unless the caller asks for it.  Everything after the first launch is shared.
//
// the kNN label inference (inference_crf.py:237-254) hands the CRF the vote map of its segments: one segment
// id per pixel and one row of k retrieved labels per segment (m <= 144 rows with the largest k-means grid here).  The
// clip, the sum, the logarithm and the division of crf_init are constant over a segment, so crf_votes_table does them
// once per segment (votes as votes_table of knn_msc.hip forms them) and crf_init_votes is a gather of that segment's row
// plus the operand write: no logf and no division per pixel, and the [h w][k] labels, their one-hot and the vote map
// itself are never formed unless the caller asks for the map.
#include <math.h>
#include <stdio.h>

#include "bilinear.hpp"
#include "common.hpp"

namespace spml {
namespace {

constexpr int kMaxClasses = 64;
constexpr int kMaxSide = 2048;
constexpr int kBlock = 256;
constexpr int kTile = 32;
constexpr int kMaxRadius = 2047;
constexpr float kClipLo = 1e-5f;                  // unary_from_softmax's default clip
constexpr float kNormEps = 1e-20f;

struct CrfHeader {
  float a2, b2;       // -log2(e) / (2 bi_xy_std^2), -log2(e) / (2 bi_rgb_std^2)
  float pos_c;        // 1 / (2 pos_xy_std^2)
  int radius;         // taps of the separable spatial kernel on either side
};

inline int spatial_radius(float pos_xy_std) {
  const double r = ceil(6.0 * (double)pos_xy_std);
  return r < 1.0 ? 1 : r > (double)kMaxRadius ? kMaxRadius : (int)r;
}

struct Layout {
  int64_t n, npad, tiles;
  int cpad, ct;
  size_t hdr, faxy, fargb, fbxy, fbrgb, n1, n2, prepared_end;        // what prepare writes (independent of ncls)
  size_t logp, spatial, tmp, qa, qb, op0, op1, total;                // what inference uses
  size_t map_bytes, op_bytes;
};

inline bool make_layout(int h, int w, int ncls, Layout& l) {
  if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide || ncls < 1 || ncls > kMaxClasses) return false;
  l.n = (int64_t)h * w;
  l.tiles = (l.n + kTile - 1) / kTile;
  l.npad = l.tiles * kTile;
  l.cpad = ncls <= 32 ? 32 : 64;
  l.ct = l.cpad / 32;
  const size_t frag = align_up((size_t)l.tiles * 64 * 16, 256);
  const size_t vec = align_up((size_t)l.npad * sizeof(float), 256);
  l.map_bytes = (size_t)ncls * (size_t)l.n * sizeof(float);
  l.op_bytes = (size_t)l.npad * (size_t)l.cpad * 4;                  // hi + lo, 2 bytes each
  const size_t map = align_up(l.map_bytes, 256);
  size_t o = 0;
  l.hdr = o, o += 256;
  l.faxy = o, o += frag;
  l.fargb = o, o += frag;
  l.fbxy = o, o += frag;
  l.fbrgb = o, o += frag;
  l.n1 = o, o += vec;
  l.n2 = o, o += vec;
  l.prepared_end = o;
  l.logp = o, o += map;
  l.spatial = o, o += map;
  l.tmp = o, o += map;
  l.qa = o, o += map;
  l.qb = o, o += map;
  l.op0 = o, o += align_up(l.op_bytes, 256);
  l.op1 = o, o += align_up(l.op_bytes, 256);
  l.total = o;
  return true;
}

// Where Qn[c][j] sits in the operand image: [tile of j][k step s][class tile][hi | lo][lane][element], so that a wave reads
// one A fragment of 32 classes x 16 pixels with one 16-byte load per lane.  Element e of lane half hh is pixel
// 16 s + 8 (e >> 2) + 4 hh + (e & 3) of the tile: the row order of accumulator registers 8 s .. 8 s + 7.
__device__ __forceinline__ size_t operand_index(int64_t j, int c, int ct_count, int part) {
  const int64_t t = j >> 5;
  const int jj = (int)(j & 31), s = jj >> 4, m = jj & 15;
  const int e = ((m >> 3) << 2) | (m & 3), hh = (m >> 2) & 1;
  const int lane = (c & 31) + 32 * hh;
  return ((((size_t)(t * 2 + s) * ct_count + (c >> 5)) * 2 + part) * 64 + lane) * 8 + e;
}

__device__ __forceinline__ void store_operand(_Float16* op, int64_t j, int c, int ct_count, float v) {
  _Float16 hi, lo;
  split_f16(v, hi, lo);
  op[operand_index(j, c, ct_count, 0)] = hi;
  op[operand_index(j, c, ct_count, 1)] = lo;
}

// thread = padded pixel j: the A (pixel as a row of the pair tile) and B (pixel as a column) fragments of both exponent
// MFMAs; k slots 0..7 live in lanes 0..31, lanes 32..63 (k 8..15) are zero.  A padded pixel is all zeros.
//   xy : A = [x, y, nlo, nhi, 1, 2048, 0, 0]      B = [-2x, -2y, 1, 2048, nlo, nhi, 0, 0]      n = x^2 + y^2 <= 2^21
//   rgb: A = [r, g, b, nlo, nhi, 1, 2048, 0]      B = [-2r, -2g, -2b, 1, 2048, nlo, nhi, 0]    n <= 195075
// with n = nlo + 2048 nhi, nlo < 2048: A . B = |f_j|^2 + |f_i|^2 - 2 f_j . f_i.
__global__ __launch_bounds__(kBlock) void crf_features(const unsigned char* __restrict__ image, int h, int w, int64_t n,
                                                       int64_t npad, CrfHeader hdr, CrfHeader* __restrict__ hdr_out,
                                                       half8* __restrict__ faxy, half8* __restrict__ fargb,
                                                       half8* __restrict__ fbxy, half8* __restrict__ fbrgb) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j == 0) *hdr_out = hdr;
  if (j >= npad) return;
  half8 axy, argb, bxy, brgb;
#pragma unroll
  for (int e = 0; e < 8; ++e) axy[e] = argb[e] = bxy[e] = brgb[e] = (_Float16)0.f;
  const half8 zero = axy;
  if (j < n) {
    const int y = (int)(j / w) - (h >> 1), x = (int)(j % w) - (w >> 1);
    const int nxy = x * x + y * y;
    const int r = image[j * 3 + 0], g = image[j * 3 + 1], b = image[j * 3 + 2];
    const int nc = r * r + g * g + b * b;
    const _Float16 one = (_Float16)1.f, big = (_Float16)2048.f;
    axy[0] = (_Float16)(float)x, axy[1] = (_Float16)(float)y;
    axy[2] = (_Float16)(float)(nxy & 2047), axy[3] = (_Float16)(float)(nxy >> 11), axy[4] = one, axy[5] = big;
    bxy[0] = (_Float16)(float)(-2 * x), bxy[1] = (_Float16)(float)(-2 * y);
    bxy[2] = one, bxy[3] = big, bxy[4] = axy[2], bxy[5] = axy[3];
    argb[0] = (_Float16)(float)r, argb[1] = (_Float16)(float)g, argb[2] = (_Float16)(float)b;
    argb[3] = (_Float16)(float)(nc & 2047), argb[4] = (_Float16)(float)(nc >> 11), argb[5] = one, argb[6] = big;
    brgb[0] = (_Float16)(float)(-2 * r), brgb[1] = (_Float16)(float)(-2 * g), brgb[2] = (_Float16)(float)(-2 * b);
    brgb[3] = one, brgb[4] = big, brgb[5] = argb[3], brgb[6] = argb[4];
  }
  const size_t lo = (size_t)(j >> 5) * 64 + (size_t)(j & 31), hi = lo + 32;
  faxy[lo] = axy, fargb[lo] = argb, fbxy[lo] = bxy, fbrgb[lo] = brgb;
  faxy[hi] = zero, fargb[hi] = zero, fbxy[hi] = zero, fbrgb[hi] = zero;
}

__device__ __forceinline__ void spatial_taps(const CrfHeader* hdr, float* g) {
  const int radius = hdr->radius;
  const float c = hdr->pos_c;
  for (int d = threadIdx.x; d <= radius; d += kBlock) g[d] = expf(-(float)(d * d) * c);
  __syncthreads();
}

// n_1 = 1 / sqrt(K1 1 + 1e-20) with K1 1 = (sum of the taps inside the row) * (sum of the taps inside the column).
__global__ __launch_bounds__(kBlock) void crf_spatial_norm(const CrfHeader* __restrict__ hdr, int h, int w,
                                                           float* __restrict__ n1) {
  __shared__ float g[kMaxRadius + 1];
  spatial_taps(hdr, g);
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (int64_t)h * w) return;
  const int radius = hdr->radius, y = (int)(p / w), x = (int)(p % w);
  float sx = 0.f, sy = 0.f;
  for (int xx = max(0, x - radius); xx <= min(w - 1, x + radius); ++xx) sx += g[abs(x - xx)];
  for (int yy = max(0, y - radius); yy <= min(h - 1, y + radius); ++yy) sy += g[abs(y - yy)];
  n1[p] = 1.0f / sqrtf(sx * sy + kNormEps);
}

// thread = (c, y, x).  kVertical = false: out = sum_x' g(x - x') n_1[y,x'] q[c,y,x'];  true: out = pos_w n_1[y,x]
// sum_y' g(y - y') q[c,y',x] (q = the first pass).
template <bool kVertical>
__global__ __launch_bounds__(kBlock) void crf_spatial_pass(const CrfHeader* __restrict__ hdr, const float* __restrict__ q,
                                                           const float* __restrict__ n1, int ncls, int h, int w,
                                                           float pos_w, float* __restrict__ out) {
  __shared__ float g[kMaxRadius + 1];
  spatial_taps(hdr, g);
  const int64_t n = (int64_t)h * w;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n * ncls) return;
  const int64_t p = idx % n;
  const float* plane = q + (idx - p);
  const int radius = hdr->radius, y = (int)(p / w), x = (int)(p % w);
  float sum = 0.f;
  if (!kVertical) {
    const float* row = plane + (int64_t)y * w;
    const float* nrow = n1 + (int64_t)y * w;
    for (int xx = max(0, x - radius); xx <= min(w - 1, x + radius); ++xx) sum += g[abs(x - xx)] * (nrow[xx] * row[xx]);
    out[idx] = sum;
  } else {
    for (int yy = max(0, y - radius); yy <= min(h - 1, y + radius); ++yy) sum += g[abs(y - yy)] * plane[(int64_t)yy * w + x];
    out[idx] = pos_w * (n1[p] * sum);
  }
}

// thread = pixel: log of the clipped probabilities, Q_0 = clip(p) / sum_c clip(p) (= softmax(-U)) in fp32 and as the first
// operand, and -- when the call runs no iteration -- the labels.
__global__ __launch_bounds__(kBlock) void crf_init(const float* __restrict__ prob, int ncls, int64_t n, int ct_count,
                                                   const float* __restrict__ n2, float* __restrict__ logp,
                                                   float* __restrict__ q, _Float16* __restrict__ op,
                                                   int64_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int c = 0; c < ncls; ++c) sum += fminf(fmaxf(prob[(size_t)c * n + i], kClipLo), 1.0f);
  const float ni = n2[i];
  float best = 0.f;
  int best_c = 0;
  for (int c = 0; c < ncls; ++c) {
    const float p = fminf(fmaxf(prob[(size_t)c * n + i], kClipLo), 1.0f);
    const float v = p / sum;
    logp[(size_t)c * n + i] = logf(p);
    q[(size_t)c * n + i] = v;
    store_operand(op, i, c, ct_count, ni * v);
    if (c == 0 || v > best) best = v, best_c = c;
  }
  if (labels != nullptr) labels[i] = best_c;
}

// The values of classes c0 .. c0 + 7 at the pixel whose taps are `t`, blended from the low-resolution map (0 at and above
// ncls): the 32 loads are in flight before the first blend.
constexpr int kInitClasses = 8;

__device__ __forceinline__ void blend_classes(const float* __restrict__ low, size_t plane, const Taps4& t, int c0, int ncls,
                                              float (&v)[kInitClasses]) {
  float a[kInitClasses], b[kInitClasses], c[kInitClasses], d[kInitClasses];
#pragma unroll
  for (int j = 0; j < kInitClasses; ++j) {
    const float* base = low + (size_t)(c0 + j < ncls ? c0 + j : 0) * plane;
    a[j] = base[t.o00]; b[j] = base[t.o01]; c[j] = base[t.o10]; d[j] = base[t.o11];
  }
#pragma unroll
  for (int j = 0; j < kInitClasses; ++j) v[j] = c0 + j < ncls ? blend(t, a[j], b[j], c[j], d[j]) : 0.f;
}

// crf_init on a map that is up-sampled on the way in (pseudo_softmaxrw_crf.py:172-185): thread = pixel of the h x w
// image, `low` is [ncls][oh][ow].  The four taps are taken once (make_taps as upsample_argmax of pseudo_label.hip calls
// it) and every class value v = blend(...) is what F.interpolate(bilinear, align_corners = False) gives.  Every class is
// blended ONCE and kept in a register (32 CT values, every index a compile-time constant; chunks at and above ncls are
// skipped by a uniform branch): the compiler fuses the multiplies and adds of `blend` differently from one inlined copy
// to the next, so a value blended a second time need not have the bits of the first -- and the written prob_up, the
// sum, log p and Q_0 must all come from the same bits for the call to equal spml_dense_crf_infer_f32 on prob_up.  First
// loop: sum_c clip(v), the arg-max of the un-clipped v (strict '>', the first NaN wins: the label before the CRF, the
// rules of upsample_argmax) and, if asked for, v itself.  Second loop: log clip(v), Q_0, the operand, the labels of a
// call without iterations -- the operations of crf_init, in its order.
template <int CT>
__global__ __launch_bounds__(kBlock) void crf_init_upsampled(const float* __restrict__ low, int ncls, int oh, int ow, int h,
                                                             int w, float scale_h, float scale_w,
                                                             const float* __restrict__ n2, float* __restrict__ logp,
                                                             float* __restrict__ q, _Float16* __restrict__ op,
                                                             int64_t* __restrict__ labels,
                                                             int64_t* __restrict__ labels_before,
                                                             float* __restrict__ prob_up) {
  constexpr int kChunks = 32 * CT / kInitClasses;
  const int64_t n = (int64_t)h * w;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Taps4 t = make_taps((int)i, w, scale_h, scale_w, oh, ow, 0, ow, 1);
  const size_t plane = (size_t)oh * ow;
  float v[32 * CT];
  float sum = 0.f, top = 0.f;
  int top_c = 0;
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    if (k * kInitClasses < ncls) {                                  // (uniform)
      float u[kInitClasses];
      blend_classes(low, plane, t, k * kInitClasses, ncls, u);
#pragma unroll
      for (int j = 0; j < kInitClasses; ++j) {
        const int c = k * kInitClasses + j;
        v[c] = u[j];
        if (c < ncls) {
          sum += fminf(fmaxf(u[j], kClipLo), 1.0f);
          if (prob_up != nullptr) prob_up[(size_t)c * n + i] = u[j];
          if (c == 0 || u[j] > top || (u[j] != u[j] && top == top)) top = u[j], top_c = c;
        }
      }
    }
  }
  if (labels_before != nullptr) labels_before[i] = top_c;
  const float ni = n2[i];
  float best = 0.f;
  int best_c = 0;
#pragma unroll
  for (int c = 0; c < 32 * CT; ++c) {
    if (c < ncls) {
      const float p = fminf(fmaxf(v[c], kClipLo), 1.0f);
      const float qv = p / sum;
      logp[(size_t)c * n + i] = logf(p);
      q[(size_t)c * n + i] = qv;
      store_operand(op, i, c, CT, ni * qv);
      if (c == 0 || qv > best) best = qv, best_c = c;
    }
  }
  if (labels != nullptr) labels[i] = best_c;
}

// One row of the segment table of the kNN entry: [log p | Q_0 | v], `cpad` = 32 CT floats each (zeros from ncls on), then
// the label before the CRF and the arg-max of Q_0 as two ints and two ints of padding: a multiple of 16 bytes, so that a
// row is read as float4s.
constexpr int kMaxVoteSegments = 4096;                            // (the limit of spml_view_votes_accumulate_f32)

__host__ __device__ constexpr int votes_row_floats(int cpad) { return 3 * cpad + 4; }

// (as segment_of of knn_msc.hip: an id outside [0, m) is outside the contract; clamped, so nothing is read out of bounds)
__device__ __forceinline__ int clamped_segment(int64_t id, int m) {
  return id < 0 ? 0 : id >= (int64_t)m ? m - 1 : (int)id;
}

// block = one wave = segment s, lane = class c: what votes_table of knn_msc.hip followed by crf_init computes for every
// pixel of the segment.  The vote is votes_table's expression -- an exact count, divided once by (float)k; a label outside
// [0, ncls) matches no column -- then the operations of crf_init in its order: the clip, the sum in ascending class order
// (every lane walks the classes through __shfl, so every lane holds the same sum), log p, p / sum, and both arg-max rules:
// strict '>' on the votes (the lowest class of a tie, np.argmax: the label before the CRF) and crf_init's on Q_0.
__global__ __launch_bounds__(kWave) void crf_votes_table(const int64_t* __restrict__ topk, int k, int ncls, int cpad,
                                                         float* __restrict__ table) {
  const int s = blockIdx.x, c = threadIdx.x;
  const int64_t* row = topk + (size_t)s * k;
  int count = 0;
  for (int j = 0; j < k; ++j) count += row[j] == (int64_t)c;
  const float v = c < ncls ? (float)count / (float)k : 0.f;
  const float p = fminf(fmaxf(v, kClipLo), 1.0f);
  float sum = 0.f, top = 0.f;
  int top_c = 0;
  for (int cc = 0; cc < ncls; ++cc) {                               // (uniform: all 64 lanes take part in every __shfl)
    sum += __shfl(p, cc, kWave);
    const float u = __shfl(v, cc, kWave);
    if (cc == 0 || u > top) top = u, top_c = cc;
  }
  const float qv = p / sum;
  float best = 0.f;
  int best_c = 0;
  for (int cc = 0; cc < ncls; ++cc) {
    const float u = __shfl(qv, cc, kWave);
    if (cc == 0 || u > best) best = u, best_c = cc;
  }
  float* out = table + (size_t)s * votes_row_floats(cpad);
  if (c < cpad) {
    out[c] = c < ncls ? logf(p) : 0.f;
    out[cpad + c] = c < ncls ? qv : 0.f;
    out[2 * cpad + c] = v;
  }
  if (c < 4) reinterpret_cast<int*>(out + 3 * cpad)[c] = c == 0 ? top_c : c == 1 ? best_c : 0;
}

// crf_init on the vote map of the kNN inference (inference_crf.py:240-245), which is never formed: thread = pixel i, one
// segment id (read once, clamped) and that segment's row of crf_votes_table as float4s -- eight classes (four loads) in
// flight at a time, chunks at and above ncls skipped by a uniform branch, every index into a register array a
// compile-time constant.  The lanes of a wave hold one or two distinct ids nearly everywhere, so a row load touches one
// or two lines; the stores are those of crf_init, coalesced over the pixels.
template <int CT>
__global__ __launch_bounds__(kBlock) void crf_init_votes(const int64_t* __restrict__ clu, const float* __restrict__ table,
                                                         int m, int ncls, int64_t n, const float* __restrict__ n2,
                                                         float* __restrict__ logp, float* __restrict__ q,
                                                         _Float16* __restrict__ op, int64_t* __restrict__ labels,
                                                         int64_t* __restrict__ labels_before, float* __restrict__ prob) {
  constexpr int kCpad = 32 * CT, kQuads = kCpad / 4;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int s = clamped_segment(clu[i], m);
  const float* row = table + (size_t)s * votes_row_floats(kCpad);
  const float4v* row4 = reinterpret_cast<const float4v*>(row);
  const float ni = n2[i];
#pragma unroll
  for (int g = 0; g < kQuads; g += 2) {
    if (4 * g < ncls) {                                             // (uniform)
      float4v lp[2], q0[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) lp[e] = row4[g + e], q0[e] = row4[kQuads + g + e];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = 4 * g + j;
        if (c < ncls) {
          logp[(size_t)c * n + i] = lp[j / 4][j % 4];
          q[(size_t)c * n + i] = q0[j / 4][j % 4];
          store_operand(op, i, c, CT, ni * q0[j / 4][j % 4]);
        }
      }
      if (prob != nullptr) {                                        // (uniform)
        float4v v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) v[e] = row4[2 * kQuads + g + e];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (4 * g + j < ncls) prob[(size_t)(4 * g + j) * n + i] = v[j / 4][j % 4];
      }
    }
  }
  const int* lab = reinterpret_cast<const int*>(row + 3 * kCpad);
  if (labels_before != nullptr) labels_before[i] = lab[0];
  if (labels != nullptr) labels[i] = lab[1];
}

// wave = 32 pixels i (the columns of every pair tile), all tiles of j.  kNorm: the A operand is a row of ones over the
// valid j, the result K_2 1 becomes n_2.  Otherwise the mean-field update of the wave's pixels (see the head of the file).
template <int CT, bool kNorm>
__global__ __launch_bounds__(kBlock) void crf_pairs(const CrfHeader* __restrict__ hdr, const half8* __restrict__ faxy,
                                                    const half8* __restrict__ fargb, const half8* __restrict__ fbxy,
                                                    const half8* __restrict__ fbrgb, const half8* __restrict__ op,
                                                    int64_t n, int tiles, int ncls, const float* __restrict__ logp,
                                                    const float* __restrict__ spatial, const float* __restrict__ n2,
                                                    float bi_w, float* __restrict__ q_next,
                                                    _Float16* __restrict__ op_next, int64_t* __restrict__ labels,
                                                    float* __restrict__ norm_out) {
  const int lane = threadIdx.x & 63;
  const int it = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (it >= tiles) return;                                         // (wave-uniform; the kernel has no barrier)
  const float a2 = hdr->a2, b2 = hdr->b2;
  const half8 bxy = fbxy[(size_t)it * 64 + lane], brgb = fbrgb[(size_t)it * 64 + lane];
  float16v acc0[CT], acc1[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[ct][r] = 0.f, acc1[ct][r] = 0.f;
  float16v zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

  for (int jt = 0; jt < tiles; ++jt) {
    const half8 axy = faxy[(size_t)jt * 64 + lane], argb = fargb[(size_t)jt * 64 + lane];
    half8 qh[2][CT], ql[2][CT];
    if (!kNorm) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const size_t f = (((size_t)jt * 2 + s) * CT + ct) * 2 * 64 + lane;
          qh[s][ct] = op[f];
          ql[s][ct] = op[f + 64];
        }
    }
    const float16v dxy = mfma32(axy, bxy, zero16);
    const float16v drgb = mfma32(argb, brgb, zero16);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      half8 kh, kl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = 8 * s + e;
        const float k = __builtin_amdgcn_exp2f(fmaf(b2, drgb[r], a2 * dxy[r]));
        _Float16 hi, lo;
        split_f16(k, hi, lo);
        kh[e] = hi, kl[e] = lo;
      }
      if (kNorm) {
        // ones[c = 0][j] for the valid j of this k step, in the operand's k order (operand_index)
        half8 ones;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int64_t j = (int64_t)jt * 32 + 16 * s + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
          ones[e] = ((lane & 31) == 0 && j < n) ? (_Float16)1.f : (_Float16)0.f;
        }
        acc0[0] = mfma32(ones, kh, acc0[0]);
        acc1[0] = mfma32(ones, kl, acc1[0]);
      } else {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          acc0[ct] = mfma32(qh[s][ct], kh, acc0[ct]);
          acc1[ct] = mfma32(qh[s][ct], kl, acc1[ct]);
          acc1[ct] = mfma32(ql[s][ct], kh, acc1[ct]);
        }
      }
    }
  }

  const int col = lane & 31, hh = lane >> 5;
  const int64_t i = (int64_t)it * 32 + col;
  const bool valid = i < n;
  if (kNorm) {
    // row c = 0 of the result: register 0 of lanes 0..31
    if (hh == 0 && valid) norm_out[i] = 1.0f / sqrtf((acc0[0][0] + acc1[0][0] * kSplitInv) + kNormEps);
    return;
  }
  const int64_t ir = valid ? i : n - 1;                            // (a padded column computes a copy of the last pixel)
  const float ni = n2[ir];
  float v[CT][16];
  float mx = -INFINITY;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * hh;
      float x = -INFINITY;
      if (c < ncls) {
        const float m = acc0[ct][r] + acc1[ct][r] * kSplitInv;
        x = (logp[(size_t)c * n + ir] + spatial[(size_t)c * n + ir]) + bi_w * (ni * m);
      }
      v[ct][r] = x;
      mx = fmaxf(mx, x);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
  float sum = 0.f;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * hh;
      const float e = c < ncls ? expf(v[ct][r] - mx) : 0.f;
      v[ct][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, kWave);
  float best = -1.f;
  int best_c = 0;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * hh;         // (ascending in (ct, r) for a lane)
      if (c < ncls) {
        const float qv = v[ct][r] / sum;
        if (valid) {
          q_next[(size_t)c * n + i] = qv;
          store_operand(op_next, i, c, CT, ni * qv);
        }
        if (qv > best) best = qv, best_c = c;
      }
    }
  if (labels != nullptr) {                                          // (uniform)
    const float other = __shfl_xor(best, 32, kWave);
    const int other_c = __shfl_xor(best_c, 32, kWave);
    if (other > best || (other == best && other_c < best_c)) best_c = other_c;
    if (hh == 0 && valid) labels[i] = best_c;
  }
}

inline bool good_std(float s) { return isfinite(s) && s > 0.f; }

// bytes of the segment table, 0 outside the limits
inline size_t votes_table_bytes(int m, int ncls) {
  if (m < 1 || m > kMaxVoteSegments || ncls < 1 || ncls > kMaxClasses) return 0;
  return (size_t)m * votes_row_floats(ncls <= 32 ? 32 : 64) * sizeof(float);
}

// (a null pointer overlaps nothing)
inline bool overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p != nullptr && q != nullptr && p0 < q0 + qn && q0 < p0 + pn;
}

}  // namespace
}  // namespace spml

using namespace spml;

extern "C" size_t spml_dense_crf_workspace_bytes(int h, int w, int ncls) {
  Layout l;
  return make_layout(h, w, ncls, l) ? l.total : 0;
}

extern "C" const char* spml_dense_crf_path_name(int h, int w, int ncls, float pos_xy_std) {
  static thread_local char name[64];
  Layout l;
  if (!make_layout(h, w, ncls, l) || !good_std(pos_xy_std)) return "unsupported";
  snprintf(name, sizeof(name), "pairs_mfma_f16x2_c%d+separable_r%d", l.cpad, spatial_radius(pos_xy_std));
  return name;
}

extern "C" int spml_dense_crf_prepare_u8(const unsigned char* image, int h, int w, float pos_xy_std, float bi_xy_std,
                                         float bi_rgb_std, void* ws, size_t ws_bytes, void* stream) {
  if (!image || h < 1 || w < 1 || !good_std(pos_xy_std) || !good_std(bi_xy_std) || !good_std(bi_rgb_std))
    return SPML_ERR_INVALID_ARG;
  Layout l;
  if (!make_layout(h, w, 1, l)) return SPML_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < l.prepared_end || ((uintptr_t)ws & 255) != 0) return SPML_ERR_WORKSPACE;
  char* base = static_cast<char*>(ws);
  CrfHeader hdr;
  const double log2e = 1.4426950408889634;
  hdr.a2 = (float)(-log2e / (2.0 * (double)bi_xy_std * (double)bi_xy_std));
  hdr.b2 = (float)(-log2e / (2.0 * (double)bi_rgb_std * (double)bi_rgb_std));
  hdr.pos_c = (float)(1.0 / (2.0 * (double)pos_xy_std * (double)pos_xy_std));
  hdr.radius = spatial_radius(pos_xy_std);
  hipStream_t s = (hipStream_t)stream;
  CrfHeader* dhdr = reinterpret_cast<CrfHeader*>(base + l.hdr);
  half8* faxy = reinterpret_cast<half8*>(base + l.faxy);
  half8* fargb = reinterpret_cast<half8*>(base + l.fargb);
  half8* fbxy = reinterpret_cast<half8*>(base + l.fbxy);
  half8* fbrgb = reinterpret_cast<half8*>(base + l.fbrgb);
  float* n1 = reinterpret_cast<float*>(base + l.n1);
  float* n2 = reinterpret_cast<float*>(base + l.n2);
  const unsigned px_blocks = (unsigned)((l.npad + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(crf_features, dim3(px_blocks), dim3(kBlock), 0, s, image, h, w, l.n, l.npad, hdr, dhdr, faxy, fargb,
                     fbxy, fbrgb);
  hipLaunchKernelGGL(crf_spatial_norm, dim3(px_blocks), dim3(kBlock), 0, s, dhdr, h, w, n1);
  const unsigned wave_blocks = (unsigned)((l.tiles + kBlock / kWave - 1) / (kBlock / kWave));
  hipLaunchKernelGGL((crf_pairs<1, true>), dim3(wave_blocks), dim3(kBlock), 0, s, dhdr, faxy, fargb, fbxy, fbrgb,
                     (const half8*)nullptr, l.n, (int)l.tiles, 1, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, 0.f, (float*)nullptr, (_Float16*)nullptr, (int64_t*)nullptr, n2);
  return launch_status();
}

// What both inference entry points check alike, in the order of the status codes; fills the layout.
static int infer_status(const void* map, int ncls, int h, int w, int iter_max, float pos_w, float bi_w, const float* q,
                 const int64_t* labels, const void* ws, size_t ws_bytes, Layout& l) {
  if (!map || !q || ncls < 1 || h < 1 || w < 1 || iter_max < 0 || !isfinite(pos_w) || !isfinite(bi_w) ||
      ((uintptr_t)map & 3) != 0 || ((uintptr_t)q & 3) != 0 || ((uintptr_t)labels & 7) != 0)
    return SPML_ERR_INVALID_ARG;
  if (!make_layout(h, w, ncls, l)) return SPML_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < l.total || ((uintptr_t)ws & 255) != 0) return SPML_ERR_WORKSPACE;
  return SPML_OK;
}

// The mean-field call around its first launch: the operand images are cleared, `launch_init(n2, logp, q0, op0, labels0)`
// writes log p, Q_0, the first operand and -- when the call runs no iteration -- the labels (crf_init or
// crf_init_upsampled, the one thing the two entry points differ in), then iter_max times the two spatial passes and the
// pair kernel; the last iteration writes the caller's q and labels.
template <typename Init>
static int mean_field(const Layout& l, char* base, int ncls, int h, int w, int iter_max, float pos_w, float bi_w, float* q,
               int64_t* labels, hipStream_t s, Init launch_init) {
  const CrfHeader* dhdr = reinterpret_cast<const CrfHeader*>(base + l.hdr);
  const half8* faxy = reinterpret_cast<const half8*>(base + l.faxy);
  const half8* fargb = reinterpret_cast<const half8*>(base + l.fargb);
  const half8* fbxy = reinterpret_cast<const half8*>(base + l.fbxy);
  const half8* fbrgb = reinterpret_cast<const half8*>(base + l.fbrgb);
  const float* n1 = reinterpret_cast<const float*>(base + l.n1);
  const float* n2 = reinterpret_cast<const float*>(base + l.n2);
  float* logp = reinterpret_cast<float*>(base + l.logp);
  float* spatial = reinterpret_cast<float*>(base + l.spatial);
  float* tmp = reinterpret_cast<float*>(base + l.tmp);
  float* qbuf[2] = {reinterpret_cast<float*>(base + l.qa), reinterpret_cast<float*>(base + l.qb)};
  _Float16* opbuf[2] = {reinterpret_cast<_Float16*>(base + l.op0), reinterpret_cast<_Float16*>(base + l.op1)};
  // the padded pixels and classes of both operand images stay zero: they contribute nothing to any message
  if (hipMemsetAsync(base + l.op0, 0, l.total - l.op0, s) != hipSuccess) return SPML_ERR_LAUNCH;
  const unsigned map_blocks = (unsigned)((l.n * ncls + kBlock - 1) / kBlock);
  const unsigned wave_blocks = (unsigned)((l.tiles + kBlock / kWave - 1) / (kBlock / kWave));
  launch_init(n2, logp, iter_max == 0 ? q : qbuf[0], opbuf[0], iter_max == 0 ? labels : (int64_t*)nullptr);
  for (int t = 0; t < iter_max; ++t) {
    const bool last = t + 1 == iter_max;
    const float* q_cur = qbuf[t & 1];
    float* q_out = last ? q : qbuf[(t + 1) & 1];
    int64_t* lab = last ? labels : (int64_t*)nullptr;
    hipLaunchKernelGGL((crf_spatial_pass<false>), dim3(map_blocks), dim3(kBlock), 0, s, dhdr, q_cur, n1, ncls, h, w, pos_w,
                       tmp);
    hipLaunchKernelGGL((crf_spatial_pass<true>), dim3(map_blocks), dim3(kBlock), 0, s, dhdr, (const float*)tmp, n1, ncls,
                       h, w, pos_w, spatial);
    const half8* op = reinterpret_cast<const half8*>(opbuf[t & 1]);
    _Float16* op_next = opbuf[(t + 1) & 1];
    if (l.ct == 1)
      hipLaunchKernelGGL((crf_pairs<1, false>), dim3(wave_blocks), dim3(kBlock), 0, s, dhdr, faxy, fargb, fbxy, fbrgb, op,
                         l.n, (int)l.tiles, ncls, (const float*)logp, (const float*)spatial, n2, bi_w, q_out, op_next, lab,
                         (float*)nullptr);
    else
      hipLaunchKernelGGL((crf_pairs<2, false>), dim3(wave_blocks), dim3(kBlock), 0, s, dhdr, faxy, fargb, fbxy, fbrgb, op,
                         l.n, (int)l.tiles, ncls, (const float*)logp, (const float*)spatial, n2, bi_w, q_out, op_next, lab,
                         (float*)nullptr);
  }
  return launch_status();
}

extern "C" int spml_dense_crf_infer_f32(const float* probmap, int ncls, int h, int w, int iter_max, float pos_w,
                                        float bi_w, float* q, int64_t* labels, void* ws, size_t ws_bytes,
                                        void* stream) {
  Layout l;
  const int status = infer_status(probmap, ncls, h, w, iter_max, pos_w, bi_w, q, labels, ws, ws_bytes, l);
  if (status != SPML_OK) return status;
  hipStream_t s = (hipStream_t)stream;
  const unsigned px_blocks = (unsigned)((l.n + kBlock - 1) / kBlock);
  return mean_field(l, static_cast<char*>(ws), ncls, h, w, iter_max, pos_w, bi_w, q, labels, s,
                    [&](const float* n2, float* logp, float* q0, _Float16* op0, int64_t* labels0) {
                      hipLaunchKernelGGL(crf_init, dim3(px_blocks), dim3(kBlock), 0, s, probmap, ncls, l.n, l.ct, n2, logp,
                                         q0, op0, labels0);
                    });
}

extern "C" int spml_dense_crf_infer_upsampled_f32(const float* lowres, int ncls, int oh, int ow, int h, int w,
                                                  int iter_max, float pos_w, float bi_w, float* q, int64_t* labels,
                                                  int64_t* labels_before, float* prob_up, void* ws, size_t ws_bytes,
                                                  void* stream) {
  if (oh < 1 || ow < 1 || ((uintptr_t)labels_before & 7) != 0 || ((uintptr_t)prob_up & 3) != 0)
    return SPML_ERR_INVALID_ARG;
  Layout l;
  const int status = infer_status(lowres, ncls, h, w, iter_max, pos_w, bi_w, q, labels, ws, ws_bytes, l);
  if (status != SPML_OK) return status;
  if ((int64_t)oh * ow > (1 << 24)) return SPML_ERR_UNSUPPORTED;       // (the limit of spml_upsample_argmax_i64)
  hipStream_t s = (hipStream_t)stream;
  const unsigned px_blocks = (unsigned)((l.n + kBlock - 1) / kBlock);
  // the scale expressions of spml_upsample_argmax_i64: the same taps, the same blended values, the same labels
  const float scale_h = (float)oh / (float)h, scale_w = (float)ow / (float)w;
  return mean_field(l, static_cast<char*>(ws), ncls, h, w, iter_max, pos_w, bi_w, q, labels, s,
                    [&](const float* n2, float* logp, float* q0, _Float16* op0, int64_t* labels0) {
                      if (l.ct == 1)
                        hipLaunchKernelGGL(crf_init_upsampled<1>, dim3(px_blocks), dim3(kBlock), 0, s, lowres, ncls, oh, ow,
                                           h, w, scale_h, scale_w, n2, logp, q0, op0, labels0, labels_before, prob_up);
                      else
                        hipLaunchKernelGGL(crf_init_upsampled<2>, dim3(px_blocks), dim3(kBlock), 0, s, lowres, ncls, oh, ow,
                                           h, w, scale_h, scale_w, n2, logp, q0, op0, labels0, labels_before, prob_up);
                    });
}

extern "C" size_t spml_dense_crf_votes_workspace_bytes(int m, int ncls) { return votes_table_bytes(m, ncls); }

extern "C" int spml_dense_crf_infer_votes_f32(const int64_t* clu, const int64_t* topk, int m, int k, int ncls, int h,
                                              int w, int iter_max, float pos_w, float bi_w, float* q, int64_t* labels,
                                              int64_t* labels_before, float* prob, void* table_ws,
                                              size_t table_ws_bytes, void* ws, size_t ws_bytes, void* stream) {
  if (!topk || m < 1 || k < 1 || ((uintptr_t)clu & 7) != 0 || ((uintptr_t)topk & 7) != 0 ||
      ((uintptr_t)labels_before & 7) != 0 || ((uintptr_t)prob & 3) != 0)
    return SPML_ERR_INVALID_ARG;
  Layout l;
  const int status = infer_status(clu, ncls, h, w, iter_max, pos_w, bi_w, q, labels, ws, ws_bytes, l);
  if (status != SPML_OK) return status;
  if (m > kMaxVoteSegments) return SPML_ERR_UNSUPPORTED;
  const size_t need = votes_table_bytes(m, ncls);
  if (!table_ws || table_ws_bytes < need || ((uintptr_t)table_ws & 15) != 0) return SPML_ERR_WORKSPACE;
  // the table is written before anything reads it: it may alias no input, no output and not the CRF's workspace
  const size_t px = (size_t)l.n * sizeof(int64_t);
  if (overlap(table_ws, need, clu, px) || overlap(table_ws, need, topk, (size_t)m * k * sizeof(int64_t)) ||
      overlap(table_ws, need, q, l.map_bytes) || overlap(table_ws, need, labels, px) ||
      overlap(table_ws, need, labels_before, px) || overlap(table_ws, need, prob, l.map_bytes) ||
      overlap(table_ws, need, ws, l.total))
    return SPML_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* table = static_cast<float*>(table_ws);
  hipLaunchKernelGGL(crf_votes_table, dim3((unsigned)m), dim3(kWave), 0, s, topk, k, ncls, l.cpad, table);
  const unsigned px_blocks = (unsigned)((l.n + kBlock - 1) / kBlock);
  return mean_field(l, static_cast<char*>(ws), ncls, h, w, iter_max, pos_w, bi_w, q, labels, s,
                    [&](const float* n2, float* logp, float* q0, _Float16* op0, int64_t* labels0) {
                      if (l.ct == 1)
                        hipLaunchKernelGGL(crf_init_votes<1>, dim3(px_blocks), dim3(kBlock), 0, s, clu,
                                           (const float*)table, m, ncls, l.n, n2, logp, q0, op0, labels0, labels_before,
                                           prob);
                      else
                        hipLaunchKernelGGL(crf_init_votes<2>, dim3(px_blocks), dim3(kBlock), 0, s, clu,
                                           (const float*)table, m, ncls, l.n, n2, logp, q0, op0, labels0, labels_before,
                                           prob);
                    });
}
