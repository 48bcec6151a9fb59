"""Float64 reference of the fused batch norm (spml_amd/csrc/bn_act.hip): plain torch arithmetic, no library
batch-norm call, on CPU or GPU tensors.  Everything is [R, C] (the rows of an NHWC tensor); inputs of any float type
are widened first.  tests/test_bn_act_ref.py keeps this file honest on the CPU, tests/test_bn_act_gpu.py holds the
kernels to it."""
import math

import torch

# (R, C) -> what the host functions of bn_act.hip make of it; tests/test_bn_act_ref.py recomputes every column from a
# restatement of bn_geom (the BnGeom record), tests/test_bn_act_gpu.py pins `chunks` through the library.
#   R, C, cq, column blocks, row lanes, chunk_rows, chunks, rows of the last chunk, apply_rows, rows of the last tile
GEOMETRY = (
    (2, 8, 4, 1, 64, 128, 1, 2, 64, 2),             # two of four quads live, R below the row lanes
    (129, 8, 4, 1, 64, 128, 2, 1, 64, 1),           # one-row last chunk (M2 = 0, mean = the row)
    (257, 24, 4, 2, 64, 128, 3, 1, 64, 1),          # second column block half dead
    (300, 40, 8, 2, 32, 128, 3, 44, 32, 12),        # cq 8, 2 of 8 quads live in block 1
    (300, 72, 16, 2, 16, 128, 3, 44, 16, 12),       # cq 16
    (300, 136, 32, 2, 8, 128, 3, 44, 8, 4),         # cq 32
    (133, 264, 64, 2, 4, 128, 2, 5, 4, 1),          # cq 64, 2 of 64 quads live in block 1
    (300, 256, 64, 1, 4, 128, 3, 44, 4, 0),         # exact blocks (contrast)
    (2603, 2048, 64, 8, 4, 128, 21, 43, 8, 3),      # apply_rows above the row lanes, ragged last tile
    (131200, 8, 4, 1, 64, 129, 1018, 7, 64, 0),     # chunk_rows > 128; all 16 register slots of bn_merge
)
SHAPES = tuple((g[0], g[1]) for g in GEOMETRY)
FP32_ONLY_SHAPES = ((9, 4), (130, 12))              # C & 3 only: one quad; an odd quad count
OUTLIER_SHAPE = (300, 40)                           # the shape that is also run with the outlier channel
OUTLIER_CHANNEL = 37                                # gamma = +1.5 there (make_inputs): in the dead-pair column block


def host_geometry(r, c):
  """bn_geom of bn_act.hip (cq, col_blocks, chunk_rows, chunks, apply_rows) restated -> one row of GEOMETRY."""
  q = c >> 2
  cq = 64 if q >= 64 else 32 if q >= 32 else 16 if q >= 16 else 8 if q >= 8 else 4
  col_blocks = (q + cq - 1) // cq
  nty = 256 // cq
  target = min(1024, max(1, 1024 // col_blocks))
  chunk_rows = max(128, (r + target - 1) // target)
  chunks = (r + chunk_rows - 1) // chunk_rows
  rows = (r * col_blocks + 4095) // 4096
  apply_rows = min(256, max(nty, (rows + nty - 1) // nty * nty))
  return (r, c, cq, col_blocks, nty, chunk_rows, chunks, r - (chunks - 1) * chunk_rows, apply_rows, r % apply_rows)


def make_inputs(r, c, outlier=False, constant=False, seed=None):
  """The inputs every batch-norm case uses (CPU fp32): x = randn * 1.7 + 0.3 with per-channel offsets, gamma in
  [0.5, 1.5] with a few negative entries, beta in [-0.3, 0.3], residual and dy from randn.
  outlier: channel OUTLIER_CHANNEL gets one row 12 sigma out and a dy that follows x there (8 * clamp(xhat, -1, 1)),
  so that sum dz*xhat / n is of order one and the third term of the backward bound dominates the whole tensor's bound.
  constant: x is one value per channel (M2 = 0)."""
  g = torch.Generator().manual_seed(r * 7919 + c if seed is None else seed)
  x = torch.randn(r, c, generator=g) * 1.7 + 0.3 + torch.randn(c, generator=g) * 2.0
  res = torch.randn(r, c, generator=g)
  dy = torch.randn(r, c, generator=g)
  gamma = torch.linspace(0.5, 1.5, c)
  gamma[1::5] *= -1.0
  beta = torch.linspace(-0.3, 0.3, c)
  if constant:
    x = (torch.randn(c, generator=g) * 2.0 + 0.3).expand(r, c).contiguous()
  if outlier:
    k = OUTLIER_CHANNEL
    assert c > k and r > 8 and gamma[k] > 0
    x[r // 3, k] += 12.0 * 1.7
    col = x[:, k].double()
    xhat = (col - col.mean()) / col.std(unbiased=False)
    dy[:, k] = (8.0 * xhat.clamp(-1.0, 1.0)).float()
    gamma[k] = 1.5
  return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta)


def forward(x, gamma, beta, eps, momentum=0.1, relu=True, residual=None, running_mean=None, running_var=None):
  """-> dict(mean, m2, invstd, cmax, cmin, y, running_mean, running_var); running var unbiased (R - 1, or 1 for R = 1)."""
  xd = x.double()
  r = xd.shape[0]
  mean = xd.sum(0) / r
  d = xd - mean
  m2 = (d * d).sum(0)
  invstd = 1.0 / torch.sqrt(m2 / r + eps)
  y = d * (invstd * gamma.double()) + beta.double()
  if residual is not None:
    y = y + residual.double()
  if relu:
    y = y.clamp_min(0.0)
  out = dict(mean=mean, m2=m2, invstd=invstd, cmax=xd.max(0).values, cmin=xd.min(0).values, y=y,
             running_mean=None, running_var=None)
  if running_mean is not None:
    out['running_mean'] = (1.0 - momentum) * running_mean.double() + momentum * mean
    out['running_var'] = (1.0 - momentum) * running_var.double() + momentum * m2 / (r - 1 if r > 1 else 1)
  return out


def backward(dy, x, mean, invstd, gamma, mask=None, count=None):
  """dz = dy where mask (bool [R, C]; None: everywhere) -> dict(dz, s0 = sum dz, s1 = sum dz * xhat, max_dz, dx,
  d_residual).  count: the rows the statistics were pooled over (default R)."""
  dz = dy.double()
  if mask is not None:
    dz = torch.where(mask, dz, torch.zeros_like(dz))
  n = float(dz.shape[0] if count is None else count)
  xhat = (x.double() - mean.double()) * invstd.double()
  s0 = dz.sum(0)
  s1 = (dz * xhat).sum(0)
  dx = gamma.double() * invstd.double() * (dz - s0 / n - xhat * (s1 / n))
  return dict(dz=dz, s0=s0, s1=s1, max_dz=dz.abs().max(0).values, dx=dx, d_residual=dz,
              abs0=dz.abs().sum(0), abs1=(dz * xhat).abs().sum(0))


def bound_fwd(mean, invstd, gamma, beta, cmax, cmin, residual_bound=0.0):
  """max_c max(|(cmax-mean)*gamma*invstd+beta|, |(cmin-mean)*gamma*invstd+beta|) + residual_bound, without slack."""
  mean, sc, b = mean.double(), gamma.double() * invstd.double(), beta.double()
  v = torch.maximum(((cmax.double() - mean) * sc + b).abs(), ((cmin.double() - mean) * sc + b).abs())
  return float(v.max()) + float(residual_bound)


def bound_bwd_terms(mean, invstd, gamma, cmax, cmin, s0, s1, max_dz, n):
  """Per channel |gamma*invstd| * (max|dz|, |sum dz|/n, max(|cmax-mean|,|cmin-mean|)*invstd * |sum dz xhat|/n)."""
  mean, is_ = mean.double(), invstd.double()
  xh = torch.maximum((cmax.double() - mean).abs(), (cmin.double() - mean).abs()) * is_
  gi = (gamma.double() * is_).abs()
  return gi * max_dz.double(), gi * s0.double().abs() / n, gi * xh * s1.double().abs() / n


def bound_bwd(mean, invstd, gamma, cmax, cmin, s0, s1, max_dz, n):
  """max_c |gamma*invstd| * (max|dz| + |sum dz|/n + max(|cmax-mean|,|cmin-mean|)*invstd * |sum dz xhat|/n)."""
  t = bound_bwd_terms(mean, invstd, gamma, cmax, cmin, s0, s1, max_dz, n)
  return float((t[0] + t[1] + t[2]).max())


def _blocks(t, chunk_rows):
  """[R, C] -> the full chunks as one [chunks - 1, chunk_rows, C] view (if any) and the last chunk [1, rest, C]."""
  r, c = t.shape
  full = (r - 1) // chunk_rows * chunk_rows
  return ([t[:full].view(full // chunk_rows, chunk_rows, c)] if full else []) + [t[full:].view(1, r - full, c)]


def chunk_stats_fwd(x, chunk_rows):
  """[4, chunks, C] = (mean, M2, max, min) of every chunk of chunk_rows rows (the last one may be shorter)."""
  parts = []
  for blk in _blocks(x.double(), chunk_rows):
    m = blk.sum(1) / blk.shape[1]
    d = blk - m.unsqueeze(1)
    parts.append(torch.stack([m, (d * d).sum(1), blk.max(1).values, blk.min(1).values]))
  return torch.cat(parts, 1)


def chunk_stats_bwd(dz, x, mean, chunk_rows):
  """[3, chunks, C] = (sum dz, sum dz * (x - mean), max |dz|) per chunk."""
  dz = dz.double()
  t = dz * (x.double() - mean.double())
  parts = []
  for a, b in zip(_blocks(dz, chunk_rows), _blocks(t, chunk_rows)):
    parts.append(torch.stack([a.sum(1), b.sum(1), a.abs().max(1).values]))
  return torch.cat(parts, 1)


def pool_chunk_stats_fwd(stats, r, chunk_rows):
  """Chan's pooling of chunk (mean, M2) and the extremes back to the whole tensor -> (mean, M2, max, min)."""
  st = stats.double()
  chunks = st.shape[1]
  n = torch.full((chunks, 1), float(chunk_rows), dtype=torch.float64, device=st.device)
  n[-1] = float(r - (chunks - 1) * chunk_rows)
  mean = (st[0] * n).sum(0) / r
  d = st[0] - mean
  return mean, (st[1] + d * d * n).sum(0), st[2].max(0).values, st[3].min(0).values


def pool_rank_stats(counts, means, m2s):
  """Chan's pooling of per-rank (count, mean, M2) [world, C] -> (total [C], mean, M2)."""
  n, mu, m2 = counts.double(), means.double(), m2s.double()
  total = n.sum(0)
  mean = (n * mu).sum(0) / total
  d = mu - mean
  return total, mean, (m2 + d * d * n).sum(0)


def pow2_scale(bound):
  """bn_pow2_scale: S = 2^(14 - e) for the smallest e with bound < 2^e; 1 for a bound that is not positive and finite."""
  bound = float(bound)
  if not bound > 0.0 or bound > 1e38:
    return 1.0
  e = 14 - math.frexp(bound)[1]
  return 2.0 ** max(-100, min(100, e))


def hl8_halves(hl8):
  """Hl8 -> float16 [rows, C / 8, 2 (h, l), 8] as stored: 16-byte units ((row * C/8 + c/8) * 2 + part)."""
  return hl8.data.view(torch.float16).view(hl8.rows, hl8.channels // 8, 2, 8)


def decode_hl8(hl8):
  """Hl8 -> float64 [rows, C]: (h + l) / S (include/spml_hip.h)."""
  halves = hl8_halves(hl8).double()
  return (halves[:, :, 0] + halves[:, :, 1]).reshape(hl8.rows, hl8.channels) / pow2_scale(hl8.bound.item())


def mask_bits(mask, rows, channels):
  """ReLU mask bytes [rows * C/4] (bit e of byte (row, q) = channel 4q + e) -> bool [rows, C]."""
  m = mask.view(rows, channels // 4, 1).to(torch.int32)
  shifts = torch.arange(4, dtype=torch.int32, device=mask.device).view(1, 1, 4)
  return ((m >> shifts) & 1).bool().reshape(rows, channels)
