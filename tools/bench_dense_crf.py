#!/usr/bin/env python3
"""Timing of the dense CRF refinement (spml/models/crf.py:23-41 as HIP kernels, csrc/dense_crf.hip) on one synthetic
image: 375 x 500 pixels, 21 classes, 10 iterations, the reference's default weights and standard deviations.

Prints one JSON line:
  * ms per image of `DenseCRF.refine` (prepare + inference; device events over whole calls);
  * ms of the prepare step alone (operands, both norms: one pass over all pixel pairs) and ms per mean-field iteration
    (the inference call at `--iters` iterations minus the same call at 0 iterations, divided by `--iters`);
  * the same mathematics as chunked framework ops on the device (`framework_dense_crf` below: per row block of pixels
    the squared distances, `exp`, and a `matmul` against n Q, for both kernels; fp32), ms per iteration over
    `--framework-iters` iterations, and the largest difference between the two results after those iterations;
  * the pair / exp / flop / byte model of one iteration from the shapes.
Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b)


def framework_dense_crf(image, prob, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std, block=2048):
  """The definition as torch ops on the device, fp32, row blocks of `block` pixels against all pixels."""
  c, h, w = prob.shape
  n = h * w
  dev = prob.device
  ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
  pos = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).float()
  rgb = image.reshape(n, 3).float()

  def rows(lo, hi, which):
    d_pos = torch.cdist(pos[lo:hi], pos).square_()
    if which == 1:
      return torch.exp_(d_pos.mul_(-1.0 / (2.0 * pos_xy_std ** 2)))
    d_rgb = torch.cdist(rgb[lo:hi], rgb).square_()
    return torch.exp_(d_pos.mul_(-1.0 / (2.0 * bi_xy_std ** 2)).add_(d_rgb, alpha=-1.0 / (2.0 * bi_rgb_std ** 2)))

  norms = []
  for which in (1, 2):
    total = torch.cat([rows(lo, min(lo + block, n), which).sum(1) for lo in range(0, n, block)])
    norms.append(torch.rsqrt(total + 1e-20))
  logp = torch.log(prob.clamp(1e-5, 1.0)).reshape(c, n)
  q = torch.softmax(logp, dim=0)
  for _ in range(iter_max):
    x = logp.clone()
    for which, weight, norm in ((1, pos_w, norms[0]), (2, bi_w, norms[1])):
      nq = (q * norm).t().contiguous()
      for lo in range(0, n, block):
        hi = min(lo + block, n)
        x[:, lo:hi] += weight * (norm[lo:hi] * torch.matmul(rows(lo, hi, which), nq).t())
    q = torch.softmax(x, dim=0)
  return q.reshape(c, h, w)


def model(h, w, ncls, radius):
  n = h * w
  cpad = 32 if ncls <= 32 else 64
  pairs = n * n
  return {'pairs': pairs, 'exp': pairs,
          'mfma_flop': pairs * 2 * (2 * 16 + 3 * cpad),       # two exponent MFMAs (k = 16) and three message MFMAs per k step
          'spatial_flop': 2 * n * ncls * 2 * (2 * radius + 1),
          # per wave of 32 pixels every tile of j is read again (L2): features 2 KiB + operands 128 * cpad bytes per tile
          'l2_bytes': (n // 32) * (n // 32) * (2048 + 128 * cpad),
          'hbm_bytes': n * ncls * 4 * 8 + n * cpad * 4 * 2}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--classes', type=int, default=21)
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--calls', type=int, default=3)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--framework-iters', type=int, default=1)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_dense_crf needs an MI355X (no CPU fallback)')
  from spml_amd.models.crf import DenseCRF
  dev = torch.device('cuda', 0)
  h, w = a.image
  params = dict(iter_max=a.iters, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
  g = torch.Generator().manual_seed(1)
  # a blocky synthetic image: 5 x 5 constant-colour regions +- 12 noise, logits that favour one class per region
  ry, rx = (torch.arange(h) * 5 // h).view(-1, 1), (torch.arange(w) * 5 // w).view(1, -1)
  region = ry * 5 + rx
  colours = torch.randint(30, 226, (25, 3), generator=g)
  image = (colours[region] + torch.randint(-12, 13, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8).to(dev)
  logits = torch.randn(a.classes, h, w, generator=g)
  logits.scatter_add_(0, torch.randint(0, a.classes, (25,), generator=g)[region][None], torch.full((1, h, w), 2.0))
  prob = torch.softmax(logits, dim=0).to(dev)
  crf = DenseCRF(**params)
  res = {'image': [h, w], 'classes': a.classes, 'iterations': a.iters, 'crf_path': crf.path_name(h, w, a.classes)}
  ws = crf.prepare(image, a.classes)
  for _ in range(a.warmup):
    crf.refine(image, prob)
  torch.cuda.synchronize()
  res['image_ms'] = spread([timed(lambda: crf.refine(image, prob)) for _ in range(a.calls)])
  res['prepare_ms'] = spread([timed(lambda: crf.prepare(image, a.classes)) for _ in range(a.calls)])
  full = [timed(lambda: crf.infer(ws, prob)) for _ in range(a.calls)]
  none = [timed(lambda: crf.infer(ws, prob, iter_max=0)) for _ in range(a.calls)]
  res['infer_ms'], res['infer_0_iterations_ms'] = spread(full), spread(none)
  res['iteration_ms'] = round((statistics.median(full) - statistics.median(none)) / max(a.iters, 1), 4)
  if a.framework_iters > 0:
    fw_params = dict(params, iter_max=a.framework_iters)
    framework_dense_crf(image, prob, **dict(fw_params, iter_max=0))            # warm-up of the allocator and the GEMM
    t_none = timed(lambda: framework_dense_crf(image, prob, **dict(fw_params, iter_max=0)))
    out = []
    t_full = timed(lambda: out.append(framework_dense_crf(image, prob, **fw_params)))
    hip = crf.infer(ws, prob, iter_max=a.framework_iters)[0]
    res['framework'] = {'iterations': a.framework_iters, 'norms_ms': round(t_none, 3),
                        'iteration_ms': round((t_full - t_none) / a.framework_iters, 3),
                        'max_abs_diff_to_hip': (out[0] - hip).abs().max().item()}
    res['framework_over_hip_per_iteration'] = round(res['framework']['iteration_ms'] / res['iteration_ms'], 2)
  radius = int(res['crf_path'].rsplit('_r', 1)[1])
  res['model_per_iteration'] = model(h, w, a.classes, radius)
  print(json.dumps(res))


if __name__ == '__main__':
  main()
