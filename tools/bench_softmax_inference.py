#!/usr/bin/env python3
"""Timing of the full-resolution softmax label inference (pyscripts/inference/inference_softmax.py:105-148) on one
synthetic image: sliding-window ResNet-101 DeepLab-v2 embedding at input resolution, the classifier head on every
crop, summed logits, arg-max.

Prints one JSON line: ms per image (device events over whole images), and per crop the time of
  (a) the HIP head (x / |x| -> split-f16, folded 3x3 convolution on the matrix cores, 1x1 head accumulated into the
      canvas) and
  (b) the framework ops of the documented fallback (`_logits` + slice `+=`)
on identical inputs, alternated in the same process, each followed once per round by its arg-max
(`spml_argmax_channels_i64` / `torch.argmax`).  Needs an MI355X: there is no fallback.
`--head-only` skips the backbone (for a kernel trace of the head alone)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def events(fn, n):
  """Device-event times (ms) of n calls of fn, one pair of events per call."""
  out = []
  for _ in range(n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b))
  return out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pad', type=int, nargs=2, default=[769, 1025])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--stride', type=int, default=342)
  ap.add_argument('--images', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=30, help='alternated (a)/(b) rounds of the per-crop head timing')
  ap.add_argument('--head-only', action='store_true')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_softmax_inference needs an MI355X (no CPU fallback)')
  from spml_amd import _ffi, inference
  from spml_amd.models.predictions import softmax_classifier as sc
  from spml_amd.train import build_models, voc12_scribble_config
  dev = torch.device('cuda', 0)
  cfg = voc12_scribble_config(batch_size=1, use_syncbn=False)
  c, ncls = cfg.network.embedding_dim, cfg.dataset.num_classes
  torch.manual_seed(235)
  head = sc.softmax_classifier(cfg).to(dev).eval()
  g = torch.Generator().manual_seed(1)
  with torch.no_grad():
    head.semantic_classifier[1].running_mean.copy_(0.05 * torch.randn(2 * c, generator=g))
    head.semantic_classifier[1].running_var.copy_(0.02 + 0.05 * torch.rand(2 * c, generator=g))
  crop, stride = (a.crop, a.crop), (a.stride, a.stride)
  res = {'image': list(a.pad), 'crop': a.crop, 'stride': a.stride, 'embedding_dim': c, 'num_classes': ncls}

  # ---- per crop: (a) HIP head, (b) framework fallback, identical inputs, alternated ----
  emb = torch.randn(1, c, a.crop, a.crop, generator=g).to(dev)
  canvas_a = torch.zeros(1, ncls, a.pad[0], a.pad[1], device=dev)
  canvas_b = torch.zeros_like(canvas_a)
  sh, sw = a.pad[0] - a.crop, a.pad[1] - a.crop
  head.prepare_inference()

  def hip_head():
    assert head.accumulate_logits(emb, canvas_a, sh, sw) == sc.HIP_HEAD_PATH

  def framework_head():
    with torch.no_grad():
      canvas_b[..., sh:sh + a.crop, sw:sw + a.crop] += head._logits(emb)

  for _ in range(a.warmup):
    hip_head(); framework_head()
    _ffi.argmax_channels(canvas_a[0], a.pad[0], a.pad[1]); torch.argmax(canvas_b, 1)
  torch.cuda.synchronize()
  scale = canvas_b.abs().max().item()
  res['head_max_abs_diff_over_max_logit'] = (canvas_a - canvas_b).abs().max().item() / scale
  t_a, t_b, t_am_a, t_am_b = [], [], [], []
  for _ in range(a.repeats):
    t_a += events(hip_head, 1)
    t_b += events(framework_head, 1)
    t_am_a += events(lambda: _ffi.argmax_channels(canvas_a[0], a.pad[0], a.pad[1]), 1)
    t_am_b += events(lambda: torch.argmax(canvas_b, 1), 1)
  res['per_crop_ms'] = {'hip_head': spread(t_a), 'framework_head': spread(t_b),
                        'framework_over_hip': round(statistics.median(t_b) / statistics.median(t_a), 3)}
  res['argmax_ms'] = {'hip': spread(t_am_a), 'framework': spread(t_am_b)}
  # bytes the head-accumulate kernel has to move: the hidden tensor once, the canvas window read and written
  p, ch = a.crop * a.crop, 2 * c
  res['head_accumulate_bytes'] = p * ch * 4 + 2 * p * ncls * 4

  # ---- whole images ----
  if not a.head_only:
    emb_model, _ = build_models(cfg, softmax_head=False)
    emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()
    image = torch.randn(1, 3, a.pad[0], a.pad[1], generator=g).to(dev)
    valid = (a.pad[0] - 20, a.pad[1] - 30)
    run = lambda: inference.predict_softmax_full_resolution(emb_model, head, image, valid, crop, stride)
    for _ in range(a.warmup):
      out = run()
    torch.cuda.synchronize()
    res['windows'] = len(inference.sliding_window_ends(a.pad[0], a.crop, a.stride)) * \
        len(inference.sliding_window_ends(a.pad[1], a.crop, a.stride))
    res['head_path'] = out['head_path']
    res['image_ms'] = spread(events(run, a.images))
  print(json.dumps(res))


if __name__ == '__main__':
  main()
