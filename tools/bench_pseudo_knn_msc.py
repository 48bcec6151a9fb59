#!/usr/bin/env python3
"""Timing of the tag recipe's kNN pseudo-label generation (pyscripts/inference/pseudo_inference_crf_msc.py:143-275,
without the denseCRF) on one synthetic image: four scales x flip, per view the sliding-window ResNet-101 DeepLab-v2
embedding, k-means over the un-padded view and top-20 retrieval per segment, the vote-view kernel, then the
tag-normalised arg-max.

Prints one JSON line:
  * ms per image of `inference.pseudo_labels_knn_multiscale` (device events over whole images);
  * the tail alone on one sum of eight views: `_ffi.tag_normalize_argmax` (spml_tag_normalize_argmax_f32, two launches)
    against `inference.framework_tag_normalize_argmax` (torch ops on the device), labels only and with the normalised
    map handed out.  The two are alternated in one process in rounds of `--calls` calls between one pair of device
    events, after a warm-up, until each has been timed for `--window` seconds (at least half a second);
  * the byte model from the shapes: the kernel pair reads the sum twice and writes the labels (plus the map when asked);
    the framework ops make seven passes over an [ncls, n] tensor (the division by the view count: read + write; the
    maximum: read; the division by the divisor: read + write; the arg-max: read) -- with n = h * w.
Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SCALES = [0.5, 1, 1.5, 2]
GRID = 12                                # the k-means grid of the inference recipes: 144 segments
TOP_K = 20


def spread(v):
  return {'median': round(statistics.median(v), 5), 'min': round(min(v), 5), 'max': round(max(v), 5), 'n': len(v)}


def byte_model(ncls, n, want_prob):
  plane = 4 * ncls * n
  return {'hip': 2 * plane + 8 * n + (plane if want_prob else 0),
          'framework': 7 * plane + 8 * n,
          'framework_passes': 'acc/V: r+w, amax: r, mean/div: r+w, argmax: r (+ the labels)'}


def timed_round(fn, calls):
  """ms per call of `calls` calls of fn between one pair of device events."""
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(calls):
    fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) / calls


def alternate(fns, calls, window_s, warmup):
  """Rounds of every fn in turn until each has been timed for `window_s` seconds -> per fn the ms per call of each round."""
  for _ in range(warmup):
    for fn in fns:
      fn()
  torch.cuda.synchronize()
  times, total = [[] for _ in fns], [0.0 for _ in fns]
  while min(total) < window_s * 1e3:
    for i, fn in enumerate(fns):
      t = timed_round(fn, calls)
      times[i].append(t)
      total[i] += t * calls
  return times, [round(t / 1e3, 3) for t in total]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--stride', type=int, default=342)
  ap.add_argument('--bank', type=int, default=20000, help='prototypes in the memory bank')
  ap.add_argument('--images', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--calls', type=int, default=200, help='calls of the tail between one pair of events')
  ap.add_argument('--window', type=float, default=0.5, help='seconds each side of the tail A/B is timed for')
  ap.add_argument('--tail-only', action='store_true', help='skip the whole-image timing')
  a = ap.parse_args()
  if a.window < 0.5:
    raise SystemExit('--window must be at least half a second')
  if not torch.cuda.is_available():
    raise SystemExit('bench_pseudo_knn_msc needs an MI355X (no CPU fallback)')
  from spml_amd import _ffi, inference
  from spml_amd.train import build_models, voc12_scribble_config
  cfg = voc12_scribble_config(batch_size=1, kmeans=GRID, use_syncbn=False)
  c, ncls = cfg.network.embedding_dim, cfg.dataset.num_classes
  dev = torch.device('cuda', 0)
  image_hw = tuple(a.image)
  n = image_hw[0] * image_hw[1]
  crop, stride = (a.crop, a.crop), (a.stride, a.stride)
  g = torch.Generator().manual_seed(1)
  res = {'image': list(image_hw), 'crop': a.crop, 'stride': a.stride, 'num_classes': ncls, 'views': 2 * len(SCALES),
         'bank': a.bank}

  # ---- the tail alone: one sum of eight views over a 12 x 12 grid of segments, every other class tagged ----
  acc = torch.zeros((ncls,) + image_hw, device=dev)
  for scale in SCALES:
    rh, rw = max(int(round(image_hw[0] * scale)), 1), max(int(round(image_hw[1] * scale)), 1)
    ys = (torch.arange(rh) * GRID // rh).view(-1, 1)
    xs = (torch.arange(rw) * GRID // rw).view(1, -1)
    clu = (ys * GRID + xs).reshape(-1).to(dev)
    for flip in (True, False):
      topk = torch.randint(0, ncls, (GRID * GRID, TOP_K), generator=g).to(dev)
      _ffi.view_votes_accumulate(clu, (rh, rw), topk, ncls, flip, acc)
  views = 2 * len(SCALES)
  tags = (torch.arange(ncls) % 2 == 0).to(dev)
  hip = _ffi.tag_normalize_argmax(acc, views, tags, 0.15, True)
  ref = inference.framework_tag_normalize_argmax(acc, views, tags, 0.15, True)
  res['tail_check'] = {'labels_differ': int((hip[0] != ref[0]).sum()), 'prob_max_abs_diff': (hip[1] - ref[1]).abs().max().item(),
                       'divisor_max_abs_diff': (hip[2] - ref[2]).abs().max().item()}
  res['tail'] = {}
  for name, want_prob in (('labels_only', False), ('with_prob', True)):
    fns = [lambda: _ffi.tag_normalize_argmax(acc, views, tags, 0.15, want_prob),
           lambda: inference.framework_tag_normalize_argmax(acc, views, tags, 0.15, want_prob)]
    times, windows = alternate(fns, a.calls, a.window, a.warmup)
    med = [statistics.median(t) for t in times]
    res['tail'][name] = {'hip_ms': spread(times[0]), 'framework_ms': spread(times[1]), 'timed_seconds': windows,
                         'calls_per_round': a.calls, 'framework_over_hip': round(med[1] / med[0], 3),
                         'bytes': byte_model(ncls, n, want_prob)}

  # ---- whole images ----
  if not a.tail_only:
    from spml_amd.models.predictions.segsort import segsort
    torch.manual_seed(235)
    emb_model, _ = build_models(cfg, softmax_head=False)
    emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()
    predictor = segsort(cfg).to(dev).eval()
    bank = torch.nn.functional.normalize(torch.randn(a.bank, c, generator=g), dim=1).to(dev)
    bank_lab = torch.randint(0, ncls, (a.bank,), generator=g).to(dev)
    image = torch.randn(1, 3, image_hw[0], image_hw[1], generator=g).to(dev)
    image_views = inference.flip_scale_views(image, SCALES, True, crop)
    run = lambda: inference.pseudo_labels_knn_multiscale(emb_model, predictor, image_views, image_hw, crop, stride, bank,
                                                         bank_lab, ncls, tags)
    for _ in range(a.warmup):
      out = run()
    torch.cuda.synchronize()
    res['combine_path'], res['normalize_path'] = out['combine_path'], out['normalize_path']
    res['segments_found'] = [int(t.shape[0]) for t in out['segment_topk']]
    per_image = []
    for _ in range(a.images):
      per_image.append(timed_round(run, 1))
    res['image_ms'] = spread(per_image)
    res['tail_share_of_image'] = round(res['tail']['labels_only']['hip_ms']['median'] / res['image_ms']['median'], 6)
  print(json.dumps(res))


if __name__ == '__main__':
  main()
