#!/usr/bin/env python3
"""Timing of the multi-scale + flip softmax label inference (pyscripts/inference/inference_softmax_msc.py:95-149) on
one synthetic image: five scales x flip, per view the sliding-window ResNet-101 DeepLab-v2 embedding and the classifier
head, then the per-view tail (counts, crop, resize, softmax, un-flip, sum) and one arg-max.

Prints one JSON line: ms per image (device events over whole images), per view the time of
  (a) the HIP tail (`spml_view_probs_accumulate_f32`, one launch) and
  (b) the framework ops of the reference (`inference.framework_view_probs_accumulate`)
on identical canvases, alternated in the same process, the algorithmic bytes of the kernel per view (the canvas
region read once, the accumulator read and written once), and the share of the image spent in the backbone, the head and
the tail, each timed on its own.  Needs an MI355X: there is no fallback.

Kernel time per view size:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o msc -- python tools/bench_softmax_msc.py --tail-only
  python tools/bench_softmax_msc.py --summarize-trace DIR/.../msc_kernel_trace.csv

`--tail-only` launches nothing but the HIP tail, `--repeats` times per view in view order, so dispatch k of
`view_probs` in the trace belongs to view k // repeats; `--summarize-trace` prints per view the median and minimum
kernel time and the fraction of the 8 TB/s HBM rate the algorithmic bytes over the median time come to."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SCALES = [0.5, 0.75, 1, 1.25, 1.5]
HBM_BYTES_PER_S = 8e12


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


def view_geometry(image_hw, crop, scales=SCALES):
  """(pad_h, pad_w, rh, rw, flip) of every view, in the order of `flip_scale_views`."""
  out = []
  for scale in scales:
    rh, rw = max(int(round(image_hw[0] * scale)), 1), max(int(round(image_hw[1] * scale)), 1)
    for flip in (True, False):
      out.append((max(rh, crop), max(rw, crop), rh, rw, flip))
  return out


def tail_bytes(ncls, image_hw, rh, rw):
  """What the tail has to move: the rh x rw region of the canvas once, the accumulator read and written."""
  return 4 * ncls * (rh * rw + 2 * image_hw[0] * image_hw[1])


def summarize_trace(path, a, ncls):
  rows = []
  with open(path) as f:
    for r in csv.DictReader(f):
      if 'view_probs' in r['Kernel_Name']:
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
  rows.sort()
  views = view_geometry(a.image, a.crop)
  if len(rows) != len(views) * a.repeats:
    raise SystemExit('expected %d view_probs dispatches (--tail-only --repeats %d), found %d'
                     % (len(views) * a.repeats, a.repeats, len(rows)))
  print('| view (padded, region, flip) | median us | min us | algorithmic MB | of 8 TB/s |')
  print('|---|---|---|---|---|')
  for k, (ph, pw, rh, rw, flip) in enumerate(views):
    t = [d / 1e3 for _, d in rows[k * a.repeats:(k + 1) * a.repeats]]
    nbytes = tail_bytes(ncls, a.image, rh, rw)
    print('| %d x %d, %d x %d, %d | %.1f | %.1f | %.2f | %.1f %% |'
          % (ph, pw, rh, rw, flip, statistics.median(t), min(t), nbytes / 1e6,
             100 * nbytes / (statistics.median(t) * 1e-6) / HBM_BYTES_PER_S))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--stride', type=int, default=342)
  ap.add_argument('--images', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=30, help='alternated (a)/(b) rounds of the per-view tail timing')
  ap.add_argument('--tail-only', action='store_true')
  ap.add_argument('--summarize-trace', default=None, metavar='CSV')
  a = ap.parse_args()
  from spml_amd.train import build_models, voc12_scribble_config
  cfg = voc12_scribble_config(batch_size=1, use_syncbn=False)
  c, ncls = cfg.network.embedding_dim, cfg.dataset.num_classes
  if a.summarize_trace:
    return summarize_trace(a.summarize_trace, a, ncls)
  if not torch.cuda.is_available():
    raise SystemExit('bench_softmax_msc needs an MI355X (no CPU fallback)')
  from spml_amd import _ffi, inference
  from spml_amd.models.predictions import softmax_classifier as sc
  dev = torch.device('cuda', 0)
  image_hw = tuple(a.image)
  crop, stride = (a.crop, a.crop), (a.stride, a.stride)
  g = torch.Generator().manual_seed(1)
  geometry = view_geometry(image_hw, a.crop)
  res = {'image': list(image_hw), 'crop': a.crop, 'stride': a.stride, 'embedding_dim': c, 'num_classes': ncls,
         'views': len(geometry)}

  # ---- per view: (a) HIP tail, (b) framework tail, identical canvases, alternated ----
  acc_a = torch.zeros((ncls,) + image_hw, device=dev)
  acc_b = torch.zeros_like(acc_a)
  tails = []
  for ph, pw, rh, rw, flip in geometry:
    canvas = (4.0 * torch.randn(ncls, ph, pw, generator=g)).to(dev)
    cnt_y = torch.from_numpy(inference.window_counts(ph, a.crop, a.stride)).to(dev)
    cnt_x = torch.from_numpy(inference.window_counts(pw, a.crop, a.stride)).to(dev)
    canvas *= cnt_y.view(-1, 1) * cnt_x.view(1, -1)              # (summed window logits: the quotient is of logit size)
    tails.append((canvas, cnt_y, cnt_x, (rh, rw), flip))
  if a.tail_only:
    for args in tails:
      for _ in range(a.repeats):
        _ffi.view_probs_accumulate(*args, acc_a)
    torch.cuda.synchronize()
    print(json.dumps(dict(res, tail_only=True, repeats=a.repeats)))
    return
  per_view, worst = [], 0.0
  for (ph, pw, rh, rw, flip), args in zip(geometry, tails):
    hip = lambda: _ffi.view_probs_accumulate(*args, acc_a)
    framework = lambda: inference.framework_view_probs_accumulate(*args, acc_b)
    acc_a.zero_(); acc_b.zero_()
    hip(); framework()
    worst = max(worst, (acc_a - acc_b).abs().max().item())
    for _ in range(a.warmup):
      hip(); framework()
    torch.cuda.synchronize()
    t_a, t_b = [], []
    for _ in range(a.repeats):
      t_a += events(hip, 1)
      t_b += events(framework, 1)
    nbytes = tail_bytes(ncls, image_hw, rh, rw)
    per_view.append({'pad': [ph, pw], 'region': [rh, rw], 'flip': int(flip), 'hip_ms': spread(t_a),
                     'framework_ms': spread(t_b), 'algorithmic_bytes': nbytes,
                     'framework_over_hip': round(statistics.median(t_b) / statistics.median(t_a), 3),
                     'hip_fraction_of_8TBps_by_events': round(nbytes / (statistics.median(t_a) * 1e-3) / HBM_BYTES_PER_S, 4)})
  res['per_view'] = per_view
  res['tail_max_abs_diff'] = worst
  tail_ms = sum(v['hip_ms']['median'] for v in per_view)
  framework_tail_ms = sum(v['framework_ms']['median'] for v in per_view)

  # ---- whole images, and the backbone / the head on their own ----
  torch.manual_seed(235)
  head = sc.softmax_classifier(cfg).to(dev).eval()
  with torch.no_grad():
    head.semantic_classifier[1].running_mean.copy_(0.05 * torch.randn(2 * c, generator=g))
    head.semantic_classifier[1].running_var.copy_(0.02 + 0.05 * torch.rand(2 * c, generator=g))
  emb_model, _ = build_models(cfg, softmax_head=False)
  emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()
  image = torch.randn(1, 3, image_hw[0], image_hw[1], generator=g).to(dev)
  views = inference.flip_scale_views(image, SCALES, True, crop)
  assert [tuple(v[0].shape[-2:]) + tuple(v[1]) + (v[2],) for v in views] == geometry
  run = lambda: inference.predict_softmax_multiscale(emb_model, head, views, image_hw, crop, stride)
  for _ in range(a.warmup):
    out = run()
  torch.cuda.synchronize()
  res['head_path'], res['combine_path'] = out['head_path'], out['combine_path']
  res['image_ms'] = spread(events(run, a.images))
  windows = [len(inference.sliding_window_ends(ph, a.crop, a.stride)) *
             len(inference.sliding_window_ends(pw, a.crop, a.stride)) for ph, pw, _, _, _ in geometry]
  res['crops'] = sum(windows)
  # the backbone on the batches of crops the image sends through it: consecutive views of one padded size form a group
  # (here the six 513 x 513 views, the 513 x 625 pair, the 562 x 750 pair), a group's crops go view after view in
  # batches of 8 -- the arrangement of inference.predict_softmax_multiscale; the image's own crops, padding included
  groups = []
  for k, view in enumerate(views):
    if groups and views[groups[-1][0]][0].shape == view[0].shape:
      groups[-1].append(k)
    else:
      groups.append([k])
  batches = []
  for part in groups:
    ph, pw = views[part[0]][0].shape[-2:]
    wins = [(v, int(eh) - a.crop, int(ew) - a.crop) for v in part
            for eh in inference.sliding_window_ends(ph, a.crop, a.stride)
            for ew in inference.sliding_window_ends(pw, a.crop, a.stride)]
    for g0 in range(0, len(wins), 8):
      batches.append(torch.cat([views[v][0][:, :, sh:sh + a.crop, sw:sw + a.crop] for v, sh, sw in wins[g0:g0 + 8]], 0)
                     .contiguous(memory_format=torch.channels_last))
  res['backbone_batches'] = [b.shape[0] for b in batches]
  assert sum(b.shape[0] for b in batches) == res['crops']

  def backbone():
    with torch.no_grad():
      for crops in batches:
        emb_model.generate_embeddings({'image': crops}, resize_as_input=True)

  # ... and the head on as many crops
  emb = torch.randn(1, c, a.crop, a.crop, generator=g).to(dev)
  canvas = torch.zeros(1, ncls, a.crop, a.crop, device=dev)

  def heads():
    for _ in range(res['crops']):
      head.accumulate_logits(emb, canvas, 0, 0)

  for _ in range(a.warmup):
    backbone(); heads()
  torch.cuda.synchronize()
  t_backbone, t_head = spread(events(backbone, a.images)), spread(events(heads, a.images))
  total = res['image_ms']['median']
  res['parts_ms'] = {'backbone': t_backbone, 'head': t_head, 'tail_hip': round(tail_ms, 4),
                     'tail_framework': round(framework_tail_ms, 4)}
  res['share_of_image'] = {'backbone': round(t_backbone['median'] / total, 4),
                           'head': round(t_head['median'] / total, 4), 'tail': round(tail_ms / total, 4)}
  print(json.dumps(res))


if __name__ == '__main__':
  main()
