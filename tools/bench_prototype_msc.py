#!/usr/bin/env python3
"""Timing of the multi-scale memory-bank pass (pyscripts/inference/prototype_msc.py:92-206) on one synthetic image:
three scales (0.5, 1, 1.5), per view the sliding-window ResNet-101 DeepLab-v2 embedding, k-means that ignores the
padding, prototypes and the majority label per segment.

Prints one JSON line: ms per image (device events over whole images); per view size, on identical maps (a 12 x 12 grid
of segments, a blocky label map with strips of the ignore value 255, so 144 x 256 counters) and alternated in one
process, the time of
  (a) the HIP tail (`spml_segment_majority_i64`: memset + count + arg-max, no host read),
  (b) `find_majority_label_index` as it stands on the device (two host reads, index_add_ of P ones, arg-max, the
      `nonzero` over all pixels that the bank pass throws away),
  (c) the same entry of the other build of csrc/segment_majority.hip (-DSPML_MAJORITY_WAVE_COMBINE=0: one atomic per
      counted pixel instead of equal keys merged inside a wave; `spml_amd._build.build_variant` makes that library),
the same A/B with 21 classes (144 x 21 counters: the LDS table), the bytes each side has to move per view and the share
of the image spent in the tail.  Needs an MI355X: there is no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SCALES = [0.5, 1, 1.5]
GRID = 12                                # the k-means grid of the inference recipes: 144 segments
NUM_LABEL_VALUES = 256


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


def view_sizes(image_hw, scales=SCALES):
  return [(max(int(round(image_hw[0] * s)), 1), max(int(round(image_hw[1] * s)), 1)) for s in scales]


def tail_bytes(p, m, ncls):
  """What each formulation has to move per view, from the shapes.  kernel: the two int64 maps once and the counter
  table (zeroed, read).  reference: the [P, ncls] int64 one-hot and the scatter index of the same size
  (segsort/common.py:251-262).  framework: what `find_majority_label_index` here materialises -- the flat index, the
  ones, major[clu], the comparison and the nonzero output (at most P rows)."""
  return {'kernel': 16 * p + 2 * 4 * m * ncls, 'reference_one_hot_and_index': 2 * 8 * p * ncls,
          'framework_temporaries': 8 * p * 4 + p}


def variant_entry(path):
  """`segment_majority` of the other build of csrc/segment_majority.hip, bound by hand (spml_amd._ffi holds one
  library)."""
  from spml_amd import _ffi
  handle = ctypes.CDLL(path)
  for name in ('spml_segment_majority_workspace_bytes', 'spml_segment_majority_i64', 'spml_segment_majority_path_name'):
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = _ffi._SIGNATURES[name]

  def run(clu, sem, m, ncls, want_hist=False):
    major = torch.empty((m,), dtype=torch.int64, device=clu.device)
    hist = torch.empty((m, ncls), dtype=torch.int64, device=clu.device) if want_hist else None
    ws = _ffi.workspace(handle.spml_segment_majority_workspace_bytes(m, ncls), clu.device)
    _ffi.check(handle.spml_segment_majority_i64(_ffi.ptr(clu, torch.int64), _ffi.ptr(sem, torch.int64), clu.numel(), m,
                                                ncls, _ffi.ptr(major), _ffi.ptr(hist, None, True), _ffi.ptr(ws),
                                                ws.numel(), _ffi.stream_ptr()), 'spml_segment_majority_i64 (variant)')
    return (major, hist) if want_hist else major
  run.path_name = lambda p, m, ncls: handle.spml_segment_majority_path_name(p, m, ncls).decode()
  return run


def synthetic_maps(rh, rw, gen, dev):
  """Segment ids of a 12 x 12 grid and a blocky label map (classes 0..20 in 9 x 9 cells, every 40th row and column the
  ignore value: scribble-free borders), both int64 [rh * rw]."""
  ys = (torch.arange(rh) * GRID // rh).view(-1, 1)
  xs = (torch.arange(rw) * GRID // rw).view(1, -1)
  clu = (ys * GRID + xs).reshape(-1)
  cells = torch.randint(0, 21, (9, 9), generator=gen)
  sem = cells[(torch.arange(rh) * 9 // rh)][:, (torch.arange(rw) * 9 // rw)].clone()
  sem[::40, :] = 255
  sem[:, ::40] = 255
  return clu.to(dev), sem.reshape(-1).to(dev)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--stride', type=int, default=342)
  ap.add_argument('--images', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--repeats', type=int, default=50, help='alternated rounds of the per-view tail timing')
  ap.add_argument('--tail-only', action='store_true', help='skip the whole-image timing')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_prototype_msc needs an MI355X (no CPU fallback)')
  from spml_amd import _build, _ffi, inference
  import spml_amd.utils.segsort.common as sc
  dev = torch.device('cuda', 0)
  image_hw = tuple(a.image)
  crop, stride = (a.crop, a.crop), (a.stride, a.stride)
  g = torch.Generator().manual_seed(1)
  m = GRID * GRID
  variant = variant_entry(_build.build_variant('segment_majority.hip', ['SPML_MAJORITY_WAVE_COMBINE=0'],
                                               'spml_majority_per_pixel_atomics', verbose=False))
  res = {'image': list(image_hw), 'crop': a.crop, 'stride': a.stride, 'scales': SCALES, 'segments': m,
         'product_path': {'256_classes': _ffi.segment_majority_path_name(image_hw[0] * image_hw[1], m, 256),
                          '21_classes': _ffi.segment_majority_path_name(image_hw[0] * image_hw[1], m, 21)},
         'variant_path': {'256_classes': variant.path_name(image_hw[0] * image_hw[1], m, 256),
                          '21_classes': variant.path_name(image_hw[0] * image_hw[1], m, 21)}}

  per_view = []
  for rh, rw in view_sizes(image_hw):
    clu, sem = synthetic_maps(rh, rw, g, dev)
    p = rh * rw
    row = {'view': [rh, rw], 'bytes': tail_bytes(p, m, NUM_LABEL_VALUES)}
    # identical results first
    major, hist = _ffi.segment_majority(clu, sem, m, NUM_LABEL_VALUES, want_hist=True)
    v_major, v_hist = variant(clu, sem, m, NUM_LABEL_VALUES, want_hist=True)
    _, f_major = sc.find_majority_label_index(sem, clu)
    if not (torch.equal(major, v_major) and torch.equal(hist, v_hist)):
      raise SystemExit('the two builds of the kernel disagree on a %d x %d view' % (rh, rw))
    top2 = hist.topk(2, dim=1).values
    clear = top2[:, 0] > top2[:, 1]
    if not torch.equal(major[clear], f_major[clear]):
      raise SystemExit('kernel and find_majority_label_index disagree on a %d x %d view' % (rh, rw))
    row['tied_segments'] = int((~clear).sum())
    for tag, ncls in (('', NUM_LABEL_VALUES), ('_21_classes', 21)):
      runs = [lambda: _ffi.segment_majority(clu, sem, m, ncls), lambda: variant(clu, sem, m, ncls)]
      if not tag:
        runs.append(lambda: sc.find_majority_label_index(sem, clu))
      for _ in range(a.warmup):
        for fn in runs:
          fn()
      torch.cuda.synchronize()
      times = [[] for _ in runs]
      for _ in range(a.repeats):
        for t, fn in zip(times, runs):
          t += events(fn, 1)
      row['hip_ms' + tag] = spread(times[0])
      row['per_pixel_atomics_ms' + tag] = spread(times[1])
      row['per_pixel_atomics_over_hip' + tag] = round(statistics.median(times[1]) / statistics.median(times[0]), 3)
      if not tag:
        row['framework_ms'] = spread(times[2])
        row['framework_over_hip'] = round(statistics.median(times[2]) / statistics.median(times[0]), 3)
    per_view.append(row)
  res['per_view'] = per_view
  tail_ms = sum(v['hip_ms']['median'] for v in per_view)
  res['tail_ms'] = {'hip': round(tail_ms, 4), 'framework': round(sum(v['framework_ms']['median'] for v in per_view), 4),
                    'per_pixel_atomics': round(sum(v['per_pixel_atomics_ms']['median'] for v in per_view), 4)}
  if a.tail_only:
    print(json.dumps(res))
    return

  # ---- whole images ----
  from spml_amd.train import build_models, voc12_scribble_config
  cfg = voc12_scribble_config(batch_size=1, kmeans=GRID, use_syncbn=False)
  torch.manual_seed(235)
  emb_model, _ = build_models(cfg, softmax_head=False)
  emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()
  image = torch.randn(1, 3, image_hw[0], image_hw[1], generator=g).to(dev)
  label = synthetic_maps(image_hw[0], image_hw[1], g, dev)[1].view(image_hw)
  views = inference.flip_scale_views(image, SCALES, False, crop)
  labels = inference.label_views(label, [hw for _, hw, _ in views])
  run = lambda: inference.multiscale_prototypes(emb_model, views, labels, crop, stride, 255, NUM_LABEL_VALUES)
  for _ in range(a.warmup):
    out = run()
  torch.cuda.synchronize()
  res['majority_path'] = out['majority_path']
  res['segments_found'] = out['segment_counts']
  res['image_ms'] = spread(events(run, a.images))
  res['share_of_image'] = {'tail_hip': round(tail_ms / res['image_ms']['median'], 5),
                           'tail_framework': round(res['tail_ms']['framework'] / res['image_ms']['median'], 5)}
  print(json.dumps(res))


if __name__ == '__main__':
  main()
