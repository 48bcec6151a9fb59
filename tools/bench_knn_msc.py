#!/usr/bin/env python3
"""Timing of the multi-scale + flip kNN label inference (pyscripts/inference/inference_msc.py:129-242) on one synthetic
image: five scales x flip, per view the sliding-window ResNet-101 DeepLab-v2 embedding, k-means over the un-padded view,
top-20 retrieval per segment against a 20 000-prototype bank, then the per-view tail (votes, resize, un-flip, sum), the
mean over the views and one arg-max.

Prints one JSON line: ms per image (device events over whole images), per view the time of
  (a) the HIP tail (`spml_view_votes_accumulate_f32`: the table launch + the view kernel),
  (b) the framework ops of the reference (`inference.framework_view_votes_accumulate`) and, with `--variant-lib`,
  (c) the same entry of another build of csrc/knn_msc.hip (the votes table staged in LDS: -DSPML_VIEW_VOTES_LDS=1)
on identical id maps (a 12 x 12 grid of segments, 144 rows of retrieved labels), alternated in the same process, the
algorithmic bytes of the tail per view (the id map read once, the accumulator read and written once) and the share of
the image spent in the tail.  Needs an MI355X: there is no fallback.

The variant library is this one file alone:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -DSPML_VIEW_VOTES_LDS=1 -shared \\
      spml_amd/csrc/knn_msc.hip -o libknn_msc_lds.so

Kernel time per view size:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o knn -- python tools/bench_knn_msc.py --tail-only
  python tools/bench_knn_msc.py --summarize-trace DIR/.../knn_kernel_trace.csv

`--tail-only` launches nothing but the HIP tail (of `--variant-lib` when given), `--repeats` times per view in view
order, so dispatch k of `view_votes` in the trace belongs to view k // repeats; `--summarize-trace` prints per view the
median and minimum kernel time and the fraction of the 8 TB/s HBM rate the algorithmic bytes over the median time come
to."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SCALES = [0.5, 0.75, 1, 1.25, 1.5]
HBM_BYTES_PER_S = 8e12
GRID = 12                                # the k-means grid of the inference recipes: 144 segments
TOP_K = 20


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
  """What the tail has to move: the int64 id map once, the accumulator read and written."""
  return 8 * rh * rw + 4 * ncls * 2 * image_hw[0] * image_hw[1]


def reference_bytes(ncls, image_hw, rh, rw):
  """What the reference's ops materialise per view: the retrieved labels per pixel (int64) and their one-hot (the
  framework's one_hot is int64, its float copy fp32) -- the byte model of DESIGN 8f, computed from the shapes."""
  return {'labels_per_pixel': 8 * rh * rw * TOP_K, 'one_hot_fp32': 4 * rh * rw * TOP_K * ncls}


def summarize_trace(path, a, ncls):
  rows = []
  with open(path) as f:
    for r in csv.DictReader(f):
      if 'view_votes' in r['Kernel_Name']:
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
  rows.sort()
  views = view_geometry(a.image, a.crop)
  if len(rows) != len(views) * a.repeats:
    raise SystemExit('expected %d view_votes dispatches (--tail-only --repeats %d), found %d'
                     % (len(views) * a.repeats, a.repeats, len(rows)))
  print('| view (region, flip) | median us | min us | algorithmic MB | of 8 TB/s |')
  print('|---|---|---|---|---|')
  for k, (_, _, rh, rw, flip) in enumerate(views):
    t = [d / 1e3 for _, d in rows[k * a.repeats:(k + 1) * a.repeats]]
    nbytes = tail_bytes(ncls, a.image, rh, rw)
    print('| %d x %d, %d | %.1f | %.1f | %.2f | %.1f %% |'
          % (rh, rw, flip, statistics.median(t), min(t), nbytes / 1e6,
             100 * nbytes / (statistics.median(t) * 1e-6) / HBM_BYTES_PER_S))


def variant_tail(path):
  """`view_votes_accumulate` of another build of csrc/knn_msc.hip, bound by hand (spml_amd._ffi holds one library)."""
  from spml_amd import _ffi
  handle = ctypes.CDLL(path)
  for name in ('spml_view_votes_workspace_bytes', 'spml_view_votes_accumulate_f32'):
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = _ffi._SIGNATURES[name]

  def run(clu, crop_hw, topk, ncls, flip, acc):
    m, k = topk.shape
    nbytes = handle.spml_view_votes_workspace_bytes(int(m), int(ncls))
    if nbytes == 0:
      raise SystemExit('%s does not take %d segments x %d classes' % (path, m, ncls))
    ws = _ffi.workspace(nbytes, acc.device)
    _ffi.check(handle.spml_view_votes_accumulate_f32(
        _ffi.ptr(clu, torch.int64), int(crop_hw[0]), int(crop_hw[1]), _ffi.ptr(topk, torch.int64), int(m), int(k),
        int(ncls), int(bool(flip)), acc.shape[1], acc.shape[2], _ffi.ptr(acc, torch.float32), _ffi.ptr(ws), ws.numel(),
        _ffi.stream_ptr()), 'spml_view_votes_accumulate_f32 (variant)')
    return acc
  return run


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--stride', type=int, default=342)
  ap.add_argument('--bank', type=int, default=20000, help='prototypes in the memory bank')
  ap.add_argument('--images', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--repeats', type=int, default=30, help='alternated rounds of the per-view tail timing')
  ap.add_argument('--variant-lib', default=None, metavar='SO', help='another build of csrc/knn_msc.hip to time beside this one')
  ap.add_argument('--tail-only', action='store_true')
  ap.add_argument('--summarize-trace', default=None, metavar='CSV')
  a = ap.parse_args()
  from spml_amd.train import build_models, voc12_scribble_config
  cfg = voc12_scribble_config(batch_size=1, kmeans=GRID, use_syncbn=False)
  c, ncls = cfg.network.embedding_dim, cfg.dataset.num_classes
  if a.summarize_trace:
    return summarize_trace(a.summarize_trace, a, ncls)
  if not torch.cuda.is_available():
    raise SystemExit('bench_knn_msc needs an MI355X (no CPU fallback)')
  from spml_amd import _ffi, inference
  dev = torch.device('cuda', 0)
  image_hw = tuple(a.image)
  crop, stride = (a.crop, a.crop), (a.stride, a.stride)
  g = torch.Generator().manual_seed(1)
  geometry = view_geometry(image_hw, a.crop)
  res = {'image': list(image_hw), 'crop': a.crop, 'stride': a.stride, 'embedding_dim': c, 'num_classes': ncls,
         'views': len(geometry), 'bank': a.bank, 'segments': GRID * GRID}
  variant = variant_tail(a.variant_lib) if a.variant_lib else None

  # ---- per view: (a) HIP tail, (b) framework tail, (c) the variant build; identical inputs, alternated ----
  accs = [torch.zeros((ncls,) + image_hw, device=dev) for _ in range(3)]
  tails = []
  for _, _, rh, rw, flip in geometry:
    ys = (torch.arange(rh) * GRID // rh).view(-1, 1)
    xs = (torch.arange(rw) * GRID // rw).view(1, -1)
    clu = (ys * GRID + xs).reshape(-1).to(dev)
    topk = torch.randint(0, ncls, (GRID * GRID, TOP_K), generator=g).to(dev)
    tails.append((clu, (rh, rw), topk, ncls, flip))
  if a.tail_only:
    run = variant or _ffi.view_votes_accumulate
    for args in tails:
      for _ in range(a.repeats):
        run(*args, accs[0])
    torch.cuda.synchronize()
    print(json.dumps(dict(res, tail_only=True, repeats=a.repeats, variant_lib=a.variant_lib)))
    return
  per_view, worst, worst_variant = [], 0.0, 0.0
  for (_, _, rh, rw, flip), args in zip(geometry, tails):
    runs = [lambda: _ffi.view_votes_accumulate(*args, accs[0]),
            lambda: inference.framework_view_votes_accumulate(*args, accs[1])]
    if variant:
      runs.append(lambda: variant(*args, accs[2]))
    for acc in accs:
      acc.zero_()
    for fn in runs:
      fn()
    worst = max(worst, (accs[0] - accs[1]).abs().max().item())
    if variant:
      worst_variant = max(worst_variant, (accs[0] - accs[2]).abs().max().item())
    for _ in range(a.warmup):
      for fn in runs:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in runs]
    for _ in range(a.repeats):
      for t, fn in zip(times, runs):
        t += events(fn, 1)
    nbytes = tail_bytes(ncls, image_hw, rh, rw)
    row = {'region': [rh, rw], 'flip': int(flip), 'hip_ms': spread(times[0]), 'framework_ms': spread(times[1]),
           'algorithmic_bytes': nbytes, 'reference_bytes': reference_bytes(ncls, image_hw, rh, rw),
           'framework_over_hip': round(statistics.median(times[1]) / statistics.median(times[0]), 3),
           'hip_fraction_of_8TBps_by_events': round(nbytes / (statistics.median(times[0]) * 1e-3) / HBM_BYTES_PER_S, 4)}
    if variant:
      row['variant_ms'] = spread(times[2])
      row['variant_over_hip'] = round(statistics.median(times[2]) / statistics.median(times[0]), 3)
    per_view.append(row)
  res['per_view'] = per_view
  res['tail_max_abs_diff'] = worst
  tail_ms = sum(v['hip_ms']['median'] for v in per_view)
  res['tail_ms'] = {'hip': round(tail_ms, 4), 'framework': round(sum(v['framework_ms']['median'] for v in per_view), 4)}
  if variant:
    res['variant_lib'] = a.variant_lib
    res['variant_max_abs_diff'] = worst_variant
    res['tail_ms']['variant'] = round(sum(v['variant_ms']['median'] for v in per_view), 4)

  # ---- whole images ----
  from spml_amd.models.predictions.segsort import segsort
  torch.manual_seed(235)
  emb_model, _ = build_models(cfg, softmax_head=False)
  emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()
  predictor = segsort(cfg).to(dev).eval()
  bank = torch.nn.functional.normalize(torch.randn(a.bank, c, generator=g), dim=1).to(dev)
  bank_lab = torch.randint(0, ncls, (a.bank,), generator=g).to(dev)
  image = torch.randn(1, 3, image_hw[0], image_hw[1], generator=g).to(dev)
  views = inference.flip_scale_views(image, SCALES, True, crop)
  assert [tuple(v[0].shape[-2:]) + tuple(v[1]) + (v[2],) for v in views] == geometry
  run = lambda: inference.predict_knn_multiscale(emb_model, predictor, views, image_hw, crop, stride, bank, bank_lab,
                                                 ncls)
  for _ in range(a.warmup):
    out = run()
  torch.cuda.synchronize()
  res['combine_path'] = out['combine_path']
  res['segments_found'] = [int(t.shape[0]) for t in out['segment_topk']]
  res['image_ms'] = spread(events(run, a.images))
  res['share_of_image'] = {'tail_hip': round(tail_ms / res['image_ms']['median'], 5),
                           'tail_framework': round(res['tail_ms']['framework'] / res['image_ms']['median'], 5)}
  print(json.dumps(res))


if __name__ == '__main__':
  main()
