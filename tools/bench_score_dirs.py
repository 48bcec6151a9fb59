#!/usr/bin/env python3
"""Timing of scoring label files (csrc/score_batch.hip) at the recipe's shape: a batch of 64 files of
375 x 500, 21 classes, with instance planes.

Prints one JSON line.  The routes alternate in one process on identical inputs, device events around each:
  * `score_batch_ms`: (a) the one `_ffi.score_batch` call on the packed planes already on the device (workspace memset,
    count launch, finish launch); `round_trip_ms`: the same with the upload of the staged planes from pinned memory
    before it and the download of `[B, 4, ncls]` after it -- what `DirectoryScorer.score_batch` does per batch;
  * `per_image_ms`: (b) the existing per-image device route on the same files, `metrics.InstanceIoU.update` from the
    uint8 maps on the device, conversions to int64 and the copy to the host per file included;
  * `host_ms`: (c) the reference's chain as numpy on the host, restated in this file (three np.histogram per file,
    np.unique and one mask + np.histogram per instance id), and `host_table_ms`: the table formulation of
    tests/score_ref.py (two np.bincount per file);
  * `equal`: the three routes give the same `[B, 4, ncls]`;
  * `upload_bytes_per_file`, `download_bytes_per_file`, against what the per-image route moves;
  * `scorer_files_per_s`: `DirectoryScorer` end to end on in-memory PNGs with the decode pool at 16 threads, and
    `decode_only_files_per_s`: the same pool decoding alone -- the two together say whether the program is decode-bound.
Needs an MI355X: there is no fallback."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def make_file(h, w, ncls, seed):
  """A blocky ground truth with unlabelled pixels, a prediction that agrees on most of it, a handful of instances."""
  rng = np.random.RandomState(seed)
  cell = lambda values, c: rng.choice(values, (h // c + 1, w // c + 1))[np.arange(h)[:, None] // c, np.arange(w)[None] // c]
  gt = cell(np.arange(ncls), 64).astype(np.uint8)
  gt[rng.rand(h, w) < 0.05] = 255
  pred = np.where(rng.rand(h, w) < 0.8, np.minimum(gt, ncls - 1), cell(np.arange(ncls), 32)).astype(np.uint8)
  inst = cell(np.array([0, 1, 2, 3, 4, 5, 255]), 96).astype(np.uint8)
  return pred, gt, inst


def host_chain(pred, gt, inst, ncls):
  """benchmark_by_mIoU.py:25-53 and benchmark_by_instance.py:97-108 restated: the reference's own numpy calls."""
  bins = np.arange(ncls + 1)
  locs = np.logical_and(gt > -1, gt < ncls)
  tp_fn, _ = np.histogram(gt[locs], bins=bins)
  tp_fp, _ = np.histogram(pred[locs], bins=bins)
  tp, _ = np.histogram(gt[np.logical_and(locs, pred == gt)], bins=bins)
  ninst = np.zeros(ncls, dtype=np.int64)
  for i, ind in enumerate(np.unique(inst)):
    if i < 255:
      npixel, _ = np.histogram(gt[inst == ind], bins=ncls, range=(0, ncls - 1))
      ninst[np.argmax(npixel)] += 1
  return np.stack([tp_fn, tp_fp, tp, ninst]).astype(np.int64)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--files', type=int, default=64)
  ap.add_argument('--num_classes', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--host_repeats', type=int, default=2)
  ap.add_argument('--scorer_files', type=int, default=512)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_score_dirs needs an MI355X (no CPU fallback)')
  import score_ref
  from PIL import Image
  from spml_amd import _ffi
  from spml_amd.utils.general import metrics
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  (h, w), ncls, B = a.image, a.num_classes, a.files
  distinct = [make_file(h, w, ncls, 100 + i) for i in range(min(B, 8))]
  files = [distinct[i % len(distinct)] for i in range(B)]

  packed_np, records = score_ref.pack(files)
  rec_bytes = records.view(np.uint8).reshape(-1)
  staging = torch.empty((packed_np.size + rec_bytes.size,), dtype=torch.uint8).pin_memory()
  staging[:packed_np.size] = torch.from_numpy(packed_np)
  staging[packed_np.size:] = torch.from_numpy(rec_bytes.copy())
  on_dev = staging.to(dev)
  packed, params_dev = on_dev[:packed_np.size], on_dev[packed_np.size:]
  maps_dev = [tuple(torch.from_numpy(m).to(dev) for m in f) for f in distinct]
  maps_dev = [maps_dev[i % len(distinct)] for i in range(B)]

  def route_a():
    return _ffi.score_batch(packed, records, ncls, params_dev=params_dev)

  def route_a_round_trip():
    up = staging.to(dev, non_blocking=True)
    return _ffi.score_batch(up[:packed_np.size], records, ncls, params_dev=up[packed_np.size:]).cpu()

  def route_b():
    rows = []
    for pred, gt, inst in maps_dev:
      stats = metrics.iou_stats(pred, gt, ncls)
      rows.append(torch.cat([stats, metrics.instance_class_counts(inst, gt, ncls).view(1, -1)], 0))
    return torch.stack(rows)

  def route_b_update_only():
    acc = metrics.InstanceIoU(ncls)
    for pred, gt, inst in maps_dev:
      acc.update(pred, gt, inst)
    return acc

  got_a = route_a().cpu().numpy()
  got_b = route_b().cpu().numpy()
  t0 = time.perf_counter()
  for _ in range(a.host_repeats):
    got_c = np.stack([host_chain(p, g, s, ncls) for p, g, s in files])
  host_ms = (time.perf_counter() - t0) * 1e3 / a.host_repeats
  t0 = time.perf_counter()
  for _ in range(a.host_repeats):
    got_t = score_ref.batch_stats(files, ncls)
  host_table_ms = (time.perf_counter() - t0) * 1e3 / a.host_repeats
  equal = bool(np.array_equal(got_a, got_b) and np.array_equal(got_a, got_c) and np.array_equal(got_a, got_t))

  t_a, t_rt, t_b = [], [], []
  for i in range(a.warmup + a.repeats):
    ms_a, _ = timed(route_a)
    ms_rt, _ = timed(route_a_round_trip)
    ms_b, _ = timed(route_b_update_only)
    if i >= a.warmup:
      t_a.append(ms_a)
      t_rt.append(ms_rt)
      t_b.append(ms_b)

  def png(plane, mode):
    f = io.BytesIO()
    im = Image.fromarray(plane)
    if mode == 'P':                                          # (a palette turns the L image into a P image, indices kept)
      im.putpalette([v for i in range(256) for v in (i, (i * 3) % 256, (i * 7) % 256)])
    im.save(f, format='PNG')
    return f.getvalue()

  encoded = [(png(p, 'L'), png(g, 'L'), png(s, 'P')) for p, g, s in distinct]
  triples = [encoded[i % len(encoded)] for i in range(a.scorer_files)]
  metrics.DirectoryScorer(ncls, batch_files=B).score(triples[:B])                      # (warm: pinned buffer, pool)
  t0 = time.perf_counter()
  result = metrics.DirectoryScorer(ncls, batch_files=B, decode_threads=16).score(triples).result()
  scorer_s = time.perf_counter() - t0
  from concurrent.futures import ThreadPoolExecutor
  t0 = time.perf_counter()
  with ThreadPoolExecutor(max_workers=16) as pool:
    list(pool.map(metrics.DirectoryScorer._decode, triples))
  decode_s = time.perf_counter() - t0

  n = h * w
  print(json.dumps({
      'shape': {'files': B, 'h': h, 'w': w, 'num_classes': ncls, 'instance_planes': True},
      'score_path': _ffi.score_batch_path_name(records, packed_np.size, ncls), 'equal': equal,
      'score_batch_ms': spread(t_a), 'round_trip_ms': spread(t_rt), 'per_image_ms': spread(t_b),
      'host_ms': round(host_ms, 2), 'host_table_ms': round(host_table_ms, 2),
      'per_image_over_score_batch': round(statistics.median(t_b) / statistics.median(t_a), 1),
      'plane_gb_per_s': round(packed_np.size / (statistics.median(t_a) * 1e-3) / 1e9, 1),
      'upload_bytes_per_file': (packed_np.size + rec_bytes.size) // B, 'download_bytes_per_file': 4 * ncls * 8,
      'per_image_route_bytes_per_file': {'upload': 3 * n, 'int64_maps_written_and_read': 4 * 8 * n, 'download': 4 * ncls * 8},
      'scorer_files': a.scorer_files, 'scorer_files_per_s': round(a.scorer_files / scorer_s, 1),
      'decode_only_files_per_s': round(a.scorer_files / decode_s, 1), 'scorer_batches': result['batches'],
      'scorer_mean_iou': round(result['mean_iou'], 4)}))


if __name__ == '__main__':
  main()
