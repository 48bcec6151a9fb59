#!/usr/bin/env python3
"""Timing of the CAM route of `pseudo_softmaxrw.py --cam_dir` (csrc/cam_ingest.hip) at the recipe's shape: a
375 x 500 image, 21 classes, a CAM file with K = 3 planes.

Prints one JSON line (device events, medians over `--repeats` after `--warmup`):
  * `ingest.hip_ms`: the one launch of `spml_cam_ingest_f32` from the K planes on the device;
    `ingest.framework_ms`: `inference.cam_with_background` + `inference.downsampled_cam` on the same device planes (the
    zeroed `[21, h, w]` array, K plane copies, max, pow, `F.interpolate`), what `pseudo_camrw_crf.py` runs;
    `ingest.max_abs_diff`: the largest difference between the two results;
  * `list.upload_bytes_per_image`: what one image sends up in its single copy (view records, RGB, semantic plane and the
    K fp32 planes), and `list.cam_bytes_per_image`, the planes' share;
  * `list.images_per_s_plain` / `images_per_s_crf`: `ListImageSource(with_cams=...)` over PNG + CAM files in a temporary
    directory through `pseudo_labels_cam` / `pseudo_labels_cam_crf` with a STAND-IN for the embedding network (a 3 -> 32
    channel mix of the view: the backbone is not what this tool times) and the real affinity, walk, up-sampling, CRF and
    export.
Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NCLS, ALPHA = 21, 6


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def make_source(h, w, classes, seed=1):
  """-> (rgb, semantic label, CAM dict {class - 1: [h, w] fp32}) of one made-up file."""
  rng = np.random.RandomState(seed)
  cell = lambda values: np.asarray(values)[rng.randint(0, len(values), (h // 32 + 1, w // 32 + 1))][
      np.arange(h)[:, None] // 32, np.arange(w)[None] // 32]
  rgb = np.clip(cell(range(200))[..., None] + rng.randint(0, 56, (h, w, 3)), 0, 255).astype(np.uint8)
  semantic = cell([0] + list(classes)).astype(np.uint8)
  cam = {c - 1: (0.15 + 0.7 * (semantic == c) + 0.1 * rng.rand(h, w)).astype(np.float32) for c in classes}
  return rgb, semantic, cam


class StandInEmbedding(torch.nn.Module):
  """`generate_embeddings` of the embedding networks, as a 3 -> 32 channel mix at the input's size."""

  def __init__(self, device):
    super().__init__()
    self.mix = torch.nn.Parameter(torch.from_numpy(np.random.RandomState(5).randn(32, 3).astype(np.float32)).to(device))

  def generate_embeddings(self, datas, resize_as_input=True):
    return {'embedding': torch.einsum('kc,nchw->nkhw', self.mix, datas['image'])}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--classes', type=int, nargs='+', default=[3, 7, 15])
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--repeats', type=int, default=50)
  ap.add_argument('--files', type=int, default=16)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_cam_lists needs an MI355X (no CPU fallback)')
  from PIL import Image
  from spml_amd import _ffi, inference, inference_cli
  dev = torch.device('cuda', 0)
  (h, w), crop = a.image, (a.crop, a.crop)
  _, _, cam = make_source(h, w, a.classes)
  keys = list(cam.keys())
  planes = torch.from_numpy(np.stack(list(cam.values()))).to(dev)
  cam_dev = {k: planes[i] for i, k in enumerate(keys)}
  res = {'image': [h, w], 'classes': NCLS, 'planes': len(keys), 'path': _ffi.cam_ingest_path_name(len(keys), h, w, NCLS)}

  # the ingest: one launch against the framework chain on the same device planes
  hip = lambda: _ffi.cam_ingest(planes, keys, (h, w), NCLS, ALPHA)
  framework = lambda: inference.downsampled_cam(inference.cam_with_background(cam_dev, (h, w), NCLS, ALPHA))
  t_hip, t_framework, got = [], [], None
  for it in range(a.warmup + a.repeats):
    x, first = timed(hip)
    y, second = timed(framework)
    got = (first, second)
    if it >= a.warmup:
      t_hip.append(x)
      t_framework.append(y)
  res['ingest'] = {'hip_ms': spread(t_hip), 'framework_ms': spread(t_framework),
                   'framework_over_hip': round(statistics.median(t_framework) / statistics.median(t_hip), 2),
                   'max_abs_diff': float((got[0] - got[1]).abs().max())}

  # a list of PNG + CAM files through ListImageSource and the two API functions
  with tempfile.TemporaryDirectory() as tmp:
    lines = []
    for sub in ('img', 'lab', 'cam'):
      os.makedirs(os.path.join(tmp, sub))
    for k in range(a.files):
      f_rgb, f_sem, f_cam = make_source(h, w, a.classes, seed=10 + k)
      Image.fromarray(f_rgb).save(os.path.join(tmp, 'img', '%04d.png' % k), compress_level=1)
      Image.fromarray(f_sem).save(os.path.join(tmp, 'lab', '%04d.png' % k), compress_level=1)
      np.save(os.path.join(tmp, 'cam', '%04d.npy' % k), f_cam)
      lines.append('img/%04d.png lab/%04d.png lab/%04d.png' % (k, k, k))
    with open(os.path.join(tmp, 'val.txt'), 'w') as f:
      f.write('\n'.join(lines) + '\n')
    config = types.SimpleNamespace(
        num_threads=4, dataset=types.SimpleNamespace(num_classes=NCLS, data_dir='', color_map_path='', semantic_ignore_index=255),
        network=types.SimpleNamespace(pixel_means=MEAN, pixel_stds=STD),
        test=types.SimpleNamespace(crop_size=list(crop), stride=list(crop), image_size=0))
    args = types.SimpleNamespace(data_dir=tmp, data_list=os.path.join(tmp, 'val.txt'), save_dir=os.path.join(tmp, 'out'),
                                 crf_iter_max=10, crf_pos_xy_std=1, crf_pos_w=3, crf_bi_xy_std=67, crf_bi_rgb_std=3, crf_bi_w=4)
    network = StandInEmbedding(dev)
    rates, uploads, fields = {}, [], {}
    for with_crf in (False, True, False, True):             # the first pair warms the page cache and the allocators
      source = inference_cli.ListImageSource(config, args, dev, [1], True, 'pseudo_labels_cam', with_guide=with_crf,
                                             with_cams=os.path.join(tmp, 'cam'))
      stage = inference_cli.CrfStage(config, args) if with_crf else None
      gray_dir = inference_cli.output_dir(args, 'semantic_gray')
      plain_stage = source._stage

      def recording_stage(nbytes):
        uploads.append(nbytes)
        return plain_stage(nbytes)
      source._stage = recording_stage

      def one(image):
        if stage is None:
          out = inference.pseudo_labels_cam(network, image.views, image.image_hw, image.cam_planes, image.cam_classes, NCLS)
          source.emit(image, out['semantic_prediction'], gray_dir)
        else:
          out = inference.pseudo_labels_cam_crf(network, image.views, image.image_hw, image.cam_planes, image.cam_classes,
                                                NCLS, image.guide, stage)
          source.emit_refined(image, out['semantic_prediction'], out['semantic_prediction_before_crf'], gray_dir)
      done, seconds = source.timed(one)
      rates[with_crf] = done / seconds
      if stage is not None:
        fields = dict(source.crf_fields(), **stage.fields(seconds))
    res['list'] = dict(fields, images_per_s_plain=round(rates[False], 2), images_per_s_crf=round(rates[True], 2),
                       upload_bytes_per_image=int(statistics.median(uploads)), cam_bytes_per_image=4 * len(keys) * h * w,
                       files=a.files, network='stand-in (3 -> 32 channel mix of the view)')
  print(json.dumps(res))


if __name__ == '__main__':
  main()
