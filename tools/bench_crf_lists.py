#!/usr/bin/env python3
"""Timing of the denseCRF stage of a program that reads image files (csrc/inference_io.hip) at the recipe's
shape: a 375 x 500 source, 21 classes, the single-view programs' guide at 320 x 426 (`test.image_size` 427 would give
that ratio; any size off the source's takes the same path).

Prints one JSON line (device events, medians over `--repeats` after `--warmup`):
  * `guide.table_ms` / `guide.resized_ms`: the one launch of `spml_crf_guide_u8` on either path;
    `guide.framework_table_ms` / `guide.framework_resized_ms`: `inference.denormalized_uint8` (framework ops) on the
    device view of the same size, which is what the programs ran before; `equal`: the two are the same bytes;
  * `export.scored_ms`: the one launch of `spml_label_export_scored_u8` from two padded 513 x 513 label maps;
    `export.separate_ms`: `export_label_map` twice, `metrics.iou_stats` twice and the compare (`!=`, `sum`, `add_`), what
    `SyntheticImageSource.emit_refined` runs per image plus the second export a list needs; `equal`: same tables;
  * `list.images_per_s_crf` / `images_per_s_plain`: `ListImageSource` over PNG files in a temporary directory with a
    STAND-IN for the network (a soft-max over channel differences of the first view: the backbone is not what this tool
    times), with the guide, the real `DenseCRF` and `emit_refined` against the same loop with `emit` alone;
    `list.crf_share`: the CRF's share of the timed seconds, `list.crf_ms_per_image`.
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
NCLS = 21


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def make_source(h, w, seed=1):
  rng = np.random.RandomState(seed)
  cell = lambda hi: rng.randint(0, hi, (h // 32 + 1, w // 32 + 1))[np.arange(h)[:, None] // 32, np.arange(w)[None] // 32]
  rgb = np.clip(cell(200)[..., None] + rng.randint(0, 56, (h, w, 3)), 0, 255).astype(np.uint8)
  return rgb, cell(NCLS).astype(np.uint8)


def alternate(first, second, warmup, repeats):
  t0, t1, out = [], [], None
  for it in range(warmup + repeats):
    a, x = timed(first)
    b, y = timed(second)
    out = (x, y)
    if it >= warmup:
      t0.append(a)
      t1.append(b)
  return t0, t1, out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--resized', type=int, nargs=2, default=[320, 426])
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--repeats', type=int, default=50)
  ap.add_argument('--files', type=int, default=16)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_crf_lists needs an MI355X (no CPU fallback)')
  from PIL import Image
  from spml_amd import _ffi, inference, inference_cli
  from spml_amd.data import transforms
  from spml_amd.utils.general import metrics, vis
  dev = torch.device('cuda', 0)
  (h, w), new_hw, crop = a.image, tuple(a.resized), (a.crop, a.crop)
  rgb, semantic = make_source(h, w)
  rgb_dev, sem_dev = torch.from_numpy(rgb).to(dev), torch.from_numpy(semantic).to(dev)
  res = {'image': [h, w], 'resized': list(new_hw), 'classes': NCLS}

  # the guide: one launch against denormalized_uint8 on the device view of the same size
  def view_of(hw):
    plan = [dict(image_off=0, label_off=0, new_h=hw[0], new_w=hw[1], pad_h=hw[0], pad_w=hw[1], flip=0)]
    records = inference.view_records(plan)
    params_dev = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).to(dev)
    mean, std = inference._normalisation(dev, MEAN, STD)
    return inference.views_from_records(rgb_dev, records, params_dev, mean, std)[0][0][0]
  res['guide'] = {'paths': [_ffi.crf_guide_path_name((h, w)), _ffi.crf_guide_path_name((h, w), new_hw)]}
  for key, hw in (('table', (h, w)), ('resized', new_hw)):
    view = view_of(hw)
    hip, framework, (got, want) = alternate(lambda: inference.crf_guide(rgb_dev, MEAN, STD, hw),
                                            lambda: inference.denormalized_uint8(view, MEAN, STD), a.warmup, a.repeats)
    res['guide'].update({key + '_ms': spread(hip), 'framework_' + key + '_ms': spread(framework),
                         key + '_framework_over_hip': round(statistics.median(framework) / statistics.median(hip), 2),
                         key + '_equal': bool(torch.equal(got, want))})

  # the scored export: one launch against two exports, two score calls and the compare
  table = torch.from_numpy(vis.voc_color_map()).to(dev)
  rng = np.random.RandomState(3)
  before = torch.from_numpy(rng.randint(0, NCLS, crop).astype(np.int64)).to(dev)
  refined = torch.where(torch.from_numpy(rng.rand(*crop) < 0.1).to(dev), (before + 1) % NCLS, before)
  valid = (min(h, a.crop), min(w, a.crop))
  scores = torch.zeros((2 * 3 * NCLS + 1,), dtype=torch.int64, device=dev)
  counts = [torch.zeros((3, NCLS), dtype=torch.int64, device=dev) for _ in range(2)]
  changed = torch.zeros((), dtype=torch.int64, device=dev)

  def separate():
    gray, _ = inference.export_label_map(refined, valid, (h, w), table)
    gray_before, _ = inference.export_label_map(before, valid, (h, w), table)
    metrics.iou_stats(gray, sem_dev, NCLS, counts[0])
    metrics.iou_stats(gray_before, sem_dev, NCLS, counts[1])
    changed.add_((gray != gray_before).sum())
  fused = lambda: inference.export_scored_label_map(refined, before, valid, (h, w), table, sem_dev, NCLS, scores)
  t_fused, t_separate, _ = alternate(fused, separate, a.warmup, a.repeats)
  res['export'] = {'scored_ms': spread(t_fused), 'separate_ms': spread(t_separate),
                   'separate_over_scored': round(statistics.median(t_separate) / statistics.median(t_fused), 2),
                   'equal': bool(torch.equal(scores[:-1].view(2, 3, NCLS), torch.stack(counts)) and int(scores[-1]) == int(changed))}

  # a list of PNG files through ListImageSource: guide + denseCRF + scored export against the plain loop
  with tempfile.TemporaryDirectory() as tmp:
    lines = []
    os.makedirs(os.path.join(tmp, 'img'))
    os.makedirs(os.path.join(tmp, 'lab'))
    for k in range(a.files):
      f_rgb, f_sem = make_source(h, w, seed=10 + k)
      Image.fromarray(f_rgb).save(os.path.join(tmp, 'img', '%04d.png' % k), compress_level=1)
      Image.fromarray(f_sem).save(os.path.join(tmp, 'lab', '%04d.png' % k), compress_level=1)
      lines.append('img/%04d.png lab/%04d.png lab/%04d.png' % (k, k, k))
    with open(os.path.join(tmp, 'val.txt'), 'w') as f:
      f.write('\n'.join(lines) + '\n')
    config = types.SimpleNamespace(
        num_threads=4, dataset=types.SimpleNamespace(num_classes=NCLS, data_dir='', color_map_path='', semantic_ignore_index=255),
        network=types.SimpleNamespace(pixel_means=MEAN, pixel_stds=STD),
        test=types.SimpleNamespace(crop_size=list(crop), stride=list(crop), image_size=0))
    args = types.SimpleNamespace(data_dir=tmp, data_list=os.path.join(tmp, 'val.txt'), save_dir=os.path.join(tmp, 'out'),
                                 crf_iter_max=10, crf_pos_xy_std=1, crf_pos_w=3, crf_bi_xy_std=67, crf_bi_rgb_std=3, crf_bi_w=4)
    weights = torch.from_numpy(np.random.RandomState(5).randn(NCLS, 3).astype(np.float32)).to(dev)

    def stand_in(image):
      logits = torch.einsum('kc,chw->khw', weights, image.views[0][0][0, :, :h, :w])
      return torch.softmax(logits, dim=0).contiguous()
    rates, shares, crf_ms = {}, None, None
    for with_crf in (False, True, False, True):             # the first pair warms the page cache and the allocators
      source = inference_cli.ListImageSource(config, args, dev, [1], False, 'predict_softmax_multiscale', with_guide=with_crf)
      stage = inference_cli.CrfStage(config, args) if with_crf else None
      gray_dir = inference_cli.output_dir(args, 'semantic_gray')

      def one(image):
        prob = stand_in(image)
        if stage is None:
          source.emit(image, prob.argmax(0), gray_dir)
        else:
          source.emit_refined(image, stage(image.guide, prob)['semantic_prediction'], prob.argmax(0), gray_dir)
      done, seconds = source.timed(one)
      rates[with_crf] = done / seconds
      if stage is not None:
        fields = stage.fields(seconds)
        shares, crf_ms = fields['crf_share'], fields['crf_share'] * seconds * 1e3 / done
        res['list'] = dict(source.crf_fields(), crf_path=fields['crf_path'])
    res['list'].update({'images_per_s_crf': round(rates[True], 2), 'images_per_s_plain': round(rates[False], 2),
                        'crf_share': shares, 'crf_ms_per_image': round(crf_ms, 2), 'files': a.files,
                        'network': 'stand-in (3 -> 21 channel mix of the view + soft-max)'})
  print(json.dumps(res))


if __name__ == '__main__':
  main()
