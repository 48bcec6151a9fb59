#!/usr/bin/env python3
"""Timing of the two ends of an inference program that reads image files (csrc/inference_io.hip) at the
recipe's shape: a 375 x 500 source, crop 513 x 513, scales 0.5, 0.75, 1, 1.25, 1.5 each flipped and plain (ten views).

Prints one JSON line:
  * `views.hip_ms`: ms of the one launch that writes all ten views and their labels (`spml_image_views_u8`; device
    events), `views.store_gb_per_s`: the bytes it must store over that time;
  * `views.framework_ms`: the same stages as framework ops on the device from the same uploaded bytes (normalise once,
    then per view `F.interpolate` bilinear / nearest, flip, zero canvas + copy), and the largest difference;
  * `views.host_ms`: the reference's chain as numpy on the host up to the ten finished fp32 views -- with PIL's resize
    STANDING IN for cv2.resize (cv2 is not installed; PIL's bilinear filter also anti-aliases when it shrinks, so this
    is a stand-in for the cost, not for the values) -- and `views.host_upload_ms`: the ten views going up from pinned
    memory; `views.raw_upload_ms`: the decoded bytes going up;
  * `views.upload_bytes`: raw bytes + records against the finished views;
  * `export.hip_ms`: the one launch from a padded 513 x 513 prediction to gray + colour bytes at 375 x 500
    (`spml_label_export_u8`) plus the copy of the 4 bytes per pixel to pinned memory; `export.framework_ms`: crop,
    nearest `F.interpolate`, table lookup on the device plus the same copy; `export.host_ms`: the reference's route (the
    padded int64 map copied down, cropped, resized, coloured with numpy; PIL's nearest resize standing in);
    `export.launch_ms_table_in_cache` / `launch_ms_table_in_lds`: the launch alone, in the product library and in the
    other build of csrc/inference_io.hip (-DSPML_EXPORT_TABLE_LDS=1; `spml_amd._build.build_variant` makes that library),
    alternating;
  * `decode_ahead_images_per_s`: `ListImageSource` over PNG files in a temporary directory, views made and label maps
    exported and written, with a stand-in for the network (the arg-max of the first view's channels).
Needs an MI355X: there is no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALES = [0.5, 0.75, 1, 1.25, 1.5]


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
  return rgb, cell(21).astype(np.uint8)


def framework_views(rgb, semantic, plan, mean, std):
  """The stages of `spml_image_views_u8` as framework ops on the device."""
  image = ((rgb.permute(2, 0, 1).float() / 255 - mean.view(3, 1, 1)) / std.view(3, 1, 1))[None]
  label = semantic[None, None].float()
  views, labels = [], []
  for p in plan:
    size = (p['new_h'], p['new_w'])
    img = F.interpolate(image, size=size, mode='bilinear', align_corners=False)
    lab = F.interpolate(label, size=size, mode='nearest')[0, 0].long()
    if p['flip']:
      img, lab = img.flip(3), lab.flip(1)
    canvas = torch.zeros((1, 3, p['pad_h'], p['pad_w']), dtype=torch.float32, device=rgb.device)
    canvas[:, :, :size[0], :size[1]] = img
    views.append(canvas)
    labels.append(lab.contiguous())
  return views, labels


def host_views(rgb, plan):
  """base_dataset.py (normalise) + create_image_pyramid + resize_with_pad on the host; PIL's resize stands in for cv2's."""
  from PIL import Image
  image = (rgb.astype(np.float32) / 255 - np.array(MEAN, np.float32)) / np.array(STD, np.float32)
  out = []
  for p in plan:
    nh, nw = p['new_h'], p['new_w']
    img = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(image[..., c]), mode='F').resize((nw, nh), Image.BILINEAR))
                    for c in range(3)], axis=2)
    if p['flip']:
      img = img[:, ::-1]
    canvas = np.zeros((p['pad_h'], p['pad_w'], 3), np.float32)
    canvas[:nh, :nw] = img
    out.append(torch.from_numpy(np.ascontiguousarray(canvas.transpose(2, 0, 1)[None])))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--repeats', type=int, default=50)
  ap.add_argument('--host_repeats', type=int, default=5)
  ap.add_argument('--files', type=int, default=64)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_inference_io needs an MI355X (no CPU fallback)')
  from PIL import Image
  from spml_amd import _build, _ffi, inference, inference_cli
  from spml_amd.data import transforms
  from spml_amd.utils.general import vis
  dev = torch.device('cuda', 0)
  crop, (h, w) = (a.crop, a.crop), a.image
  rgb, semantic = make_source(h, w)
  plan = transforms.plan_views(h, w, SCALES, True, crop)
  records = inference.view_records(plan)
  image_bytes, label_bytes = transforms.view_buffer_bytes(plan)
  mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
  raw = np.concatenate([records.view(np.uint8).reshape(-1), rgb.reshape(-1), semantic.reshape(-1)])
  stage = torch.from_numpy(raw).pin_memory()
  packed = stage.to(dev)
  params_dev = packed[:records.nbytes]
  rgb_dev = packed[records.nbytes:records.nbytes + 3 * h * w].view(h, w, 3)
  sem_dev = packed[records.nbytes + 3 * h * w:].view(h, w)
  images = torch.empty((image_bytes // 4,), dtype=torch.float32, device=dev)
  labels = torch.empty((label_bytes // 8,), dtype=torch.int64, device=dev)
  res = {'image': [h, w], 'crop': a.crop, 'scales': SCALES, 'views': {}, 'export': {}}

  hip = lambda: _ffi.image_views(rgb_dev, sem_dev, records, params_dev, mean, std, images, labels)
  framework = lambda: framework_views(rgb_dev, sem_dev, plan, mean, std)
  th, tf = [], []
  for it in range(a.warmup + a.repeats):
    t0, _ = timed(hip)
    t1, fw = timed(framework)
    if it >= a.warmup:
      th.append(t0)
      tf.append(t1)
  views, label_views = inference.views_from_records(rgb_dev, records, params_dev, mean, std, sem_dev)
  stored = sum(12 * p['pad_h'] * p['pad_w'] + 8 * p['new_h'] * p['new_w'] for p in plan)
  host_times, upload_times, raw_times = [], [], []
  for it in range(1 + a.host_repeats):
    t0 = time.perf_counter()
    finished = host_views(rgb, plan)
    if it:
      host_times.append((time.perf_counter() - t0) * 1e3)
    pinned = [v.pin_memory() for v in finished]
    t, _ = timed(lambda: [v.to(dev, non_blocking=True) for v in pinned])
    t_raw, _ = timed(lambda: stage.to(dev, non_blocking=True))
    if it:
      upload_times.append(t)
      raw_times.append(t_raw)
  res['views'] = {
      'hip_ms': spread(th), 'framework_ms': spread(tf),
      'framework_over_hip': round(statistics.median(tf) / statistics.median(th), 2),
      'stored_bytes': int(stored), 'store_gb_per_s': round(stored / (statistics.median(th) * 1e-3) / 1e9, 1),
      'max_abs_diff_image': max((f - v[0]).abs().max().item() for f, v in zip(fw[0], views)),
      'labels_equal': all(torch.equal(f, l) for f, l in zip(fw[1], label_views)),
      'host_ms': spread(host_times), 'host_upload_ms': spread(upload_times), 'raw_upload_ms': spread(raw_times),
      'upload_bytes': {'raw_and_records': int(raw.size), 'finished_views': int(sum(12 * p['pad_h'] * p['pad_w'] for p in plan))},
      'host_resize_is_a_stand_in': 'PIL.Image.resize in the place of cv2.resize'}

  # the export: a padded 513 x 513 prediction whose valid rectangle is the 375 x 500 image
  table = torch.from_numpy(vis.voc_color_map()).to(dev)
  table_host = vis.voc_color_map()
  pred = torch.from_numpy(np.random.RandomState(3).randint(0, 21, crop).astype(np.int64)).to(dev)
  valid = (min(h, a.crop), min(w, a.crop))
  out = torch.empty((4 * h * w,), dtype=torch.uint8, device=dev)
  gray, color = out[:h * w].view(h, w), out[h * w:].view(h, w, 3)
  host_out = torch.empty((4 * h * w,), dtype=torch.uint8, pin_memory=True)

  def hip_export():
    inference.export_label_map(pred, valid, (h, w), table, out=(gray, color))
    host_out.copy_(out, non_blocking=True)

  def framework_export():
    g = F.interpolate(pred[None, None, :valid[0], :valid[1]].float(), size=(h, w), mode='nearest')[0, 0].to(torch.uint8)
    both = torch.cat([g.reshape(-1), table[g.long()].reshape(-1)])
    host_out.copy_(both, non_blocking=True)
    return g

  def host_export():
    p = pred.cpu().numpy().astype(np.uint8)[:valid[0], :valid[1]]
    g = np.asarray(Image.fromarray(p).resize((w, h), Image.NEAREST))
    return g, table_host[g]
  th, tf, tc = [], [], []
  for it in range(a.warmup + a.repeats):
    t0, _ = timed(hip_export)
    t1, g = timed(framework_export)
    torch.cuda.synchronize()
    c0 = time.perf_counter()
    host_export()
    c1 = time.perf_counter()
    if it >= a.warmup:
      th.append(t0)
      tf.append(t1)
      tc.append((c1 - c0) * 1e3)
  # the table through the cache (the product library) against the table staged in LDS (the other build), launch alone
  other = ctypes.CDLL(_build.build_variant('inference_io.hip', ['SPML_EXPORT_TABLE_LDS=1'], 'spml_export_table_lds',
                                           verbose=False))
  other.spml_label_export_u8.restype, other.spml_label_export_u8.argtypes = _ffi._SIGNATURES['spml_label_export_u8']
  lds_out = torch.empty_like(out)

  def launch(lib, buf):
    _ffi.check(lib.spml_label_export_u8(_ffi.ptr(pred, torch.int64), a.crop, a.crop, valid[0], valid[1], h, w,
                                        _ffi.ptr(table, torch.uint8), _ffi.ptr(buf[:h * w]), _ffi.ptr(buf[h * w:]),
                                        _ffi.stream_ptr()), 'spml_label_export_u8')
  t_cache, t_lds = [], []
  for it in range(a.warmup + a.repeats):
    t0, _ = timed(lambda: launch(_ffi.lib(), out))
    t1, _ = timed(lambda: launch(other, lds_out))
    if it >= a.warmup:
      t_cache.append(t0)
      t_lds.append(t1)
  if not torch.equal(out, lds_out):
    raise SystemExit('the two builds of label_export disagree')
  res['export'] = {'hip_ms': spread(th), 'framework_ms': spread(tf), 'host_ms': spread(tc),
                   'launch_ms_table_in_cache': spread(t_cache), 'launch_ms_table_in_lds': spread(t_lds),
                   'framework_over_hip': round(statistics.median(tf) / statistics.median(th), 2),
                   'gray_equal': bool(torch.equal(g, gray)),
                   'download_bytes': {'gray_and_colour': 4 * h * w, 'padded_int64_prediction': 8 * a.crop * a.crop}}

  # decode ahead: PNG files -> views -> (stand-in network) -> export -> PNG files
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
        num_threads=4, dataset=types.SimpleNamespace(num_classes=21, data_dir='', color_map_path='', semantic_ignore_index=255),
        network=types.SimpleNamespace(pixel_means=MEAN, pixel_stds=STD),
        test=types.SimpleNamespace(crop_size=list(crop), stride=list(crop), image_size=0))
    args = types.SimpleNamespace(data_dir=tmp, data_list=os.path.join(tmp, 'val.txt'), save_dir=os.path.join(tmp, 'out'))
    rates = []
    for _ in range(2):                                    # the first pass warms the page cache and the allocators
      source = inference_cli.ListImageSource(config, args, dev, SCALES, True, 'predict_softmax_multiscale')
      gray_dir = inference_cli.output_dir(args, 'semantic_gray')

      def one(image):
        stand_in = image.views[4][0][0, :, :h, :w].argmax(0)
        source.emit(image, stand_in, gray_dir)
      done, seconds = source.timed(one)
      rates.append(done / seconds)
    res['decode_ahead_images_per_s'] = round(rates[-1], 1)
    res['decode_ahead_files'] = a.files
    res['decode_ahead_threads'] = 4
  print(json.dumps(res))


if __name__ == '__main__':
  main()
