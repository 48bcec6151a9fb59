#!/usr/bin/env python3
"""Timing of the training data path (spml_amd/data, csrc/augment.hip) at the recipe's shape: batch 16, crop
513 x 513, sources 375 x 500, random mirror and random scale (0.5 - 1.5) on, the blur off and on (sigma 2 on every image).

Prints one JSON line:
  * `hip_ms`: ms per batch of the two launches (`spml_augment_batch_u8`, `spml_augment_tags_u8`; device events);
  * `framework_ms`: the same stages as framework ops on the device, from the same uploaded bytes (per image: / 255, flip,
    `F.interpolate` bilinear / nearest, pad, slice, grouped `conv2d` over a reflect pad, normalise; stack, `.long()`,
    `scatter_` for the tags), and the largest difference between the two results;
  * `host_ms_1_thread`, `host_ms_16_threads`: the reference's chain as numpy on the host up to the collated tensors --
    with PIL's resize STANDING IN for cv2.resize (cv2 is not installed; PIL's bilinear filter also anti-aliases when it
    shrinks, so this is a stand-in for the cost, not for the values) and the blur as 25 shifted numpy adds;
  * `upload_bytes`: per batch, raw bytes + records against the finished fp32 image + two int64 maps;
  * `batcher_images_per_s`: `DeviceBatcher` over in-memory PNGs, 16 decode threads, whole batches until the device is idle.
Needs an MI355X: there is no fallback."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def make_sources(n, h, w, seed=1):
  rng = np.random.RandomState(seed)
  out = []
  for _ in range(n):
    cell = lambda hi: rng.randint(0, hi, (h // 32 + 1, w // 32 + 1))[np.arange(h)[:, None] // 32, np.arange(w)[None] // 32]
    rgb = np.clip(cell(200)[..., None] + rng.randint(0, 56, (h, w, 3)), 0, 255).astype(np.uint8)
    sem = cell(21).astype(np.uint8)
    sem[:, :8] = 255
    out.append((rgb, sem, cell(6).astype(np.uint8)))
  return out


def framework_batch(packed, records, mean, std, size, device):
  """The stages of csrc/augment.hip as framework ops on the device, image by image."""
  images, sems, insts = [], [], []
  tags = torch.zeros((len(records), 256), dtype=torch.int64, device=device)
  for k, r in enumerate(records):
    h, w, nh, nw = int(r['h']), int(r['w']), int(r['new_h']), int(r['new_w'])
    rgb = packed[int(r['image_off']):int(r['image_off']) + 3 * h * w].view(h, w, 3)
    lab = torch.stack([packed[int(r[o]):int(r[o]) + h * w].view(h, w) for o in ('sem_off', 'inst_off')])
    tags[k].scatter_(0, lab[0].reshape(-1).long(), 1)
    img = rgb.permute(2, 0, 1).float() / 255
    if r['flip']:
      img, lab = img.flip(2), lab.flip(2)
    img = F.interpolate(img[None], size=(nh, nw), mode='bilinear', align_corners=False)[0]
    lab = F.interpolate(lab[None].float(), size=(nh, nw), mode='nearest')[0]
    ph, pw = max(nh, size[0]), max(nw, size[1])
    canvas = mean.view(3, 1, 1).expand(3, ph, pw).clone()
    canvas[:, :nh, :nw] = img
    lcanvas = torch.full((2, ph, pw), 255.0, device=device)
    lcanvas[:, :nh, :nw] = lab
    sh, sw = int(r['start_h']), int(r['start_w'])
    img = canvas[:, sh:sh + size[0], sw:sw + size[1]]
    lab = lcanvas[:, sh:sh + size[0], sw:sw + size[1]]
    if r['gray']:
      img = ((img[0] * 0.3 + img[1] * 0.59) + img[2] * 0.11).expand(3, -1, -1)
    if r['blur']:
      k5 = torch.from_numpy(np.ascontiguousarray(r['weights'])).to(device).view(1, 1, 5, 5).expand(3, 1, 5, 5)
      img = F.conv2d(F.pad(img[None], (2, 2, 2, 2), mode='reflect'), k5, groups=3)[0]
    images.append((img - mean.view(3, 1, 1)) / std.view(3, 1, 1))
    sems.append(lab[0])
    insts.append(lab[1])
  return torch.stack(images), torch.stack(sems).long(), torch.stack(insts).long(), tags


def host_sample(sample, plan, size):
  """base_dataset.py:135-155,183-186 (+ list_tag_dataset.py:207-213) on the host; PIL's resize stands in for cv2's."""
  from PIL import Image
  rgb, sem, inst = sample
  image = rgb.astype(np.float32) / 255
  label = np.stack([sem, inst], axis=2)
  if plan['flip']:
    image, label = image[:, ::-1], label[:, ::-1]
  nh, nw = plan['new_h'], plan['new_w']
  image = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(image[..., c]), mode='F').resize((nw, nh), Image.BILINEAR))
                    for c in range(3)], axis=2)
  label = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(label[..., c])).resize((nw, nh), Image.NEAREST))
                    for c in range(2)], axis=2)
  ph, pw = max(nh, size[0]), max(nw, size[1])
  canvas = np.empty((ph, pw, 3), np.float32)
  canvas[:] = np.array(MEAN, np.float32)
  canvas[:nh, :nw] = image
  lcanvas = np.full((ph, pw, 2), 255, np.uint8)
  lcanvas[:nh, :nw] = label
  sh, sw = plan['start_h'], plan['start_w']
  image = canvas[sh:sh + size[0], sw:sw + size[1]]
  label = lcanvas[sh:sh + size[0], sw:sw + size[1]]
  if plan['blur']:
    padded = np.pad(image, ((2, 2), (2, 2), (0, 0)), mode='reflect')
    weight = plan['weights'].reshape(5, 5)
    out = np.zeros_like(image)
    for i in range(5):
      for j in range(5):
        out += weight[i, j] * padded[i:i + size[0], j:j + size[1]]
    image = out
  image = (image - np.array(MEAN, np.float32)) / np.array(STD, np.float32)
  tags = np.zeros((256,), np.uint8)
  tags[np.unique(sem)] = 1
  return image.transpose(2, 0, 1), label[..., 0], label[..., 1], tags


def host_batch(samples, plans, size, pool):
  parts = list((pool.map if pool else map)(lambda sp: host_sample(sp[0], sp[1], size), zip(samples, plans)))
  image = torch.from_numpy(np.stack([p[0] for p in parts]))                    # base_dataset.py:192-223
  labels = [torch.from_numpy(np.stack([p[k] for p in parts])).long() for k in (1, 2, 3)]
  return image, labels


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--host_repeats', type=int, default=3)
  ap.add_argument('--batcher_batches', type=int, default=20)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_data_pipeline needs an MI355X (no CPU fallback)')
  from PIL import Image
  from spml_amd import ops
  from spml_amd.data import DeviceBatcher, batcher, transforms
  from spml_amd.data.datasets import ListTagDataset
  dev = torch.device('cuda', 0)
  size = (a.crop, a.crop)
  h, w = a.image
  samples = make_sources(a.batch, h, w)
  mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
  remap = torch.arange(256, dtype=torch.uint8, device=dev)
  res = {'batch': a.batch, 'crop': a.crop, 'image': [h, w], 'scale_range': [0.5, 1.5]}
  for blur in (False, True):
    plans = [transforms.plan_training(transforms.sample_rng(235, 0, k), h, w, size, True, True, True, (0.5, 1.5))
             for k in range(a.batch)]
    if blur:
      for p in plans:
        p['blur'], p['weights'] = True, transforms.blur_weights(2.0).reshape(25).astype(np.float32)
    full = [s + (p, k) for k, (s, p) in enumerate(zip(samples, plans))]
    _, total = batcher.packed_layout(full)
    stage = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    records = batcher.pack(full, stage.numpy())
    packed = stage.to(dev)
    params_dev = packed[:records.size * records.dtype.itemsize]
    out = ops.augment_batch(packed, records, mean, std, remap, size, params_dev=params_dev)
    tag_out = ops.augment_tags(packed, records, params_dev=params_dev)

    def hip():
      ops.augment_batch(packed, records, mean, std, remap, size, params_dev=params_dev, out=out)
      return ops.augment_tags(packed, records, params_dev=params_dev, out=tag_out)

    def framework():
      return framework_batch(packed, records, mean, std, size, dev)

    th, tf = [], []
    for it in range(a.warmup + a.repeats):
      t0, _ = timed(hip)
      t1, fw = timed(framework)
      if it >= a.warmup:
        th.append(t0)
        tf.append(t1)
    entry = {'hip_ms': spread(th), 'framework_ms': spread(tf),
             'framework_over_hip': round(statistics.median(tf) / statistics.median(th), 2),
             'max_abs_diff_image': (fw[0] - out[0]).abs().max().item(),
             'labels_equal': bool(torch.equal(fw[1], out[1]) and torch.equal(fw[2], out[2]) and torch.equal(fw[3], tag_out))}
    for threads in (1, 16):
      pool = ThreadPoolExecutor(max_workers=threads) if threads > 1 else None
      times = []
      for it in range(1 + a.host_repeats):
        t0 = time.perf_counter()
        host_batch(samples, plans, size, pool)
        if it:
          times.append((time.perf_counter() - t0) * 1e3)
      if pool:
        pool.shutdown()
      entry['host_ms_%d_thread%s' % (threads, 's' if threads > 1 else '')] = spread(times)
    entry['upload_bytes'] = {'raw_and_records': int(total), 'finished_batch': a.batch * a.crop * a.crop * (12 + 16)}
    res['blur_on' if blur else 'blur_off'] = entry
  res['host_resize_is_a_stand_in'] = 'PIL.Image.resize in the place of cv2.resize'

  # the batcher end to end: PNG bytes in memory, 16 decode threads
  def png(arr):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format='PNG', compress_level=1)
    return buf.getvalue()
  blobs = [tuple(png(x) for x in s) for s in samples]

  class InMemory(ListTagDataset):
    def _read_image_and_label_paths(self, data_dir, data_list):
      names = ['memory/%d' % k for k in range(len(blobs))]
      return names, names, names

    def _get_datas_by_index(self, idx):
      image, sem, inst = blobs[idx]
      return (np.array(Image.open(io.BytesIO(image)).convert(mode='RGB')),
              np.array(Image.open(io.BytesIO(sem)).convert(mode='L')),
              np.array(Image.open(io.BytesIO(inst)).convert(mode='L')))

  ds = InMemory('', '', img_mean=MEAN, img_std=STD, size=size, random_crop=True, random_scale=True, random_mirror=True,
                training=True)
  loader = DeviceBatcher(ds, a.batch, dev, num_threads=16)
  for _ in range(2):
    next(loader)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(a.batcher_batches):
    next(loader)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  loader.close()
  res['batcher_images_per_s'] = round(a.batcher_batches * a.batch / dt, 1)
  res['batcher_ms_per_batch'] = round(dt / a.batcher_batches * 1e3, 2)
  res['png_bytes_per_image'] = int(sum(len(b) for s in blobs for b in s) / len(blobs))
  print(json.dumps(res))


if __name__ == '__main__':
  main()
