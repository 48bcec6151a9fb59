#!/usr/bin/env python3
"""Timing of the random-walk pseudo labels with denseCRF refinement (pyscripts/inference/pseudo_softmaxrw_crf.py,
spml_amd.inference.pseudo_labels_softmax_crf) on one synthetic 375 x 500 image padded to 513 x 513:
ResNet-101 DeepLab-v2, C = 64, 21 classes, the flip pair at scale 1, 6 squarings, 10 CRF iterations.

Prints one JSON line:
  * ms per image (device events over whole calls of `pseudo_labels_softmax_crf`);
  * ms of the CRF tail alone (`random_walk_crf_refine` on the image's walked maps: prepare + the fused call) and its share
    of the image time;
  * the init stage both ways on identical device inputs, alternated in this process: the fused launch
    (`spml_dense_crf_infer_upsampled_f32` with no iteration: memset + crf_init_upsampled) against the framework ops
    feeding the existing entry (`F.interpolate` + `argmax`, then `spml_dense_crf_infer_f32` with no iteration: memset +
    crf_init); median and min - max of both;
  * the same comparison for the whole call with all iterations, and the largest difference between the two results.
Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SCALES, COMBINE, WALK_STEPS = (1,), 'prob_mean', 6


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def alternated(hip, framework, warmup, repeats):
  th, tf, out_h, out_f = [], [], None, None
  for it in range(warmup + repeats):
    t0, out_h = timed(hip)
    t1, out_f = timed(framework)
    if it >= warmup:
      th.append(t0)
      tf.append(t1)
  return {'fused': spread(th), 'framework': spread(tf),
          'framework_over_fused': round(statistics.median(tf) / statistics.median(th), 3)}, out_h, out_f


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--images', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=30, help='alternated fused / framework rounds of the init stage')
  ap.add_argument('--full-repeats', type=int, default=8, help='alternated rounds of the whole CRF call')
  ap.add_argument('--crf_iter_max', type=int, default=10)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_pseudo_labels_crf needs an MI355X (no CPU fallback)')
  from spml_amd import inference
  from spml_amd.models.crf import DenseCRF
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
  h, w = a.image
  image = torch.randn(1, 3, h, w, generator=g).to(dev)
  tags = torch.zeros(ncls, dtype=torch.bool)
  tags[[0, 3, 7, 15]] = True
  tags = tags.to(dev)
  emb_model, _ = build_models(cfg, softmax_head=False)
  emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()
  crf = DenseCRF(iter_max=a.crf_iter_max, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
  image_u8 = inference.denormalized_uint8(image, cfg.network.pixel_means, cfg.network.pixel_stds)[:h, :w].contiguous()
  views = inference.flip_scale_views(image, SCALES, True, (a.crop, a.crop))
  res = {'image': [h, w], 'crop': a.crop, 'embedding_dim': c, 'num_classes': ncls, 'views': len(views),
         'walk_steps': WALK_STEPS, 'crf_iter_max': a.crf_iter_max, 'crf_path': crf.path_name(h, w, ncls)}

  run = lambda: inference.pseudo_labels_softmax_crf(emb_model, head, views, (h, w), tags, image_u8, crf,
                                                    combine=COMBINE, walk_steps=WALK_STEPS)
  for _ in range(a.warmup):
    out = run()
  torch.cuda.synchronize()
  res['head_path'] = out['head_path']
  res['image_ms'] = spread([timed(run)[0] for _ in range(a.images)])
  cam_rw = out['cam_rw'].contiguous()
  res['changed_by_crf'] = round((out['semantic_prediction'] != out['semantic_prediction_before_crf']).float().mean().item(), 4)

  tail = lambda: inference.random_walk_crf_refine(image_u8, cam_rw, crf)
  for _ in range(a.warmup):
    tail()
  res['crf_tail_ms'] = spread([timed(tail)[0] for _ in range(a.images)])
  res['crf_share_of_image'] = round(res['crf_tail_ms']['median'] / res['image_ms']['median'], 4)

  with torch.no_grad():
    ws = crf.prepare(image_u8, ncls)

    def fused(iter_max):
      return crf.infer_upsampled(ws, cam_rw, (h, w), iter_max=iter_max)[:3]

    def framework(iter_max):
      up = F.interpolate(cam_rw.unsqueeze(0), size=(h, w), mode='bilinear', align_corners=False)[0]
      before = up.argmax(0)
      q, labels = crf.infer(ws, up, iter_max=iter_max)
      return q, labels, before

    res['init_stage_ms'], _, _ = alternated(lambda: fused(0), lambda: framework(0), a.warmup, a.repeats)
    res['crf_call_ms'], got, want = alternated(lambda: fused(a.crf_iter_max), lambda: framework(a.crf_iter_max), 1,
                                               a.full_repeats)
    res['fused_vs_framework'] = {'max_abs_diff_q': (got[0] - want[0]).abs().max().item(),
                                 'label_mismatch_share': (got[1] != want[1]).float().mean().item(),
                                 'label_before_mismatch_share': (got[2] != want[2]).float().mean().item()}
  print(json.dumps(res))


if __name__ == '__main__':
  main()
