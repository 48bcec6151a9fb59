#!/usr/bin/env python3
"""Timing of the DensePose pseudo labels (pyscripts/inference/pseudo_denseposerw_crf.py,
spml_amd.inference.pseudo_labels_densepose_crf) on one synthetic 375 x 500 image padded to 513 x 513:
ResNet-101 PSPNet of the DensePose recipe, C = 32, 15 classes, a 24 x 24 k-means grid over the half-resolution map,
point labels on about 1 % of the pixels, 6 squarings, 10 CRF iterations.

Prints one JSON line:
  * ms per image (device events over whole calls of `pseudo_labels_densepose_crf`);
  * ms of the CRF tail alone (`random_walk_crf_refine` on the image's walked maps: prepare + the fused call) and its share
    of the image time;
  * the class-map stage both ways on identical device inputs (the image's own retrieval and segment ids), alternated in
    this process: `spml_segment_tag_cam_f32` (memset, count, probs, gather) + `spml_cam_finalize_f32` against
    `framework_densepose_segment_cam` + `spml_cam_finalize_f32`; median and min - max of both, the count kernel the shape
    takes, and the largest difference between the two results.
Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

WALK_STEPS = 6


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
  return {'hip': spread(th), 'framework': spread(tf),
          'framework_over_hip': round(statistics.median(tf) / statistics.median(th), 3)}, out_h, out_f


def point_labels(h, w, ncls, g):
  """A blocky class map over four classes with about 1 % of its pixels kept as points (the others 254: unlabelled), an
  ignore strip (255) along the right edge, and the cell as the instance."""
  classes = torch.tensor([0, 3, 7, ncls - 1])
  cell = (torch.arange(h) * 3 // h).view(h, 1) * 4 + (torch.arange(w) * 4 // w).view(1, w)
  dense = classes[torch.randint(0, 4, (12,), generator=g)[cell]]
  dense[: h // 3, : w // 4], dense[h - h // 3:, w - w // 4:] = classes[0], classes[3]
  semantic = torch.where(torch.rand(h, w, generator=g) < 0.01, dense, torch.full_like(dense, 254))
  semantic[:, w - 6:] = 255
  return semantic, cell.expand(h, w).contiguous()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--kmeans_num_clusters', default='24,24')
  ap.add_argument('--images', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=30, help='alternated HIP / framework rounds of the class-map stage')
  ap.add_argument('--crf_iter_max', type=int, default=10)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_densepose_pseudo needs an MI355X (no CPU fallback)')
  from spml_amd import _ffi, inference
  from spml_amd.models.crf import DenseCRF
  from spml_amd.train import build_models, densepose_point_config
  dev = torch.device('cuda', 0)
  grid = [int(v) for v in a.kmeans_num_clusters.split(',')]
  cfg = densepose_point_config(batch_size=1, use_syncbn=False)
  cfg.network.kmeans_num_clusters = grid
  c, ncls = cfg.network.embedding_dim, cfg.dataset.num_classes
  torch.manual_seed(235)
  g = torch.Generator().manual_seed(1)
  h, w = a.image
  image = torch.randn(1, 3, h, w, generator=g).to(dev)
  semantic, instance = (t.to(dev) for t in point_labels(h, w, ncls, g))
  tags = inference.label_tags_from_map(semantic, ncls)
  emb_model = build_models(cfg, recipe='densepose')[0].to(dev).to(memory_format=torch.channels_last).eval()
  crf = DenseCRF(iter_max=a.crf_iter_max, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
  padded = inference.flip_scale_views(image, [1], False, (a.crop, a.crop))[0][0]
  image_u8 = inference.denormalized_uint8(padded, cfg.network.pixel_means, cfg.network.pixel_stds)[:h, :w].contiguous()
  res = {'image': [h, w], 'crop': a.crop, 'embedding_dim': c, 'num_classes': ncls, 'kmeans_num_clusters': grid,
         'walk_steps': WALK_STEPS, 'crf_iter_max': a.crf_iter_max, 'crf_path': crf.path_name(h, w, ncls)}

  run = lambda: inference.pseudo_labels_densepose_crf(emb_model, padded, (h, w), semantic, instance, tags, image_u8, crf,
                                                      walk_steps=WALK_STEPS)
  for _ in range(a.warmup):
    out = run()
  torch.cuda.synchronize()
  res['cam_path'], res['num_segments'] = out['cam_path'], out['num_segments']
  res['image_ms'] = spread([timed(run)[0] for _ in range(a.images)])
  cam_rw = out['cam_rw'].contiguous()
  res['changed_by_crf'] = round((out['semantic_prediction'] != out['semantic_prediction_before_crf']).float().mean().item(), 4)

  tail = lambda: inference.random_walk_crf_refine(image_u8, cam_rw, crf)
  for _ in range(a.warmup):
    tail()
  res['crf_tail_ms'] = spread([timed(tail)[0] for _ in range(a.images)])
  res['crf_share_of_image'] = round(res['crf_tail_ms']['median'] / res['image_ms']['median'], 4)

  # the class-map stage on what the image's own retrieval gave: the same clustering again through densepose_segment_cam
  half_hw, out_hw = (h // 2, w // 2), (h // 8, w // 8)
  with torch.no_grad():
    embs = emb_model.generate_embeddings({'image': padded.contiguous(memory_format=torch.channels_last)},
                                         resize_as_input=True)['embedding'].float()
    embs = torch.nn.functional.interpolate(embs, size=(a.crop // 2, a.crop // 2), mode='bilinear')
    embs = embs[:, :, :half_hw[0], :half_hw[1]].contiguous()
    kept = torch.where(semantic == 255, torch.full_like(semantic, ncls), semantic)
    from spml_amd.utils.general.common import resize_labels
    clustered = emb_model.generate_clusters(embs, resize_labels(kept.unsqueeze(0), half_hw),
                                            resize_labels(instance.unsqueeze(0), half_hw))
    fed = inference.densepose_segment_cam(clustered, tags, half_hw, out_hw, ncls, cfg.network.label_divisor)
    args = (fed['nn_index'], fed['nn_value'], fed['proto_label'], -1.0, fed['cluster_index'])
    s = fed['num_segments']
    res['stage_segments'] = s
    res['count_path'] = _ffi.segment_tag_cam_path_name(half_hw[0] * half_hw[1], s, ncls)

    def hip():
      return _ffi.cam_finalize(_ffi.segment_tag_cam(*args, s, ncls, half_hw, out_hw), 1, tags, 'prob_mean', None)

    def framework():
      acc = inference.framework_densepose_segment_cam(*args, ncls, half_hw, out_hw).contiguous()
      return _ffi.cam_finalize(acc, 1, tags, 'prob_mean', None)

    res['cam_stage_ms'], got, want = alternated(hip, framework, a.warmup, a.repeats)
    res['hip_vs_framework'] = {'max_abs_diff_cam': (got - want).abs().max().item(),
                               'nan': bool(torch.isnan(got).any())}
  print(json.dumps(res))


if __name__ == '__main__':
  main()
