#!/usr/bin/env python3
"""Timing of the denseCRF tails of the kNN label inference (pyscripts/inference/inference_crf.py and
inference_crf_msc.py) on one synthetic 375 x 500 image with 21 classes: a 12 x 12 grid of segments (the
largest k-means grid here: 144 rows), 20 retrieved labels per segment, 10 CRF iterations.  The network and the retrieval
in front of the tails are those of `inference_msc.py` (tools/bench_knn_msc.py) and are not run here.

Prints one JSON line:
  * ms per image of both programs' CRF tails (device events over whole calls): `knn_votes_crf_refine` on the segments
    (prepare + the fused call) and `dense_crf_refine` on a `[21, h, w]` vote map (prepare + the existing entry);
  * the init stage both ways on identical device inputs, alternated in this process: the fused launches
    (`spml_dense_crf_infer_votes_f32` with no iteration: crf_votes_table + memset + crf_init_votes) against
    `framework_segment_votes` + `argmax` feeding the existing entry (`spml_dense_crf_infer_f32` with no iteration: memset
    + crf_init); median and min - max of both;
  * the same comparison for the whole call with all iterations, and the largest difference between the two results.
Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


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
  ap.add_argument('--grid', type=int, nargs=2, default=[12, 12])
  ap.add_argument('--classes', type=int, default=21)
  ap.add_argument('--images', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=30, help='alternated fused / framework rounds of the init stage')
  ap.add_argument('--full-repeats', type=int, default=8, help='alternated rounds of the whole CRF call')
  ap.add_argument('--crf_iter_max', type=int, default=10)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_knn_crf needs an MI355X (no CPU fallback)')
  from spml_amd import inference
  from spml_amd.models.crf import DenseCRF
  dev = torch.device('cuda', 0)
  (h, w), (gy, gx), ncls, k = a.image, a.grid, a.classes, 20
  g = torch.Generator().manual_seed(1)
  m = gy * gx
  # a blocky image (one colour per segment +- noise) and segments whose rows favour one class each
  cell = (torch.arange(h) * gy // h).view(h, 1) * gx + (torch.arange(w) * gx // w).view(1, w)
  clu = torch.randperm(m, generator=g)[cell].reshape(-1).contiguous().to(dev)
  colours = torch.randint(30, 226, (m, 3), generator=g)
  image_u8 = (colours[cell] + torch.randint(-12, 13, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8).to(dev)
  favoured = torch.randint(0, ncls, (m, 1), generator=g)
  topk = torch.where(torch.rand(m, k, generator=g) < 0.7, favoured.expand(m, k),
                     torch.randint(0, ncls, (m, k), generator=g)).contiguous().to(dev)
  crf = DenseCRF(iter_max=a.crf_iter_max, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
  res = {'image': [h, w], 'segments': m, 'retrievals': k, 'num_classes': ncls, 'crf_iter_max': a.crf_iter_max,
         'crf_path': crf.path_name(h, w, ncls)}

  votes = inference.framework_segment_votes(clu, topk, ncls, (h, w))
  tail = lambda: inference.knn_votes_crf_refine(image_u8, clu, topk, ncls, crf)
  tail_msc = lambda: inference.dense_crf_refine(image_u8, votes, crf)
  for _ in range(a.warmup):
    out = tail()
    tail_msc()
  torch.cuda.synchronize()
  res['votes_path'] = out['votes_path']
  res['inference_crf_tail_ms'] = spread([timed(tail)[0] for _ in range(a.images)])
  res['inference_crf_msc_tail_ms'] = spread([timed(tail_msc)[0] for _ in range(a.images)])
  res['changed_by_crf'] = round((out['semantic_prediction'] != out['semantic_prediction_before_crf']).float().mean().item(), 4)

  with torch.no_grad():
    ws = crf.prepare(image_u8, ncls)

    def fused(iter_max):
      return crf.infer_votes(ws, clu, topk, ncls, (h, w), iter_max=iter_max)[:3]

    def framework(iter_max):
      prob = inference.framework_segment_votes(clu, topk, ncls, (h, w))
      before = prob.argmax(0)
      q, labels = crf.infer(ws, prob, iter_max=iter_max)
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
