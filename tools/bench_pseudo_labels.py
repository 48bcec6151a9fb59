#!/usr/bin/env python3
"""Timing of the pseudo-label generation (pyscripts/inference/pseudo_softmaxrw_crf.py / pseudo_softmax.py up to the
arg-max, spml_amd.inference.pseudo_labels_softmax) on one synthetic 375 x 500 image padded to 513 x 513: ResNet-101
DeepLab-v2, C = 64, 21 classes, both recipes (`pseudo_softmaxrw`: 2 views, 6 squarings; `pseudo_softmax`: 4 views, none).

Prints one JSON line:
  * ms per image (device events over whole calls of `pseudo_labels_softmax`);
  * ms per stage of one image -- backbone, classifier head, view kernels, affinity, CAM finalisation, the walk's library
    GEMMs, up-sampling + arg-max -- from device events around the same calls issued stage by stage;
  * for every stage that is a new kernel, the same stage written as the reference's framework ops (`flip`,
    `F.interpolate`, `norm`, `softmax`, `mean`, `max`, `masked_fill`, `interpolate` + `argmax`) on identical device
    inputs, alternated with the HIP form in this process: median and min - max of both, and the largest difference
    between their results.
Needs an MI355X: there is no fallback.  `--stages-only` skips the backbone (for a kernel trace of the new kernels)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

RECIPES = {'pseudo_softmaxrw': ((1,), 'prob_mean', 6), 'pseudo_softmax': ((0.75, 1), 'logit_mean', 0)}


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def spread(v):
  return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4), 'n': len(v)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--image', type=int, nargs=2, default=[375, 500])
  ap.add_argument('--crop', type=int, default=513)
  ap.add_argument('--images', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=30, help='alternated HIP / framework rounds per stage')
  ap.add_argument('--stages-only', action='store_true')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_pseudo_labels needs an MI355X (no CPU fallback)')
  from spml_amd import _ffi, inference
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
  oh, ow = h // 8, w // 8
  n = oh * ow
  image = torch.randn(1, 3, h, w, generator=g).to(dev)
  tags = torch.zeros(ncls, dtype=torch.bool)
  tags[[0, 3, 7, 15]] = True
  tags = tags.to(dev)
  res = {'image': [h, w], 'crop': a.crop, 'embedding_dim': c, 'num_classes': ncls, 'pixels_eighth': n, 'recipes': {}}
  emb_model = None
  if not a.stages_only:
    emb_model, _ = build_models(cfg, softmax_head=False)
    emb_model = emb_model.to(dev).to(memory_format=torch.channels_last).eval()

  for name, (scales, combine, steps) in RECIPES.items():
    views = inference.flip_scale_views(image, scales, True, (a.crop, a.crop))
    nv = len(views)
    r = {'views': nv, 'combine': combine, 'walk_steps': steps}
    batch = torch.cat([v[0] for v in views], 0).contiguous(memory_format=torch.channels_last)

    def backbone():
      if emb_model is None:          # --stages-only: a smooth random map in the backbone's memory format
        base = torch.randn(nv, c, a.crop // 16 + 2, a.crop // 16 + 2, generator=g).to(dev)
        e = F.interpolate(base, size=(a.crop, a.crop), mode='bilinear', align_corners=False)
        return (e + 0.05 * torch.randn(e.shape, device=dev)).contiguous(memory_format=torch.channels_last)
      with torch.no_grad():
        return emb_model.generate_embeddings({'image': batch}, resize_as_input=True)['embedding'].float()

    head.prepare_inference()
    canvases = torch.zeros((nv, 1, ncls, a.crop, a.crop), device=dev)

    def run_head(embs):
      canvases.zero_()
      for i in range(nv):
        assert head.accumulate_logits(embs[i:i + 1], canvases[i], 0, 0) == sc.HIP_HEAD_PATH

    units = torch.empty((nv, c, n), device=dev)
    acc = torch.zeros((ncls, n), device=dev)

    def view_kernels_hip(embs):
      acc.zero_()
      for i, (_, crop_hw, flip) in enumerate(views):
        _ffi.resample_unit(embs[i], crop_hw, flip, (oh, ow), units, i)
        _ffi.resample_classes_accumulate(canvases[i, 0], crop_hw, flip, (oh, ow), acc, combine)
      return units, acc

    def view_kernels_framework(embs):                     # pseudo_softmaxrw_crf.py:130-144, the ops as they stand
      out_u, out_p = [], []
      for i, (_, (rh, rw), flip) in enumerate(views):
        e = embs[i:i + 1][:, :, :rh, :rw]
        l = canvases[i][..., :rh, :rw]
        if flip:
          e, l = torch.flip(e, dims=[3]), torch.flip(l, dims=[3])
        e = F.interpolate(e, size=(oh, ow), mode='bilinear')
        out_u.append(e / torch.norm(e, dim=1))
        l = F.interpolate(l, size=(oh, ow), mode='bilinear')
        out_p.append(F.softmax(l, dim=1) if combine == 'prob_mean' else l)
      return out_u, out_p

    def finalize_framework(terms):                        # :146-157
      probs = torch.mean(torch.cat(terms, dim=0), dim=0)
      if combine == 'logit_mean':
        probs = F.softmax(probs, dim=0)
      max_prob = torch.max(probs.view(ncls, -1), dim=1)[0]
      cam = probs / max_prob.view(ncls, 1, 1)
      return cam.masked_fill((~tags).view(-1, 1, 1).expand(-1, oh, ow), 0)

    def labels_framework(cam_rw):                         # :173-176 on the device
      return F.interpolate(cam_rw.unsqueeze(0), size=(h, w), mode='bilinear', align_corners=False).argmax(1)[0]

    # ---- stage by stage (the calls of pseudo_labels_softmax, events between the stages) ----
    stage = {k: [] for k in ('backbone', 'head', 'view_kernels', 'affinity', 'cam_finalize', 'walk_gemms',
                             'upsample_argmax')}
    with torch.no_grad():
      for it in range(a.warmup + a.repeats):
        t_b, embs = timed(backbone)
        t_h, _ = timed(lambda: run_head(embs))
        t_v, _ = timed(lambda: view_kernels_hip(embs))
        t_a, trans = timed(lambda: _ffi.affinity_transition(units, 5.0, 20))
        t_f, cam = timed(lambda: _ffi.cam_finalize(acc, nv, tags, combine).view(ncls, oh, ow))
        t_w, cam_rw = timed(lambda: inference._walk(trans, cam, steps))
        t_u, pred = timed(lambda: _ffi.upsample_argmax(cam_rw, h, w))
        if it >= a.warmup:
          for k, t in zip(stage, (t_b, t_h, t_v, t_a, t_f, t_w, t_u)):
            stage[k].append(t)
      r['stage_ms'] = {k: spread(v) for k, v in stage.items()}
      if emb_model is None:
        r['stage_ms'].pop('backbone')

      # ---- like for like: HIP form against the framework ops on identical inputs, alternated ----
      ab = {k: ([], []) for k in ('view_kernels', 'cam_finalize', 'upsample_argmax')}
      for it in range(a.warmup + a.repeats):
        t0, _ = timed(lambda: view_kernels_hip(embs))
        t1, (fu, fp) = timed(lambda: view_kernels_framework(embs))
        t2, cam_h = timed(lambda: _ffi.cam_finalize(acc, nv, tags, combine).view(ncls, oh, ow))
        t3, cam_f = timed(lambda: finalize_framework(fp))
        t4, pred_h = timed(lambda: _ffi.upsample_argmax(cam_rw, h, w))
        t5, pred_f = timed(lambda: labels_framework(cam_rw))
        if it >= a.warmup:
          for k, th, tf in (('view_kernels', t0, t1), ('cam_finalize', t2, t3), ('upsample_argmax', t4, t5)):
            ab[k][0].append(th)
            ab[k][1].append(tf)
      r['hip_vs_framework_ms'] = {
          k: {'hip': spread(vh), 'framework': spread(vf),
              'framework_over_hip': round(statistics.median(vf) / statistics.median(vh), 3)}
          for k, (vh, vf) in ab.items()}
      r['max_abs_diff'] = {
          'unit_embedding': max((units[i].view(c, oh, ow) - fu[i][0]).abs().max().item() for i in range(nv)),
          'cam': (cam_h - cam_f).abs().max().item(),
          'label_mismatch_share': (pred_h != pred_f).float().mean().item()}

    # ---- whole images ----
    if emb_model is not None:
      run = lambda: inference.pseudo_labels_softmax(emb_model, head, views, (h, w), tags, combine=combine,
                                                    walk_steps=steps)
      for _ in range(a.warmup):
        out = run()
      torch.cuda.synchronize()
      r['head_path'] = out['head_path']
      r['image_ms'] = spread([timed(run)[0] for _ in range(a.images)])
      r['walk_gemm_share_of_image'] = round(r['stage_ms']['walk_gemms']['median'] / r['image_ms']['median'], 4)
    res['recipes'][name] = r
  print(json.dumps(res))


if __name__ == '__main__':
  main()
