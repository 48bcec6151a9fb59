#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the REAL reference.

Runs only in the build container, where the reference tree is mounted
read-only at /root/reference.  It imports the reference's own leaf functions
(nothing is copied), feeds them seeded synthetic inputs on CPU / fp32 and stores
inputs + outputs as small .npz files.  The oracle (oracle/spml_oracle.py) and,
on the GPU box, the HIP path are then checked against these files.

Two in-memory shims are needed to run the reference on CPU:
  * spml/utils/segsort/common.py:376 reads ``tensor.device.index`` which is
    None on CPU -> the function source is exec'd with ``(… .index or 0)``;
  * torch.nn.parallel.scatter_gather.gather asserts on CPU tensors ->
    replaced by torch.cat while B1 goldens are generated.

Usage:  python tools/gen_golden.py  [--ref /root/reference] [--out tests/golden]
"""

import argparse
import inspect
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True


def _np(x):
  if isinstance(x, torch.Tensor):
    return x.detach().cpu().numpy()
  return np.asarray(x)


ONLY = None      # --only a,b: write just these fixtures (the others stay as committed)


def save(out_dir, name, **arrays):
  if ONLY is not None and name not in ONLY:
    return
  path = os.path.join(out_dir, name + '.npz')
  np.savez_compressed(path, **{k: _np(v) for k, v in arrays.items()})
  print('wrote %-40s %7.1f KB' % (path, os.path.getsize(path) / 1024.0))


def coherent_embedding(gen, n, c, h, w, blobs=5, noise=0.35, strengths=None):
  """Spatially coherent embedding map: a few random directions blended by
  smooth spatial weights plus noise (so k-means has structure to find).
  `strengths`: one factor per blob direction (the same random draws without it)."""
  dirs = torch.randn(blobs, c, generator=gen)
  if strengths is not None:
    dirs = dirs * torch.tensor(strengths, dtype=dirs.dtype).view(blobs, 1)
  cy = torch.rand(n, blobs, generator=gen)
  cx = torch.rand(n, blobs, generator=gen)
  yy = torch.linspace(0, 1, h).view(1, 1, h, 1)
  xx = torch.linspace(0, 1, w).view(1, 1, 1, w)
  wgt = torch.exp(-((yy - cy.view(n, blobs, 1, 1)) ** 2 +
                    (xx - cx.view(n, blobs, 1, 1)) ** 2) / 0.05)
  emb = torch.einsum('nbhw,bc->nchw', wgt, dirs)
  emb = emb + noise * torch.randn(n, c, h, w, generator=gen)
  return emb.float()


def blocky_labels(gen, n, h, w, cells, low, high):
  grid = torch.randint(low, high, (n, cells, cells), generator=gen)
  iy = (torch.arange(h) * cells // h).clamp(max=cells - 1)
  ix = (torch.arange(w) * cells // w).clamp(max=cells - 1)
  return grid[:, iy][:, :, ix].long()


def gen_n7(ref, out):
  """N7: pseudo-label generation.  pyscripts/inference/pseudo_softmaxrw_crf.py:130-144 per view and :146-170 once
  (`prob_mean`, WALK_STEPS read from its line 29) and pseudo_softmax.py:129-144 / :146-173 (`logit_mean`, once with the
  file's WALK_STEPS = 0 and once with 6), exec'd from the reference's own lines on seeded CPU inputs.  The stub network
  is its stride-8 maps (stored as fp16-exact values): both this generator and the tests form the network outputs as
  `F.interpolate(coarse, size=(Hp, Wp), mode='bilinear', align_corners=False)`, what `resize_as_input=True` does in
  the real model.  The scripts' last step (`cv2.resize(..., INTER_LINEAR)` + `np.argmax`) cannot run without cv2: the
  yardstick of the labels is CPU `F.interpolate(cam_rw, size=(h, w), mode='bilinear', align_corners=False)` (the same
  half-pixel mapping); its top-1 minus top-2 margin is stored."""
  import linecache
  import textwrap
  F = torch.nn.functional

  def ref_lines(path, first, last):
    txt = ''.join(linecache.getline(path, i) for i in range(first, last + 1))
    assert txt.strip(), path
    return textwrap.dedent(txt).replace('.cuda()', '')

  def walk_steps_of(path):
    for i in range(20, 40):
      ln = linecache.getline(path, i).strip()
      if ln.startswith('WALK_STEPS'):
        return int(ln.split('=')[1])
    raise AssertionError('no WALK_STEPS in ' + path)

  rw_py = os.path.join(ref, 'pyscripts', 'inference', 'pseudo_softmaxrw_crf.py')
  sm_py = os.path.join(ref, 'pyscripts', 'inference', 'pseudo_softmax.py')
  scripts = {
      'rw': (rw_py, ref_lines(rw_py, 130, 144), ref_lines(rw_py, 146, 170), walk_steps_of(rw_py)),
      'sm0': (sm_py, ref_lines(sm_py, 129, 144), ref_lines(sm_py, 146, 173), walk_steps_of(sm_py)),
      'sm6': (sm_py, ref_lines(sm_py, 129, 144), ref_lines(sm_py, 146, 173), 6)}
  assert scripts['rw'][3] == 6 and scripts['sm0'][3] == 0
  assert 'F.softmax(semantic_logit, dim=1)' in scripts['rw'][1] and 'cam_rw = cam_rw.view' in scripts['rw'][2]
  assert 'semantic_probs.append(semantic_logit)' in scripts['sm0'][1] and 'F.softmax(semantic_probs, dim=0)' in scripts['sm0'][2]

  def coarse_view(field, view_hw, pad_hw, flip, noise, gen):
    """Stride-8 map of one view: the image-space field at the view's size, flipped with the image, padded (edge
    values) to the padded size, sampled at stride 8, noise added at that resolution; fp16-exact."""
    f = F.interpolate(field, size=view_hw, mode='bilinear', align_corners=False)
    if flip:
      f = torch.flip(f, dims=[3])
    f = F.pad(f, (0, pad_hw[1] - view_hw[1], 0, pad_hw[0] - view_hw[0]), mode='replicate')
    c = F.interpolate(f, size=(pad_hw[0] // 8 + 1, pad_hw[1] // 8 + 1), mode='bilinear', align_corners=False)
    c = c + noise * c.abs().mean() * torch.randn(c.shape, generator=gen)
    return c[0].half()

  store = {}
  # (seed, C, image, tags, views = (scale-resized size, padded size) per scale; per scale the flipped view first).
  # Seeds: 1700 meets every condition asserted below at once; for the second case 1701, 1721 and 1751 exceed the
  # low-margin cap in the `sm0` recipe (5.0 %, 3.1 %, 1.9 % of the pixels), 1711, 1731 and 1741 meet everything, and
  # 1731 has the fewest low margins of those.
  cases = [(1700, 16, (88, 120), (0, 3, 7, 15), [((88, 120), (96, 128))]),
           (1731, 32, (93, 77), (0, 5, 12), [((70, 58), (72, 64)), ((93, 77), (96, 80))])]
  for ci, (seed, c, image_hw, tags, scales) in enumerate(cases):
    gen = torch.Generator().manual_seed(seed)
    image_h, image_w = image_hw
    emb_field = torch.randn(1, c, image_h // 48 + 2, image_w // 48 + 2, generator=gen)
    cls_field = 4.0 * torch.randn(1, 21, image_h // 32 + 2, image_w // 32 + 2, generator=gen)
    label_tags = torch.zeros(21, dtype=torch.bool)
    label_tags[list(tags)] = True
    views = []
    for view_hw, pad_hw in scales:
      for flip in (True, False):
        views.append((coarse_view(emb_field, view_hw, pad_hw, flip, 0.03, gen),
                      coarse_view(cls_field, view_hw, pad_hw, flip, 0.03, gen), view_hw, pad_hw, flip))
    t = 'c%d_' % ci
    store[t + 'image_hw'] = np.array(image_hw)
    store[t + 'tags'] = label_tags.numpy()
    store[t + 'views'] = np.array([[p[0], p[1], v[0], v[1], int(fl)] for _, _, v, p, fl in views])
    for vi, (ce, cl, _, _, _) in enumerate(views):
      store[t + 'emb%d' % vi] = ce.numpy()
      store[t + 'logit%d' % vi] = cl.numpy()
    trans0 = None
    for tag, (path, src_view, src_once, steps) in scripts.items():
      env = {'torch': torch, 'F': F, 'affs': [], 'semantic_probs': [], 'image_h': image_h, 'image_w': image_w,
             'label_tags': label_tags.clone(), 'WALK_STEPS': steps, 'TH': None}
      units = []
      for ce, cl, view_hw, pad_hw, flip in views:
        env['embeddings'] = {'embedding': F.interpolate(ce.float().unsqueeze(0), size=pad_hw, mode='bilinear',
                                                        align_corners=False)}
        env['outputs'] = {'semantic_logit': F.interpolate(cl.float().unsqueeze(0), size=pad_hw, mode='bilinear',
                                                          align_corners=False)}
        env['resize_image_h'], env['resize_image_w'] = view_hw
        env['data_info'] = {'is_flip': flip}
        exec(compile(src_view, path + ':view', 'exec'), env)
        units.append(env['embs'].clone())
      exec(compile(src_once, path + ':once', 'exec'), env)
      trans = env['aff_mat'] / torch.sum(env['aff_mat'], dim=0, keepdim=True)
      cam, cam_rw = env['cam_full_arr'], env['cam_rw']
      oh, ow = image_h // 8, image_w // 8
      assert tuple(cam.shape) == (21, oh, ow) == tuple(cam_rw.shape) and tuple(trans.shape) == (oh * ow, oh * ow)
      if trans0 is None:                                    # the embedding side is the same in both scripts
        trans0 = trans
        store[t + 'trans'] = trans
        for vi, u in enumerate(units):
          store[t + 'unit%d' % vi] = u
      assert torch.equal(trans, trans0)
      up = lambda m: F.interpolate(m.unsqueeze(0), size=image_hw, mode='bilinear', align_corners=False)[0]
      top2 = up(cam_rw).topk(2, dim=0).values
      margin = top2[0] - top2[1]
      # the conditions that keep the tests from passing vacuously
      diag = trans.diagonal().mean().item()
      moved = (up(cam).argmax(0) != up(cam_rw).argmax(0)).float().mean().item()
      low = (margin < 2e-4 * cam_rw.abs().max()).float().mean().item()
      winners = up(cam_rw).argmax(0).unique().numel()
      print('n7 case %d %-3s: mean diag %.3f, arg-max moved by the walk on %.1f %%, low margin %.2f %%, %d classes win'
            % (ci, tag, diag, 100 * moved, 100 * low, winners))
      assert diag < 0.8, 'incoherent embeddings: the transition matrix is the identity -- pick another seed'
      # (one application of T without a squaring moves few labels: the 3 % floor is asked of the walked recipes)
      assert steps == 0 or moved >= 0.03, 'the walk changes too few labels -- pick another seed'
      assert low <= 0.01 and winners >= 3
      store.update({t + tag + '_cam': cam, t + tag + '_cam_rw': cam_rw, t + tag + '_margin': margin})
  store['recipes'] = np.array(['rw:prob_mean:6', 'sm0:logit_mean:0', 'sm6:logit_mean:6'])
  save(out, 'n7_pseudo_labels', **store)


def gen_n8(ref, out):
  """N8: multi-scale + flip softmax inference.  pyscripts/inference/inference_softmax_msc.py:107-143 exec'd per view and
  :146-149 once, from the reference's own lines on seeded CPU inputs (`.cuda()` / `.to("cuda:0")` stripped).
  `transforms.resize_with_pad` (:99-102) needs cv2 to import: the views are zero-padded here, before the exec'd lines.
  The stub network is the N6 arrangement: a seeded 5x5 convolution as the embedding model and the reference's own
  SoftmaxClassifier with seeded non-trivial running statistics; the last 1x1's weight is multiplied by 6 so that the maps
  are confident (with the default initialisation every probability is near 1 / ncls and the labels say nothing).
  Stored: per scale the un-flipped scaled image (flip and zero-padding are exact: the tests rebuild the views), the conv
  and head state, the view list, the summed probabilities and `semantic_pred` of the reference, its top-1 minus top-2
  margin and `max_abs_logit`, the largest |crop logit| the wrapped prediction model saw."""
  import linecache
  import math
  import textwrap
  import spml.models.predictions.softmax_classifier as p_cls
  F = torch.nn.functional

  def ref_lines(path, first, last):
    txt = ''.join(linecache.getline(path, i) for i in range(first, last + 1))
    assert txt.strip(), path
    return textwrap.dedent(txt).replace('.cuda()', '').replace('.to("cuda:0")', '')

  msc_py = os.path.join(ref, 'pyscripts', 'inference', 'inference_softmax_msc.py')
  src_view, src_once = ref_lines(msc_py, 107, 143), ref_lines(msc_py, 146, 149)
  assert 'semantic_logit /= counts' in src_view and 'F.softmax(semantic_logit, dim=1)' in src_view
  assert 'semantic_logit[..., ::-1]' in src_view and 'cuda' not in src_view
  assert 'np.sum(semantic_logits, axis=0)' in src_once and 'np.argmax(semantic_logits, axis=0)' in src_once

  class StubEmbedder:
    def __init__(self, conv):
      self.conv = conv

    def __call__(self, datas, targets=None, resize_as_input=False):
      assert resize_as_input
      return {'embedding': self.conv(datas['image'])}

  class RecordingHead:
    def __init__(self, head):
      self.head, self.max_abs_logit = head, 0.0

    def __call__(self, datas):
      outputs = self.head(datas)
      self.max_abs_logit = max(self.max_abs_logit, outputs['semantic_logit'].abs().max().item())
      return outputs

  store = {}
  # (seed, C, classes, image, crop, stride, scales).  Seeds are changed until the two assertions at the end hold.
  cases = [(1800, 16, 5, (44, 60), (32, 32), (20, 20), (0.5, 1, 1.5)),
           (1810, 32, 21, (41, 50), (50, 50), (33, 33), (0.75, 1, 1.25))]
  for ci, (seed, c, ncls, image_hw, crop, stride, scales) in enumerate(cases):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    image_h, image_w = image_hw
    conv = torch.nn.Conv2d(3, c, 5, padding=2)
    base = torch.randn(1, 3, image_h // 8 + 2, image_w // 8 + 2, generator=gen)
    image = F.interpolate(base, size=image_hw, mode='bilinear', align_corners=False)
    image = image + 0.05 * torch.randn(1, 3, image_h, image_w, generator=gen)
    cfg = AttrDict(dataset=AttrDict(semantic_ignore_index=255, num_classes=ncls),
                   network=AttrDict(embedding_dim=c),
                   test=AttrDict(stride=list(stride), crop_size=list(crop)))
    head = p_cls.SoftmaxClassifier(cfg)
    with torch.no_grad():
      bn = head.semantic_classifier[1]
      bn.weight.copy_(0.5 + torch.rand(2 * c, generator=gen))
      bn.bias.copy_(0.1 * torch.randn(2 * c, generator=gen))
      bn.running_mean.copy_(0.05 * torch.randn(2 * c, generator=gen))
      bn.running_var.copy_(0.02 + 0.05 * torch.rand(2 * c, generator=gen))
      head.semantic_classifier[4].weight.mul_(6.0)
      head.semantic_classifier[4].bias.copy_(0.1 * torch.randn(ncls, generator=gen))
    head.eval()
    recorder = RecordingHead(head)
    t = 'c%d_' % ci
    views, semantic_logits = [], []
    for si, scale in enumerate(scales):
      size = (max(int(round(image_h * scale)), 1), max(int(round(image_w * scale)), 1))
      scaled = image if scale == 1 else F.interpolate(image, size=size, mode='bilinear', align_corners=False)
      store[t + 'scaled%d' % si] = scaled
      rh, rw = scaled.shape[-2:]
      pad_h, pad_w = max(rh, crop[0]), max(rw, crop[1])
      for flip in (True, False):                              # create_image_pyramid: the flipped view first
        view = torch.zeros(1, 3, pad_h, pad_w)
        view[:, :, :rh, :rw] = torch.flip(scaled, dims=[3]) if flip else scaled
        views.append([si, pad_h, pad_w, rh, rw, int(flip)])
        env = {'config': cfg, 'math': math, 'np': np, 'torch': torch, 'F': F, 'image_batch': {'image': view},
               'pad_image_h': pad_h, 'pad_image_w': pad_w, 'resize_image_h': rh, 'resize_image_w': rw,
               'image_h': image_h, 'image_w': image_w, 'data_info': {'is_flip': flip},
               'embedding_model': StubEmbedder(conv), 'prediction_model': recorder,
               'semantic_logits': semantic_logits}
        with torch.no_grad():
          exec(compile(src_view, msc_py + ':107-143', 'exec'), env)
        assert semantic_logits[-1].shape == (1, ncls, image_h, image_w) and semantic_logits[-1].dtype == np.float32
        assert tuple(env['counts'].shape) == (1, 1, pad_h, pad_w)
    env = {'np': np, 'semantic_logits': semantic_logits}
    exec(compile(src_once, msc_py + ':146-149', 'exec'), env)
    prob, pred = env['semantic_logits'], env['semantic_pred']
    assert prob.shape == (ncls, image_h, image_w) and prob.dtype == np.float32
    assert pred.shape == image_hw and pred.dtype == np.uint8
    top2 = torch.from_numpy(prob).topk(2, dim=0).values
    margin = top2[0] - top2[1]
    # B: the project's logit bound is 1e-4 * max|logit| per view, a softmax moves a probability by at most half of the
    # logit error, the errors of the views add up; a label can flip only where the margin is below 2 B
    bound = 0.5 * len(views) * 1e-4 * recorder.max_abs_logit
    low = (margin < 2 * bound).float().mean().item()
    winners = np.unique(pred).size
    print('n8 case %d: %d views, max|logit| %.3f, B %.3e, low margin %.2f %%, %d classes win, max prob sum %.3f'
          % (ci, len(views), recorder.max_abs_logit, bound, 100 * low, winners, prob.max()))
    assert low < 0.01, 'case %d: %.4f of the pixels have a low margin -- pick another seed' % (ci, low)
    assert winners >= 3, 'case %d: only %d classes win -- pick another seed' % (ci, winners)
    store.update({
        t + 'conv_w': conv.weight, t + 'conv_b': conv.bias,
        t + 'cfg': np.array([c, ncls, image_h, image_w, crop[0], crop[1], stride[0], stride[1]]),
        t + 'views': np.array(views), t + 'semantic_prob': prob, t + 'semantic_pred': pred, t + 'margin': margin,
        t + 'max_abs_logit': np.array(recorder.max_abs_logit, dtype=np.float64),
        t + 'state_names': np.array(list(head.state_dict().keys()))})
    store.update({t + 'sd_' + k: v for k, v in head.state_dict().items()})
  save(out, 'n8_softmax_msc', **store)
  size = os.path.getsize(os.path.join(out, 'n8_softmax_msc.npz'))
  assert size < 600 * 1024, 'n8_softmax_msc.npz is %d bytes' % size


def cpu_shimmed_segment_by_kmeans(s_common):
  """The CPU shim of main(): spml/utils/segsort/common.py:376 reads `tensor.device.index`, None on the CPU."""
  src = inspect.getsource(s_common.segment_by_kmeans)
  assert 'cur_cluster_indices.device.index' in src
  ns = dict(s_common.__dict__)
  exec(compile(src.replace('cur_cluster_indices.device.index', '(cur_cluster_indices.device.index or 0)'),
               '<segment_by_kmeans+cpu-shim>', 'exec'), ns)
  return ns['segment_by_kmeans']


def stub_embedder_class(e_dl):
  """A seeded convolution as `generate_embeddings` with the reference's own `generate_clusters` (N9, N10)."""
  class StubEmbedder:
    label_divisor = 2048
    semantic_ignore_index = 255
    kmeans_iterations = 10

    def __init__(self, conv, clusters):
      self.conv, self.kmeans_num_clusters = conv, clusters

    def generate_embeddings(self, datas, targets=None, resize_as_input=False):
      assert resize_as_input
      return {'embedding': self.conv(datas['image']), 'local_feature': None}

    generate_clusters = e_dl.ResnetDeeplab.generate_clusters
  return StubEmbedder


def gen_n9(ref, out):
  """N9: multi-scale + flip kNN inference.  pyscripts/inference/inference_msc.py:157-226 exec'd per view (window ends,
  per-crop normalise + overlap average, crop to the un-padded view, k-means, Segsort.predictions against a memory bank,
  one-hot + mean over the 20 retrievals) and :237-242 once, from the reference's own lines on seeded CPU inputs.  The
  arrangement of N5 and N8: a seeded 5x5 convolution as `generate_embeddings`, the reference's own `generate_clusters`
  (on the CPU-shimmed segment_by_kmeans) and `Segsort`, a bank of perturbed image embeddings with random labels.
  cv2 is not installed: as in `gen_n7` the yardstick of :230-231 (`cv2.resize(..., INTER_LINEAR)`) is CPU
  `F.interpolate(..., mode='bilinear', align_corners=False)`, the same half-pixel mapping; the flip of :232-233 is
  applied to its result.  Stored per view: `cluster_index` (int16, dense), the labels retrieved per SEGMENT (uint8
  `[m, 20]`, recovered from `semantic_score`: all pixels of a segment are asserted to agree) and the view's vote map;
  once: `semantic_prob`, `semantic_pred` and the top-1 minus top-2 `margin`.  Labels are compared where the margin is at
  least 2e-4 * max|semantic_prob| (the N7 rule); at most 1 % of the pixels may fall below (asserted here)."""
  import linecache
  import math
  import textwrap
  import spml.models.embeddings.resnet_deeplab as e_dl
  import spml.models.predictions.segsort as p_segsort
  import spml.utils.general.common as g_common
  import spml.utils.segsort.common as s_common
  F = torch.nn.functional

  def ref_lines(path, first, last):
    txt = ''.join(linecache.getline(path, i) for i in range(first, last + 1))
    assert txt.strip(), path
    return textwrap.dedent(txt).replace('.cuda()', '').replace('.to("cuda:0")', '')

  msc_py = os.path.join(ref, 'pyscripts', 'inference', 'inference_msc.py')
  src_view, src_once = ref_lines(msc_py, 157, 226), ref_lines(msc_py, 237, 242)
  assert 'patch_ind_h' in src_view and '[..., :resize_image_h, :resize_image_w]' in src_view and 'cuda' not in src_view
  assert 'with_prediction=True' in src_view and 'torch.mean(semantic_topk, dim=1)' in src_view
  assert src_view.rstrip().endswith('semantic_topk.view(resize_image_h, resize_image_w, -1)')
  assert 'np.mean(semantic_topks, axis=0)' in src_once and 'np.argmax(semantic_prob, axis=0)' in src_once
  resize_src = ref_lines(msc_py, 230, 233)
  assert 'cv2.INTER_LINEAR' in resize_src and 'semantic_topk[:, ::-1]' in resize_src

  ns = {'segment_by_kmeans': cpu_shimmed_segment_by_kmeans(s_common)}
  StubEmbedder = stub_embedder_class(e_dl)

  store = {}
  # (seed, C, classes, image, crop, stride, scales, k-means grid, bank size).  (a) one scale, a flip pair, no padding;
  # (b) two scales, odd image width: 0.75 up-samples to the image from a padded view (45 x 58 in 48 x 58, two windows
  # along x), 1.25 down-samples to it (75 x 96: 2 x 3 windows).  The banks hold 400 / 500 entries so that the 20
  # retrievals of a segment are its neighbourhood (with 80 entries they were a quarter of the bank and every vote map
  # diffuse).  Seeds: 1900 meets the cap for (a) (0.45 % of the pixels under the margin); for (b) 1910 sits on the cap
  # (1.00 %) and is rejected, 1911 has 0.09 % (1912-1914: 0.15 %, 0.39 %, 0.17 %; 1915: 2.25 %).
  cases = [(1900, 16, 5, (44, 60), (44, 60), (30, 30), (1,), (4, 4), 400),
           (1911, 32, 7, (60, 77), (48, 48), (32, 32), (0.75, 1.25), (5, 4), 500)]
  orig = e_dl.segsort_common.segment_by_kmeans
  e_dl.segsort_common.segment_by_kmeans = ns['segment_by_kmeans']
  try:
    for ci, (seed, c, ncls, image_hw, crop, stride, scales, grid, n_bank) in enumerate(cases):
      gen = torch.Generator().manual_seed(seed)
      torch.manual_seed(seed)
      image_h, image_w = image_hw
      conv = torch.nn.Conv2d(3, c, 5, padding=2)
      base = torch.randn(1, 3, image_h // 8 + 2, image_w // 8 + 2, generator=gen)
      image = F.interpolate(base, size=image_hw, mode='bilinear', align_corners=False)
      image = image + 0.05 * torch.randn(1, 3, image_h, image_w, generator=gen)
      cfg = AttrDict(
          train=AttrDict(sem_ann_loss_types='none', sem_occ_loss_types='none', img_sim_loss_types='none',
                         feat_aff_loss_types='none', sem_ann_concentration=0.0, sem_occ_concentration=0.0,
                         img_sim_concentration=0.0, feat_aff_concentration=0.0, sem_ann_loss_weight=0.0,
                         sem_occ_loss_weight=0.0, img_sim_loss_weight=0.0, feat_aff_loss_weight=0.0),
          dataset=AttrDict(semantic_ignore_index=255, num_classes=ncls),
          network=AttrDict(label_divisor=2048),
          test=AttrDict(stride=list(stride), crop_size=list(crop)))
      predictor = p_segsort.Segsort(cfg)
      # a memory bank that looks like the image's own segments (N5): normalised embeddings of random pixels, perturbed
      with torch.no_grad():
        full = g_common.normalize_embedding(conv(image).permute(0, 2, 3, 1).reshape(-1, c))
      pick = torch.randint(0, full.shape[0], (n_bank,), generator=gen)
      bank = g_common.normalize_embedding(full[pick] + 0.1 * torch.randn(n_bank, c, generator=gen))
      # random labels, drawn per cell of a coarse grid over the image; an entry takes the label of its source pixel's
      # cell.  (Votes are multiples of 1/20: with labels drawn per ENTRY the top two classes of a segment tie so often
      # that 14 % of the pixels of case (a) had a zero margin -- whole segments, not a matter of seeds.)
      bank_lab = blocky_labels(gen, 1, image_h, image_w, 4, 0, ncls)[0].reshape(-1)[pick]
      t = 'c%d_' % ci
      views, semantic_topks = [], []
      for si, scale in enumerate(scales):
        size = (max(int(round(image_h * scale)), 1), max(int(round(image_w * scale)), 1))
        scaled = image if scale == 1 else F.interpolate(image, size=size, mode='bilinear', align_corners=False)
        store[t + 'scaled%d' % si] = scaled
        rh, rw = scaled.shape[-2:]
        pad_h, pad_w = max(rh, crop[0]), max(rw, crop[1])
        for flip in (True, False):                            # create_image_pyramid: the flipped view first
          view = torch.zeros(1, 3, pad_h, pad_w)
          view[:, :, :rh, :rw] = torch.flip(scaled, dims=[3]) if flip else scaled
          fake = torch.full((1, pad_h, pad_w), 255, dtype=torch.long)
          fake[:, :rh, :rw] = 0                               # :140-151
          env = {'config': cfg, 'math': math, 'np': np, 'torch': torch, 'image_batch': {'image': view},
                 'pad_image_h': pad_h, 'pad_image_w': pad_w, 'resize_image_h': rh, 'resize_image_w': rw,
                 'embedding_model': StubEmbedder(conv, list(grid)), 'prediction_model': predictor,
                 'common_utils': g_common, 'fake_label_batch': {'semantic_label': fake, 'instance_label': fake.clone()},
                 'semantic_memory_prototypes': bank, 'semantic_memory_prototype_labels': bank_lab}
          with torch.no_grad():
            exec(compile(src_view, msc_py + ':157-226', 'exec'), env)
          votes = env['semantic_topk']
          assert tuple(votes.shape) == (rh, rw, ncls) and votes.dtype == torch.float32
          # :228-233 with F.interpolate in the place of cv2.resize
          resized = F.interpolate(votes.permute(2, 0, 1).unsqueeze(0), size=image_hw, mode='bilinear',
                                  align_corners=False)[0].permute(1, 2, 0).numpy().astype(np.float32)
          if flip:
            resized = resized[:, ::-1]
          semantic_topks.append(resized)
          # dense segment ids and the labels retrieved per segment, from the per-pixel outputs
          score = env['outputs']['semantic_score']
          _, clu = torch.unique(env['embeddings']['cluster_index'], return_inverse=True)
          m = int(clu.max()) + 1
          assert tuple(score.shape) == (rh * rw, 20) and clu.shape[0] == rh * rw
          first = torch.full((m,), rh * rw, dtype=torch.long).scatter_reduce(0, clu, torch.arange(rh * rw), 'amin')
          topk = score[first]
          assert torch.equal(topk[clu], score), 'the pixels of a segment disagree on their retrieved labels'
          assert m <= 32767 and int(topk.max()) < ncls
          vi = len(views)
          views.append([si, pad_h, pad_w, rh, rw, int(flip), m])
          store[t + 'cluster_index%d' % vi] = clu.to(torch.int16)
          store[t + 'topk%d' % vi] = topk.to(torch.uint8)
          store[t + 'votes%d' % vi] = np.ascontiguousarray(resized.transpose(2, 0, 1))
      env = {'np': np, 'semantic_topks': semantic_topks}
      exec(compile(src_once, msc_py + ':237-242', 'exec'), env)
      prob, pred = env['semantic_prob'], env['semantic_pred']
      assert prob.shape == (ncls, image_h, image_w) and prob.dtype == np.float32
      assert pred.shape == image_hw and pred.dtype == np.uint8
      top2 = torch.from_numpy(np.ascontiguousarray(prob)).topk(2, dim=0).values
      margin = top2[0] - top2[1]
      low = (margin < 2e-4 * float(np.abs(prob).max())).float().mean().item()
      winners = np.unique(pred).size
      print('n9 case %d (seed %d): %d views, segments %s, low margin %.2f %%, %d classes win, max prob %.3f'
            % (ci, seed, len(views), [v[6] for v in views], 100 * low, winners, prob.max()))
      assert low <= 0.01, 'case %d: %.4f of the pixels have a low margin -- pick another seed' % (ci, low)
      assert winners >= 3, 'case %d: only %d classes win -- pick another seed' % (ci, winners)
      store.update({
          t + 'conv_w': conv.weight, t + 'conv_b': conv.bias, t + 'bank': bank, t + 'bank_lab': bank_lab,
          t + 'cfg': np.array([c, ncls, image_h, image_w, crop[0], crop[1], stride[0], stride[1], grid[0], grid[1]]),
          t + 'views': np.array(views), t + 'semantic_prob': np.ascontiguousarray(prob), t + 'semantic_pred': pred,
          t + 'margin': margin})
  finally:
    e_dl.segsort_common.segment_by_kmeans = orig
  save(out, 'n9_knn_msc', **store)
  size = os.path.getsize(os.path.join(out, 'n9_knn_msc.npz'))
  assert size < 600 * 1024, 'n9_knn_msc.npz is %d bytes' % size


def gen_n10(ref, out):
  """N10: multi-scale memory-bank generation.  pyscripts/inference/prototype_msc.py:126-197 exec'd per view (window
  ends, per-crop normalise + overlap average, k-means that ignores the padding, `calculate_prototypes_from_labels`,
  `find_majority_label_index`, the append to `prototype_results`) and :204-206 once (the concatenation), from the
  reference's own lines on seeded CPU inputs, with the arrangement of N9: a seeded 5x5 convolution as
  `generate_embeddings` and the reference's own `generate_clusters` on the CPU-shimmed segment_by_kmeans.  The views are
  those of `create_image_pyramid(scales=[0.5, 1, 1.5], is_flip=False)` (:92-95) restated with torch (cv2 is not
  installed): images bilinear, labels `nearest` -- what `spml_amd.inference.flip_scale_views` / `label_views` make.
  Stored per view: the label view (uint8), the embedding over the un-padded region, `cluster_index` (int16), prototypes
  and labels; once: the image and the concatenated bank.  The scaled images are NOT stored (with them the file is 948 KB,
  more than any other N fixture): a test rebuilds them from the image with the same CPU `F.interpolate` call
  (`flip_scale_views`), and the stored embedding of every view pins the result.  The reference's tie order on a GPU is unspecified
  (scatter_add_ + argmax): a seed is taken only if in every segment of every view the top-1 and top-2 class counts
  differ (asserted here)."""
  import linecache
  import math
  import textwrap
  import spml.models.embeddings.resnet_deeplab as e_dl
  import spml.utils.general.common as g_common
  import spml.utils.segsort.common as s_common
  F = torch.nn.functional

  def ref_lines(path, first, last):
    txt = ''.join(linecache.getline(path, i) for i in range(first, last + 1))
    assert txt.strip(), path
    return textwrap.dedent(txt).replace('.cuda()', '').replace('.to("cuda:0")', '')

  msc_py = os.path.join(ref, 'pyscripts', 'inference', 'prototype_msc.py')
  src_view, src_once = ref_lines(msc_py, 126, 197), ref_lines(msc_py, 204, 206)
  assert src_view.lstrip().startswith('# Create the ending index of each patch.') and 'cuda' not in src_view
  assert 'patch_ind_h' in src_view and 'embeddings[k] /= counts' in src_view and 'generate_clusters' in src_view
  assert 'segsort_common.calculate_prototypes_from_labels(' in src_view
  assert 'segsort_common.find_majority_label_index(' in src_view and "label_batch['semantic_label']" in src_view
  assert src_view.rstrip().endswith("prototype_results['prototype_label'].append(prototype_labels)")
  assert 'np.concatenate(v, axis=0)' in src_once and 'prototype_results[k] = v' in src_once
  pyramid = ref_lines(msc_py, 92, 95)
  assert 'scales=[0.5, 1, 1.5]' in pyramid and 'is_flip=False' in pyramid
  scales = (0.5, 1, 1.5)

  shimmed = cpu_shimmed_segment_by_kmeans(s_common)
  StubEmbedder = stub_embedder_class(e_dl)
  store = {}
  # (seed, C, classes, image, crop, stride, k-means grid, label cells, share of 255 cells).  Case 0: the views are
  # 22 x 30 (padded to the crop, one window), 44 x 60 (1 x 2 windows) and 66 x 90 (2 x 3 windows).  Case 1: label cells
  # hold the ignore value 255, so the class count of the bank pass is 256 and some prototypes carry 255.
  cases = [(2000, 16, 5, (44, 60), (48, 48), (32, 32), (3, 3), 4, 0.0),
           (2010, 8, 5, (40, 52), (48, 48), (32, 32), (5, 4), 4, 0.25)]
  orig = e_dl.segsort_common.segment_by_kmeans
  e_dl.segsort_common.segment_by_kmeans = shimmed
  try:
    for ci, (seed, c, ncls, image_hw, crop, stride, grid, cells, ignored) in enumerate(cases):
      gen = torch.Generator().manual_seed(seed)
      torch.manual_seed(seed)
      image_h, image_w = image_hw
      conv = torch.nn.Conv2d(3, c, 5, padding=2)
      base = torch.randn(1, 3, image_h // 8 + 2, image_w // 8 + 2, generator=gen)
      image = F.interpolate(base, size=image_hw, mode='bilinear', align_corners=False)
      image = image + 0.05 * torch.randn(1, 3, image_h, image_w, generator=gen)
      label = blocky_labels(gen, 1, image_h, image_w, cells, 0, ncls)[0]
      if ignored:
        drop = blocky_labels(gen, 1, image_h, image_w, cells, 0, 1000)[0] < int(1000 * ignored)
        label = label.masked_fill(drop, 255)
      cfg = AttrDict(dataset=AttrDict(semantic_ignore_index=255, num_classes=ncls),
                     network=AttrDict(label_divisor=2048), test=AttrDict(stride=list(stride), crop_size=list(crop)))
      t = 'c%d_' % ci
      views, prototype_results = [], {'prototype': [], 'prototype_label': []}
      for vi, scale in enumerate(scales):
        size = (max(int(round(image_h * scale)), 1), max(int(round(image_w * scale)), 1))
        scaled = image if scale == 1 else F.interpolate(image, size=size, mode='bilinear', align_corners=False)
        rh, rw = scaled.shape[-2:]
        lab = label if scale == 1 else F.interpolate(label[None, None].float(), size=(rh, rw), mode='nearest')[0, 0].long()
        pad_h, pad_w = max(rh, crop[0]), max(rw, crop[1])
        view = torch.zeros(1, 3, pad_h, pad_w)
        view[:, :, :rh, :rw] = scaled
        fake = torch.full((1, pad_h, pad_w), 255, dtype=torch.long)
        fake[:, :rh, :rw] = 0                                 # :109-120
        env = {'config': cfg, 'math': math, 'np': np, 'torch': torch, 'image_batch': {'image': view},
               'pad_image_h': pad_h, 'pad_image_w': pad_w, 'embedding_model': StubEmbedder(conv, list(grid)),
               'common_utils': g_common, 'segsort_common': s_common,
               'fake_label_batch': {'semantic_label': fake, 'instance_label': fake.clone()},
               'label_batch': {'semantic_label': lab.unsqueeze(0)}, 'prototype_results': prototype_results}
        with torch.no_grad():
          exec(compile(src_view, msc_py + ':126-197', 'exec'), env)
        protos, plab = torch.from_numpy(env['prototypes']), torch.from_numpy(env['prototype_labels'])
        clu = env['embeddings']['cluster_index']
        m = protos.shape[0]
        assert clu.shape[0] == rh * rw and int(clu.min()) == 0 and int(clu.max()) + 1 == m == plab.shape[0] <= 32767
        assert protos.dtype == torch.float32 and plab.dtype == torch.int64
        # the tie condition: top-1 and top-2 class counts of every segment differ
        width = int(lab.max()) + 1
        hist = torch.bincount(clu * width + lab.reshape(-1), minlength=m * width).view(m, width)
        top2 = hist.topk(2, dim=1).values if width > 1 else torch.cat([hist, hist * 0 - 1], 1)
        assert (top2[:, 0] > top2[:, 1]).all(), 'case %d view %d: a segment ties -- pick another seed' % (ci, vi)
        assert torch.equal(hist.argmax(1), plab)
        views.append([pad_h, pad_w, rh, rw, m])
        store[t + 'label%d' % vi] = lab.to(torch.uint8)
        store[t + 'embedding%d' % vi] = env['embeddings']['embedding'][..., :rh, :rw].contiguous()
        store[t + 'cluster_index%d' % vi] = clu.to(torch.int16)
        store[t + 'prototypes%d' % vi] = protos
        store[t + 'prototype_labels%d' % vi] = plab.to(torch.uint8)
      env = {'np': np, 'prototype_results': prototype_results}
      exec(compile(src_once, msc_py + ':204-206', 'exec'), env)
      bank, bank_lab = prototype_results['prototype'], prototype_results['prototype_label']
      total = sum(v[4] for v in views)
      assert bank.shape == (total, c) and bank.dtype == np.float32 and bank_lab.shape == (total,)
      n_ignored = int((bank_lab == 255).sum())
      print('n10 case %d (seed %d): views %s, %d prototypes, labels %s, %d with the ignore label'
            % (ci, seed, [(v[2], v[3], v[4]) for v in views], total, np.unique(bank_lab).tolist(), n_ignored))
      assert np.unique(bank_lab).size >= 3, 'case %d: fewer than 3 labels in the bank -- pick another seed' % ci
      assert (n_ignored > 0) == bool(ignored) and n_ignored < total // 2, 'case %d: pick another seed' % ci
      store.update({
          t + 'conv_w': conv.weight, t + 'conv_b': conv.bias, t + 'views': np.array(views), t + 'image': image,
          t + 'cfg': np.array([c, ncls, image_h, image_w, crop[0], crop[1], stride[0], stride[1], grid[0], grid[1]]),
          t + 'bank': bank, t + 'bank_lab': bank_lab.astype(np.uint8)})
  finally:
    e_dl.segsort_common.segment_by_kmeans = orig
  save(out, 'n10_prototype_msc', **store)
  if ONLY is None or 'n10_prototype_msc' in ONLY:
    size = os.path.getsize(os.path.join(out, 'n10_prototype_msc.npz'))
    assert size < 880 * 1024, 'n10_prototype_msc.npz is %d bytes' % size      # (no larger than the largest N fixture)


class _NumpyWithBool:
  """`np` for the exec of pseudo_inference_crf_msc.py:138-141: `np.bool` left numpy in 1.24; everything else is numpy's."""
  bool = bool

  def __getattr__(self, name):
    return getattr(np, name)


def gen_n11(ref, out):
  """N11: the tag recipe's kNN pseudo labels.  pyscripts/inference/pseudo_inference_crf_msc.py:138-141 exec'd for the
  tags, :172-241 per view (the lines of inference_msc.py:157-226, see `gen_n9`) and :252-263 + :275 once (mean over the
  views, per-class maximum, floor 0.15, 1 for the untagged classes, division; arg-max -- the denseCRF of :273 between
  them is out of scope), with the arrangement of `gen_n9`: stub embedder, CPU-shimmed k-means, the reference's `Segsort`,
  a perturbed bank, CPU `F.interpolate` in the place of `cv2.resize`.  Both cases use the recipe's four scales x flip.
  The bank's labels are drawn per coarse cell over the classes but the last; the last class takes a few single entries,
  so that its votes stay under the floor.  The image's label map (the source of the tags) carries every class but one
  strong one.  Stored per view what N9 stores (`cluster_index`, per-segment `topk`, the vote map); the image once (the
  views are `flip_scale_views`' of it: tests rebuild them); once `label_map`, `label_tags`, `divisor`, the normalised
  `semantic_prob`, `semantic_pred`, the un-normalised `mean_prob` and the top-1 minus top-2 `margin` of the normalised
  map.  Asserted (seeds are advanced until all hold): every normalisation branch is met, at least 3 classes win, the
  normalised labels differ from the plain arg-max of the mean on at least 5 % of the pixels, and at most 1 % of the
  pixels have a margin under 2e-4 * max|semantic_prob| (the N7 rule; the cap is NOT raised: two tagged classes that
  peak on one vote plateau tie on all of it, and such seeds are rejected)."""
  import linecache
  import math
  import textwrap
  import spml.models.embeddings.resnet_deeplab as e_dl
  import spml.models.predictions.segsort as p_segsort
  import spml.utils.general.common as g_common
  import spml.utils.segsort.common as s_common
  F = torch.nn.functional

  def ref_lines(path, first, last):
    txt = ''.join(linecache.getline(path, i) for i in range(first, last + 1))
    assert txt.strip(), path
    return textwrap.dedent(txt).replace('.cuda()', '').replace('.to("cuda:0")', '')

  msc_py = os.path.join(ref, 'pyscripts', 'inference', 'pseudo_inference_crf_msc.py')
  src_tags, src_view = ref_lines(msc_py, 138, 141), ref_lines(msc_py, 172, 241)
  src_norm, src_pred = ref_lines(msc_py, 252, 263), ref_lines(msc_py, 275, 275)
  assert 'np.unique(original_label_batch' in src_tags and 'dtype=np.bool' in src_tags
  assert 'patch_ind_h' in src_view and '[..., :resize_image_h, :resize_image_w]' in src_view and 'cuda' not in src_view
  assert 'with_prediction=True' in src_view and 'torch.mean(semantic_topk, dim=1)' in src_view
  assert src_view.rstrip().endswith('semantic_topk.view(resize_image_h, resize_image_w, -1)')
  assert 'np.mean(semantic_topks, axis=0)' in src_norm and 'np.maximum(max_prob, 0.15)' in src_norm
  assert 'max_prob[~label_tags, :, :] = 1' in src_norm and src_norm.rstrip().endswith('semantic_prob / max_prob')
  assert 'np.argmax(semantic_prob, axis=0)' in src_pred
  assert 'scales=[0.5, 1, 1.5, 2]' in ref_lines(msc_py, 133, 136)
  resize_src = ref_lines(msc_py, 245, 248)
  assert 'cv2.INTER_LINEAR' in resize_src and 'semantic_topk[:, ::-1]' in resize_src

  ns = {'segment_by_kmeans': cpu_shimmed_segment_by_kmeans(s_common)}
  StubEmbedder = stub_embedder_class(e_dl)
  scales = (0.5, 1, 1.5, 2)
  floor32 = np.float32(0.15)

  def one_case(seed, c, ncls, image_hw, crop, stride, grid, n_bank):
    """-> (store dict, report dict), or (None, reason) when a condition fails for this seed."""
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    image_h, image_w = image_hw
    conv = torch.nn.Conv2d(3, c, 5, padding=2)
    base = torch.randn(1, 3, image_h // 8 + 2, image_w // 8 + 2, generator=gen)
    image = F.interpolate(base, size=image_hw, mode='bilinear', align_corners=False)
    image = image + 0.05 * torch.randn(1, 3, image_h, image_w, generator=gen)
    cfg = AttrDict(
        train=AttrDict(sem_ann_loss_types='none', sem_occ_loss_types='none', img_sim_loss_types='none',
                       feat_aff_loss_types='none', sem_ann_concentration=0.0, sem_occ_concentration=0.0,
                       img_sim_concentration=0.0, feat_aff_concentration=0.0, sem_ann_loss_weight=0.0,
                       sem_occ_loss_weight=0.0, img_sim_loss_weight=0.0, feat_aff_loss_weight=0.0),
        dataset=AttrDict(semantic_ignore_index=255, num_classes=ncls),
        network=AttrDict(label_divisor=2048),
        test=AttrDict(stride=list(stride), crop_size=list(crop)))
    predictor = p_segsort.Segsort(cfg)
    with torch.no_grad():
      full = g_common.normalize_embedding(conv(image).permute(0, 2, 3, 1).reshape(-1, c))
    pick = torch.randint(0, full.shape[0], (n_bank,), generator=gen)
    bank = g_common.normalize_embedding(full[pick] + 0.1 * torch.randn(n_bank, c, generator=gen))
    bank_lab = blocky_labels(gen, 1, image_h, image_w, 4, 0, ncls - 1)[0].reshape(-1)[pick]
    weak = ncls - 1                                         # a few single entries: votes of 1/20 or 2/20 at most places
    bank_lab[torch.randperm(n_bank, generator=gen)[:max(n_bank // 40, 4)]] = weak
    # the image's label map: every class but one strong one, in stripes, with unlabelled (255) gaps
    untagged = int(torch.randint(0, ncls - 1, (1,), generator=gen))
    carried = [k for k in range(ncls) if k != untagged]
    label_map = np.full(image_hw, 255, dtype=np.uint8)
    for j, k in enumerate(carried):
      label_map[:, j * image_w // len(carried):(j + 1) * image_w // len(carried) - 1] = k
    env = {'np': _NumpyWithBool(), 'config': cfg, 'original_label_batch': {'semantic_label': label_map}}
    exec(compile(src_tags, msc_py + ':138-141', 'exec'), env)
    label_tags = env['label_tags']
    assert label_tags.dtype == np.bool_ and label_tags.tolist() == [k != untagged for k in range(ncls)]

    per_view, views, semantic_topks = {}, [], []
    for si, scale in enumerate(scales):
      size = (max(int(round(image_h * scale)), 1), max(int(round(image_w * scale)), 1))
      scaled = image if scale == 1 else F.interpolate(image, size=size, mode='bilinear', align_corners=False)
      rh, rw = scaled.shape[-2:]
      pad_h, pad_w = max(rh, crop[0]), max(rw, crop[1])
      for flip in (True, False):                            # create_image_pyramid: the flipped view first
        view = torch.zeros(1, 3, pad_h, pad_w)
        view[:, :, :rh, :rw] = torch.flip(scaled, dims=[3]) if flip else scaled
        fake = torch.full((1, pad_h, pad_w), 255, dtype=torch.long)
        fake[:, :rh, :rw] = 0                               # :155-166
        env = {'config': cfg, 'math': math, 'np': np, 'torch': torch, 'image_batch': {'image': view},
               'pad_image_h': pad_h, 'pad_image_w': pad_w, 'resize_image_h': rh, 'resize_image_w': rw,
               'embedding_model': StubEmbedder(conv, list(grid)), 'prediction_model': predictor,
               'common_utils': g_common, 'fake_label_batch': {'semantic_label': fake, 'instance_label': fake.clone()},
               'semantic_memory_prototypes': bank, 'semantic_memory_prototype_labels': bank_lab}
        with torch.no_grad():
          exec(compile(src_view, msc_py + ':172-241', 'exec'), env)
        votes = env['semantic_topk']
        assert tuple(votes.shape) == (rh, rw, ncls) and votes.dtype == torch.float32
        # :243-248 with F.interpolate in the place of cv2.resize
        resized = F.interpolate(votes.permute(2, 0, 1).unsqueeze(0), size=image_hw, mode='bilinear',
                                align_corners=False)[0].permute(1, 2, 0).numpy().astype(np.float32)
        if flip:
          resized = resized[:, ::-1]
        semantic_topks.append(resized)
        score = env['outputs']['semantic_score']
        _, clu = torch.unique(env['embeddings']['cluster_index'], return_inverse=True)
        m = int(clu.max()) + 1
        assert tuple(score.shape) == (rh * rw, 20) and clu.shape[0] == rh * rw
        first = torch.full((m,), rh * rw, dtype=torch.long).scatter_reduce(0, clu, torch.arange(rh * rw), 'amin')
        topk = score[first]
        assert torch.equal(topk[clu], score), 'the pixels of a segment disagree on their retrieved labels'
        assert m <= 32767 and int(topk.max()) < ncls
        vi = len(views)
        views.append([si, pad_h, pad_w, rh, rw, int(flip), m])
        per_view['cluster_index%d' % vi] = clu.to(torch.int16)
        per_view['topk%d' % vi] = topk.to(torch.uint8)
        per_view['votes%d' % vi] = np.ascontiguousarray(resized.transpose(2, 0, 1))
    plain = np.mean(np.stack(semantic_topks, axis=0).astype(np.float32), axis=0).transpose(2, 0, 1)
    env = {'np': np, 'semantic_topks': semantic_topks, 'label_tags': label_tags}
    exec(compile(src_norm, msc_py + ':252-263', 'exec'), env)
    prob, divisor = env['semantic_prob'], env['max_prob'].reshape(-1)
    exec(compile(src_pred, msc_py + ':275', 'exec'), env)
    pred = env['semantic_pred']
    assert prob.shape == (ncls, image_h, image_w) and prob.dtype == np.float32 and divisor.dtype == np.float32
    assert pred.shape == image_hw and pred.dtype == np.uint8
    peak = plain.reshape(ncls, -1).max(1)
    wins = np.bincount(pred.reshape(-1), minlength=ncls)
    top2 = torch.from_numpy(np.ascontiguousarray(prob)).topk(2, dim=0).values
    margin = top2[0] - top2[1]
    low = (margin < 2e-4 * float(np.abs(prob).max())).float().mean().item()
    moved = float((pred != np.argmax(plain, axis=0)).mean())
    report = dict(seed=seed, untagged=untagged, peak=np.round(peak, 3).tolist(), wins=wins.tolist(), low=low, moved=moved,
                  segments=[v[6] for v in views])
    checks = [
        ('a tagged class with a peak of at least 0.15', bool((label_tags & (peak >= floor32)).any())),
        ('a tagged class with votes under the floor', bool((label_tags & (peak < floor32) & (peak > 0)).any())),
        ('the untagged class has votes and wins pixels', peak[untagged] > 0 and wins[untagged] > 0),
        ('at least 3 classes win', int((wins > 0).sum()) >= 3),
        ('the normalisation moves at least 5 % of the labels', moved >= 0.05),
        ('at most 1 % of the pixels under the margin', low <= 0.01)]
    failed = [what for what, ok in checks if not ok]
    if failed:
      return None, dict(report, failed=failed)
    assert np.array_equal(divisor, np.where(label_tags, np.maximum(peak, floor32), np.float32(1)))
    store = dict(per_view)
    store.update({
        'image': image, 'conv_w': conv.weight, 'conv_b': conv.bias, 'bank': bank, 'bank_lab': bank_lab,
        'cfg': np.array([c, ncls, image_h, image_w, crop[0], crop[1], stride[0], stride[1], grid[0], grid[1]]),
        'scales': np.array(scales, dtype=np.float64), 'views': np.array(views), 'label_map': label_map,
        'label_tags': label_tags, 'divisor': divisor, 'mean_prob': np.ascontiguousarray(plain),
        'semantic_prob': np.ascontiguousarray(prob), 'semantic_pred': pred, 'margin': margin})
    return store, report

  # (first seed, C, classes, image, crop, stride, k-means grid, bank size).  (a) image = crop: the scale-1 views are not
  # padded; (b) odd width, a padded 0.5 view (18 x 23 in 24 x 24) and 4 x 6 windows at scale 2 (72 x 90, stride 16).
  cases = [(2100, 16, 5, (44, 60), (44, 60), (30, 30), (4, 4), 400),
           (2200, 16, 6, (36, 45), (24, 24), (16, 16), (3, 3), 300)]
  store = {}
  orig = e_dl.segsort_common.segment_by_kmeans
  e_dl.segsort_common.segment_by_kmeans = ns['segment_by_kmeans']
  try:
    for ci, (seed0, c, ncls, image_hw, crop, stride, grid, n_bank) in enumerate(cases):
      for seed in range(seed0, seed0 + 40):
        got, report = one_case(seed, c, ncls, image_hw, crop, stride, grid, n_bank)
        print('n11 case %d: %s' % (ci, report))
        if got is not None:
          break
      else:
        raise AssertionError('n11 case %d: no seed in %d .. %d meets the conditions' % (ci, seed0, seed0 + 39))
      store.update({'c%d_%s' % (ci, k): v for k, v in got.items()})
      store['c%d_seed' % ci] = np.array(seed)
  finally:
    e_dl.segsort_common.segment_by_kmeans = orig
  save(out, 'n11_pseudo_knn_msc', **store)
  size = os.path.getsize(os.path.join(out, 'n11_pseudo_knn_msc.npz'))
  assert size <= 600 * 1024, 'n11_pseudo_knn_msc.npz is %d bytes' % size


def gen_n11_instance(ref, out):
  """The instance-weighted IoU of pyscripts/benchmark/benchmark_by_instance.py: its own `iou_stats` (:27-55) and the
  lines :88-113 exec'd per image, :115-116 and :139 once, on seeded uint8 maps of 40 x 52 -- three images for 21 classes
  and two for 15.  Among them: an instance all of whose pixels are 255 in the ground truth (it counts for class 0), an
  instance tied between two classes (the lower one), an image with all 256 ids (`if i < 255` drops the largest), an
  image with one id, and ground-truth values between the class count and 255 (outside the histogram's range).  Stored:
  `pred`, `gt`, `inst` (uint8), the per-image `ninst_`, the final `iou` and `mean_iou`."""
  import linecache
  import textwrap
  py = os.path.join(ref, 'pyscripts', 'benchmark', 'benchmark_by_instance.py')

  def ref_lines(first, last):
    txt = ''.join(linecache.getline(py, i) for i in range(first, last + 1))
    assert txt.strip(), py
    return textwrap.dedent(txt)

  src_stats, src_image, src_final, src_mean = ref_lines(27, 55), ref_lines(88, 113), ref_lines(115, 116), ref_lines(139, 139)
  assert src_stats.startswith('def iou_stats(') and 'if i < 255:' in src_image and 'ninst += ninst_' in src_image
  assert 'range=(0, args.num_classes-1)' in src_image and 'iou /= ninst+1e-12' in src_final and 'mean_iou' in src_mean
  h, w = 40, 52
  for nc in (15, 21):     # np.histogram(bins=nc, range=(0, nc-1)) bins the integers 0 .. nc-1 as themselves
    for v in range(nc):
      hist, _ = np.histogram(np.array([v], dtype=np.uint8), bins=nc, range=(0, nc - 1))
      assert int(np.argmax(hist)) == v and hist.sum() == 1, (nc, v)
    assert np.histogram(np.array([nc, 254, 255], dtype=np.uint8), bins=nc, range=(0, nc - 1))[0].sum() == 0

  def blocky(rng, cells_y, cells_x, values):
    grid = rng.choice(values, size=(cells_y, cells_x))
    return np.ascontiguousarray(grid[np.arange(h) * cells_y // h][:, np.arange(w) * cells_x // w].astype(np.uint8))

  def blocky_image(rng, nc):
    """A few instances (ids 0, 3, 5, 9, 200, 255 ...) over a blocky ground truth; id 3 is unlabelled throughout and
    id 5 is split evenly between two classes."""
    inst = blocky(rng, 4, 4, np.array([0, 3, 5, 9, 200, 255]))
    inst[:10, :13], inst[10:20, :13], inst[:10, 13:26] = 3, 5, 0              # (every special id occurs)
    gt = blocky(rng, 5, 6, np.arange(nc))
    gt[rng.random((h, w)) < 0.1] = 255
    gt[rng.random((h, w)) < 0.03] = min(nc + 2, 254)                           # neither a class nor 255
    gt[inst == 3] = 255
    five = np.flatnonzero(inst.reshape(-1) == 5)
    assert five.size % 2 == 0 and five.size > 0
    a, b = sorted(rng.choice(np.arange(1, nc), size=2, replace=False).tolist())
    flat = gt.reshape(-1)
    assert flat.base is gt
    flat[five[:five.size // 2]], flat[five[five.size // 2:]] = b, a
    return inst, gt, (a, b)

  store = {}
  for nc, kinds in ((21, ('blocky', 'all_ids', 'one_id')), (15, ('blocky', 'all_ids'))):
    rng = np.random.default_rng(1100 + nc)
    env = {'np': np}
    exec(compile(src_stats, py + ':27-55', 'exec'), env)
    env.update(args=AttrDict(num_classes=nc), iou=np.zeros(nc, dtype=np.float64), ninst=np.zeros(nc, dtype=np.float64))
    for ii, kind in enumerate(kinds):
      if kind == 'blocky':
        inst, gt, (a, b) = blocky_image(rng, nc)
      elif kind == 'all_ids':
        inst = rng.permutation(np.arange(h * w) % 256).reshape(h, w).astype(np.uint8)
        gt = rng.integers(0, nc, size=(h, w)).astype(np.uint8)
        gt[rng.random((h, w)) < 0.2] = 255
      else:
        inst = np.full((h, w), 7, dtype=np.uint8)
        gt = blocky(rng, 3, 3, np.arange(nc))
      pred = np.where(rng.random((h, w)) < 0.7, np.minimum(gt, nc - 1), rng.integers(0, nc, size=(h, w))).astype(np.uint8)
      env.update(pred=pred, gt=gt, inst=inst)
      exec(compile(src_image, py + ':88-113', 'exec'), env)
      ninst_ = env['ninst_']
      ids = np.unique(inst)
      if kind == 'blocky':
        assert {0, 3, 5, 255} <= set(ids.tolist()) and (gt[inst == 3] == 255).all()
        counts5 = np.bincount(gt[inst == 5], minlength=256)
        assert counts5[a] == counts5[b] == counts5[:nc].max() and a < b
        assert ninst_.sum() == ids.size
      elif kind == 'all_ids':
        assert ids.size == 256 and ninst_.sum() == 255
      else:
        assert ids.size == 1 and ninst_.sum() == 1
      t = 'n%d_i%d_' % (nc, ii)
      store.update({t + 'pred': pred, t + 'gt': gt, t + 'inst': inst, t + 'ninst': ninst_.copy()})
    exec(compile(src_final, py + ':115-116', 'exec'), env)
    exec(compile(src_mean, py + ':139', 'exec'), env)
    assert np.isfinite(env['iou']).all() and 0.0 < env['mean_iou'] < 100.0
    store.update({'n%d_images' % nc: np.array(len(kinds)), 'n%d_iou' % nc: env['iou'], 'n%d_mean_iou' % nc: np.array(env['mean_iou'])})
    print('n11 instance IoU, %d classes: %d images, mean IoU %.4f' % (nc, len(kinds), env['mean_iou']))
  save(out, 'n11_instance_iou', **store)


# (seed, C, image, k-means grid, tagged classes).  (a) half map 20 x 28 -> 5 x 7, scale exactly 4; (b) half map 21 x 30 ->
# 5 x 7: scales 4.2 and 30 / 7, the taps of the last row and column clamp at the border.  Seeds: the first from 2100 / 2150
# on that meet every condition asserted in gen_n12 (2100, 2101: a pixel's two nearest prototypes 1.6e-5 apart; 2150
# passes at once).
N12_CASES = [(2102, 8, (40, 56), (4, 4), (2, 7, 11)), (2150, 8, (43, 61), (4, 5), (0, 5, 14))]


def gen_n12(ref, out):
  """N12: DensePose pseudo labels.  pyscripts/inference/pseudo_denseposerw_crf.py:137-142 (the affinity), :145-168 (labels
  to the half map, k-means, tag propagation by the nearest labelled prototype), :172-190 (per-segment shares, the map at
  1/8 of the image, the normalisation by each class's maximum, the tag mask) and :193-201 (the walk), exec'd from the
  reference's own lines on seeded CPU inputs, with the stub embedder's `generate_clusters` (the reference's own, on the
  CPU-shimmed segment_by_kmeans).  The input is the half-resolution embedding itself (what :130-135 leave).  The lines
  hard-code 15 classes.  cv2 is not installed and :203-207 are the tail that `n7_pseudo_labels` pins already.  The
  retrieval inside `gather_multiset_labels_per_batch_by_nearest_neighbor` is not visible from outside: the nearest index
  and value are recomputed with that function's own expressions (models/utils.py:198-206) and asserted to reproduce its
  result.  The fixture pins the defined behaviour: every tagged class has a non-zero maximum, nothing is NaN, and every
  pixel's nearest labelled prototype leads the second one by more than 1e-4 (asserted; another seed otherwise), so that
  the last bits of another normalisation cannot move a pixel to another prototype."""
  import linecache
  import textwrap
  import spml.models.embeddings.resnet_deeplab as e_dl
  import spml.models.utils as model_utils
  import spml.utils.general.common as g_common
  import spml.utils.segsort.common as s_common
  F = torch.nn.functional

  def ref_lines(first, last):
    txt = ''.join(linecache.getline(py, i) for i in range(first, last + 1))
    assert txt.strip(), py
    return textwrap.dedent(txt).replace('.cuda()', '')

  py = os.path.join(ref, 'pyscripts', 'inference', 'pseudo_denseposerw_crf.py')
  src_aff, src_tags, src_cam, src_walk = ref_lines(137, 142), ref_lines(145, 168), ref_lines(172, 190), ref_lines(193, 201)
  assert src_aff.lstrip().startswith('# Create affinity matrix') and 'exp_()' in src_aff
  assert 'generate_clusters' in src_tags and src_tags.rstrip().endswith('label_divisor=config.network.label_divisor)')
  assert src_cam.lstrip().startswith('s_probs = common_utils.segment_mean') and 'cam_full_arr[0] = TH' in src_cam
  assert 'aff_mat = aff ** 20' in src_walk and src_walk.rstrip().endswith('cam_rw.view(15, cam_shape[0], cam_shape[1])')
  walk_steps = [int(linecache.getline(py, i).split('=')[1]) for i in range(20, 40)
                if linecache.getline(py, i).startswith('WALK_STEPS')]
  assert walk_steps == [6]

  ncls, divisor = 15, 2048
  cfg = AttrDict(dataset=AttrDict(num_classes=ncls), network=AttrDict(label_divisor=divisor))
  StubEmbedder = stub_embedder_class(e_dl)
  store = {}
  cases = N12_CASES
  orig = e_dl.segsort_common.segment_by_kmeans
  e_dl.segsort_common.segment_by_kmeans = cpu_shimmed_segment_by_kmeans(s_common)
  try:
    for ci, (seed, c, image_hw, grid, tags) in enumerate(cases):
      gen = torch.Generator().manual_seed(seed)
      image_h, image_w = image_hw
      h2, w2 = image_h // 2, image_w // 2
      emb = coherent_embedding(gen, 1, c, h2, w2)
      # a blocky class map over the three tagged classes, about 10 % of its pixels kept (the others unlabelled: 254),
      # and an ignore strip (255) along the right edge; the instance label is the cell
      cells = blocky_labels(gen, 1, image_h, image_w, 3, 0, 3)[0]
      dense = torch.tensor(tags)[cells]
      keep = torch.rand(image_h, image_w, generator=gen) < 0.10
      semantic = torch.where(keep, dense, torch.full_like(dense, 254))
      semantic[:, image_w - 4:] = 255
      instance = blocky_labels(gen, 1, image_h, image_w, 3, 0, 4)[0]
      label_tags = torch.zeros(ncls, dtype=torch.bool)
      present = torch.unique(semantic)
      label_tags[present[present < ncls]] = True                       # :106-110
      assert label_tags.nonzero().view(-1).tolist() == sorted(tags)
      lab = semantic.clone()
      lab[lab == 255] = ncls                                           # :121-123
      env = {'torch': torch, 'F': F, 'config': cfg, 'common_utils': g_common, 'segsort_common': s_common,
             'model_utils': model_utils, 'embeddings': {'embedding': emb.clone()}, 'image_h': image_h, 'image_w': image_w,
             'label_batch': {'semantic_label': lab.unsqueeze(0), 'instance_label': instance.unsqueeze(0)},
             'embedding_model': StubEmbedder(None, list(grid)), 'label_tags': label_tags.clone(), 'TH': None,
             'WALK_STEPS': walk_steps[0]}
      with torch.no_grad():
        exec(compile(src_aff, py + ':137-142', 'exec'), env)
        exec(compile(src_tags, py + ':145-168', 'exec'), env)
        s_labs, c_inds, s_tags = env['s_labs'], env['c_inds'], env['s_tags']
        clusterings = env['clusterings']
        # the retrieval of models/utils.py:198-206 again, for its index and value
        rows, protos = clusterings['cluster_embedding'], env['protos']
        valid = (s_labs < ncls).view(1, -1)
        dists = torch.mm(rows, protos.t())
        dists = torch.where(valid.expand_as(dists), dists, dists.min() - 1)
        top2 = torch.topk(dists, 2, dim=1)
        nn_value, nn_index = top2.values[:, 0], top2.indices[:, 0]
        assert torch.equal(g_common.one_hot(s_labs[nn_index].view(-1, 1), ncls + 1).sum(1)[:, :ncls], s_tags)
        lead = float((top2.values[:, 0] - top2.values[:, 1]).min())
        exec(compile(src_cam, py + ':172-190', 'exec'), env)
        s_probs, resampled, cam = env['s_probs'], env['semantic_probs'], env['cam_full_arr']
        exec(compile(src_walk, py + ':193-201', 'exec'), env)
      trans = env['aff_mat'] / torch.sum(env['aff_mat'], dim=0, keepdim=True)
      cam_rw = env['cam_rw']
      n, oh, ow = h2 * w2, image_h // 8, image_w // 8
      m = int(s_labs.shape[0])
      assert tuple(c_inds.shape) == (n,) == tuple(nn_index.shape) and int(c_inds.max()) + 1 == m
      assert tuple(s_probs.shape) == (m, ncls) and tuple(resampled.shape) == (1, ncls, oh, ow)
      assert tuple(cam.shape) == (1, ncls, oh, ow) and tuple(cam_rw.shape) == (ncls, oh, ow)
      assert tuple(trans.shape) == (oh * ow, oh * ow)
      peaks = cam[0].reshape(ncls, -1).max(1).values
      print('n12 case %d (seed %d): %d segments (%d labelled), nearest prototype leads by %.2e, class peaks %s'
            % (ci, seed, m, int(valid.sum()), lead, [round(float(v), 3) for v in peaks[label_tags]]))
      assert not any(bool(torch.isnan(t).any()) for t in (s_probs, resampled, cam, cam_rw)), 'NaN -- pick another seed'
      assert bool((peaks[label_tags] == 1).all()) and bool((peaks[~label_tags] == 0).all()), 'pick another seed'
      assert lead > 1e-4, 'a pixel sits between two prototypes -- pick another seed'
      assert bool(torch.equal(torch.bincount(c_inds, minlength=m) > 0, torch.ones(m, dtype=torch.bool)))
      t = 'c%d_' % ci
      store.update({
          t + 'cfg': np.array([c, ncls, image_h, image_w, grid[0], grid[1], divisor, walk_steps[0]]),
          t + 'embedding': emb[0], t + 'semantic_label': semantic.to(torch.uint8),
          t + 'instance_label': instance.to(torch.uint8), t + 'tags': label_tags,
          t + 'cluster_embedding': rows, t + 'cluster_semantic_label': clusterings['cluster_semantic_label'].to(torch.int16),
          t + 'raw_cluster_index': clusterings['cluster_index'].to(torch.int16),
          t + 'cluster_index': c_inds.to(torch.int16), t + 'proto_label': s_labs.to(torch.int16),
          t + 'nn_index': nn_index.to(torch.int16), t + 'nn_value': nn_value, t + 's_tags': s_tags.to(torch.uint8),
          t + 's_probs': s_probs, t + 'semantic_probs': resampled[0], t + 'cam_full_arr': cam[0], t + 'trans': trans,
          t + 'cam_rw': cam_rw})
  finally:
    e_dl.segsort_common.segment_by_kmeans = orig
  save(out, 'n12_densepose_pseudo', **store)
  size = os.path.getsize(os.path.join(out, 'n12_densepose_pseudo.npz'))
  assert size < 600 * 1024, 'n12_densepose_pseudo.npz is %d bytes' % size


def gen_n13(ref, out):
  """N13: the numpy-only stages of the training augmentation.  `spml/data/transforms.py` imports cv2, which is not
  installed: an empty module stands in for it in memory while the file is imported (none of the functions called here
  touches it).  `transforms.mirror`, `resize_with_pad` and `random_crop_with_pad` (with `return_bbox`, under a seeded
  `np.random`) are the reference's own functions; the grayscale lines (list_tag_dataset.py:202-205), the blur-weight lines
  (:210-212) and the tag lines (:76-78) are exec'd from the reference's file.  `cv2.resize` and `cv2.filter2D` themselves
  cannot be run: tests/augment_ref.py restates them and tests/test_augment.py holds those two to ATen on the CPU."""
  import linecache
  import textwrap
  had = sys.modules.get('cv2')
  sys.modules['cv2'] = types.ModuleType('cv2')
  try:
    import spml.data.transforms as transforms
  finally:
    if had is None:
      del sys.modules['cv2']
    else:
      sys.modules['cv2'] = had
  py = os.path.join(ref, 'spml', 'data', 'datasets', 'list_tag_dataset.py')

  def ref_lines(first, last):
    txt = ''.join(linecache.getline(py, i) for i in range(first, last + 1))
    assert txt.strip(), py
    return textwrap.dedent(txt)

  src_gray, src_weight, src_tags = ref_lines(202, 205), ref_lines(210, 212), ref_lines(76, 78)
  assert src_gray.startswith('rgb2gray = np.array([0.3, 0.59, 0.11]') and 'np.tile(image, (1,1,3))' in src_gray
  assert src_weight.startswith('w_x, w_y = np.meshgrid') and src_weight.rstrip().endswith('weight / weight.sum()')
  assert src_tags.startswith('cats = np.unique(semantic_label)') and src_tags.rstrip().endswith('semantic_tags[cats] = 1')

  rng = np.random.RandomState(235)
  mean = (0.485, 0.456, 0.406)
  store = {'mean': np.array(mean)}
  # (h, w, crop): both sides below the crop, one above and one below, both above, equal to the crop
  for ci, (h, w, crop) in enumerate([(5, 7, (9, 11)), (13, 6, (9, 11)), (17, 19, (9, 11)), (9, 11, (9, 11))]):
    image = (rng.randint(0, 256, (h, w, 3)).astype(np.float32) / 255).astype(np.float32)
    label = np.stack([rng.choice(np.array([0, 3, 14, 254, 255], np.uint8), (h, w)),
                      rng.randint(0, 256, (h, w)).astype(np.uint8)], axis=2)
    m_image, m_label = transforms.mirror(image, label)
    p_image = transforms.resize_with_pad(image, crop, mean)
    p_label = transforms.resize_with_pad(label, crop, 255)
    np.random.seed(1000 + ci)
    c_image, c_label, bbox = transforms.random_crop_with_pad(image, label, crop, mean, 255, return_bbox=True)
    env = {'np': np, 'image': c_image}
    exec(compile(src_gray, py + ':202-205', 'exec'), env)
    env_t = {'np': np, 'semantic_label': label[..., 0]}
    exec(compile(src_tags, py + ':76-78', 'exec'), env_t)
    t = 'c%d_' % ci
    store.update({t + 'image': image, t + 'label': label, t + 'crop': np.array(crop), t + 'mirror_image': m_image,
                  t + 'mirror_label': m_label, t + 'pad_image': p_image, t + 'pad_label': p_label,
                  t + 'crop_image': c_image, t + 'crop_label': c_label, t + 'bbox': np.array(bbox),
                  t + 'gray': env['image'], t + 'tags': env_t['semantic_tags']})
  sigmas = np.array([0.1, 0.7, 2.5, 5.0])
  weights = []
  for sigma in sigmas:
    env = {'np': np, 'sigma': float(sigma)}
    exec(compile(src_weight, py + ':210-212', 'exec'), env)
    weights.append(env['weight'])
  store.update({'sigmas': sigmas, 'weights': np.stack(weights)})
  save(out, 'n13_augment', **store)
  size = os.path.getsize(os.path.join(out, 'n13_augment.npz'))
  assert size < 100 * 1024, 'n13_augment.npz is %d bytes' % size


def gen_n14(ref, out):
  """N14: what the reference's inference programs ask of cv2 and do around it.  `spml/data/transforms.py` and
  `spml/utils/general/others.py` are imported with a RECORDING stand-in for cv2 in memory: its `resize` notes
  `(dsize, interpolation)` and returns an array of that size whose every pixel holds its own column index, so that a
  mirror of the resized array shows.  Recorded: the sizes `resize_with_interpolation` and `resize` request for a table
  of `(h, w, image_size)` and `(h, w, scale)` cases; the order, sizes, interpolation modes and flip flags of
  `create_image_pyramid`; `resize_with_pad` with 0; the uint8 table of `load_color_map` on `misc/colormapvoc.mat`
  (vis.py imports torchvision, which is not installed: an empty module stands in for it, none of it is called).
  cv2's pixels themselves cannot be run: tests/augment_ref.py restates them."""
  calls = []
  cv2 = types.ModuleType('cv2')
  cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1

  def resize(src, dsize, interpolation=1):
    calls.append((int(dsize[0]), int(dsize[1]), int(interpolation)))
    shape = (int(dsize[1]), int(dsize[0])) + tuple(src.shape[2:])
    ramp = np.arange(shape[1]).reshape((1, shape[1]) + (1,) * (len(shape) - 2))
    return np.broadcast_to(ramp, shape).astype(src.dtype)
  cv2.resize = resize
  stand_ins = {'cv2': cv2, 'torchvision': types.ModuleType('torchvision'), 'torchvision.utils': types.ModuleType('torchvision.utils')}
  stand_ins['torchvision'].utils = stand_ins['torchvision.utils']
  had = {name: sys.modules.get(name) for name in stand_ins}
  for name in ('spml.data.transforms', 'spml.utils.general.others'):      # (n13 may have imported them with its own cv2)
    sys.modules.pop(name, None)
  sys.modules.update(stand_ins)
  try:
    import spml.data.transforms as transforms
    import spml.utils.general.others as others
    import spml.utils.general.vis as vis
  finally:
    for name, module in had.items():
      if module is None:
        del sys.modules[name]
      else:
        sys.modules[name] = module
  assert transforms.cv2 is cv2

  store = {}
  interp_cases = [(23, 43, 23), (43, 23, 23), (375, 500, 513), (500, 375, 513), (41, 29, 33), (366, 500, 512),
                  (333, 500, 320), (17, 17, 40), (1, 9, 4)]
  sizes = []
  for h, w, size in interp_cases:
    del calls[:]
    got = transforms.resize_with_interpolation(np.zeros((h, w, 3), np.float32), size, method='bilinear')
    (new_w, new_h, inter), = calls
    assert inter == cv2.INTER_LINEAR and got.shape == (new_h, new_w, 3)
    sizes.append((new_h, new_w))
  store.update({'interp_cases': np.array(interp_cases), 'interp_sizes': np.array(sizes)})
  assert sizes[0] == (12, 22)

  scale_cases = [(375, 500, s) for s in (0.5, 0.75, 1, 1.25, 1.5)] + \
                [(23, 37, s) for s in (0.5, 1, 1.75)] + [(41, 29, s) for s in (0.5, 1, 1.75)] + \
                [(333, 500, 0.75), (281, 500, 1.25), (500, 334, 1.5), (3, 5, 0.5), (97, 113, 0.7)]
  sizes = []
  for h, w, scale in scale_cases:
    del calls[:]
    transforms.resize(np.zeros((h, w, 3), np.float32), np.zeros((h, w, 2), np.uint8), scale)
    (iw, ih, ii), (lw, lh, li) = calls
    assert (ii, li) == (cv2.INTER_LINEAR, cv2.INTER_NEAREST) and (iw, ih) == (lw, lh)
    sizes.append((ih, iw))
  store.update({'scale_cases': np.array(scale_cases, dtype=np.float64), 'scale_sizes': np.array(sizes)})

  # create_image_pyramid: order, sizes, flags; the first pixel of a mirrored view holds the last column's index
  for tag, (h, w), scales, is_flip in [('msc', (375, 500), [0.5, 0.75, 1, 1.25, 1.5], True),
                                       ('bank', (41, 29), [0.5, 1, 1.5], False),
                                       ('small', (23, 37), [0.5, 1, 1.75], True)]:
    del calls[:]
    batches = others.create_image_pyramid(
        {'image': np.zeros((3, h, w), np.float32)},
        {'semantic_label': np.zeros((h, w), np.uint8), 'instance_label': np.zeros((h, w), np.uint8)}, scales, is_flip)
    assert len(calls) == 2 * len(batches) and all(c[2] == (cv2.INTER_LINEAR, cv2.INTER_NEAREST)[i % 2] for i, c in enumerate(calls))
    store.update({
        tag + '_hw': np.array([h, w]), tag + '_scales': np.array(scales, dtype=np.float64), tag + '_is_flip': np.array(is_flip),
        tag + '_sizes': np.array([b[0]['image'].shape[-2:] for b in batches]),
        tag + '_label_sizes': np.array([b[1]['semantic_label'].shape for b in batches]),
        tag + '_flips': np.array([b[2]['is_flip'] for b in batches]),
        tag + '_first_column': np.array([int(b[0]['image'][0, 0, 0]) for b in batches]),
        tag + '_first_label_column': np.array([int(b[1]['semantic_label'][0, 0]) for b in batches])})

  rng = np.random.RandomState(914)
  for ci, (h, w, crop) in enumerate([(5, 7, (9, 11)), (13, 6, (9, 11)), (17, 19, (9, 11)), (9, 11, (9, 11))]):
    image = rng.standard_normal((h, w, 3)).astype(np.float32)
    store.update({'pad%d_image' % ci: image, 'pad%d_crop' % ci: np.array(crop),
                  'pad%d_out' % ci: transforms.resize_with_pad(image, crop, image_pad_value=0)})

  table = vis.load_color_map(os.path.join(ref, 'misc', 'colormapvoc.mat')).numpy()
  assert table.shape == (256, 3) and table.dtype == np.uint8
  store['color_map'] = table
  save(out, 'n14_inference_io', **store)
  size = os.path.getsize(os.path.join(out, 'n14_inference_io.npz'))
  assert size < 100 * 1024, 'n14_inference_io.npz is %d bytes' % size


def gen_n15(ref, out):
  """N15: scoring directories.  pyscripts/benchmark/benchmark_by_mIoU.py: its own `iou_stats` (:25-53), the per-file lines
  :80-88 and the final lines :90, :113, :116; pyscripts/benchmark/benchmark_by_instance.py: `iou_stats` (:27-55), the
  per-file lines :88-113 and the final lines :115-116, :139 -- exec'd as they stand on seeded uint8 triples, five files
  of different sizes for 21 classes and four for 15.  Between them: predictions equal to the class count (the
  histogram's last bin is closed on the right; over the last class they are still no true positive), above it and 255,
  all at counted pixels; ground truth between the class
  count and 254 and at 255; a file without a counted pixel; an instance all of whose pixels are uncounted (class 0); an
  instance tied between two classes (the lower one); a file with all 256 ids (`if i < 255` drops the largest); a file
  with one id; a 1 x 1 file.  Stored per file: `pred`, `gt`, `inst` (uint8) and `rows` int64 [4, ncls] (TP+FN, TP+FP,
  TP, instances per class); per class count the final `iou`, `mean_iou`, `pixel_acc` of the first program and
  `inst_iou`, `inst_mean_iou` of the second."""
  import linecache
  import textwrap
  py_m = os.path.join(ref, 'pyscripts', 'benchmark', 'benchmark_by_mIoU.py')
  py_i = os.path.join(ref, 'pyscripts', 'benchmark', 'benchmark_by_instance.py')

  def ref_lines(py, first, last):
    txt = ''.join(linecache.getline(py, i) for i in range(first, last + 1))
    assert txt.strip(), py
    return textwrap.dedent(txt)

  m_stats, m_file = ref_lines(py_m, 25, 53), ref_lines(py_m, 80, 88)
  m_final = ref_lines(py_m, 90, 90) + ref_lines(py_m, 113, 113) + ref_lines(py_m, 116, 116)
  i_stats, i_file = ref_lines(py_i, 27, 55), ref_lines(py_i, 88, 113)
  i_final = ref_lines(py_i, 115, 116) + ref_lines(py_i, 139, 139)
  assert m_stats.startswith('def iou_stats(') and i_stats.startswith('def iou_stats(')
  assert m_file.startswith('_tp_fn, _tp_fp, _tp = iou_stats(') and m_file.rstrip().endswith('tp += _tp')
  assert 'iou = tp / (tp_fn + tp_fp - tp + 1e-12) * 100.0' in m_final and 'mean_pixel_acc = ' in m_final
  assert 'if i < 255:' in i_file and 'ninst += ninst_' in i_file and 'iou /= ninst+1e-12' in i_final

  def blocky(rng, h, w, cells_y, cells_x, values):
    grid = rng.choice(values, size=(cells_y, cells_x))
    return np.ascontiguousarray(grid[np.arange(h) * cells_y // h][:, np.arange(w) * cells_x // w].astype(np.uint8))

  def triple(rng, nc, kind):
    if kind == 'blocky':
      h, w = 40, 52
      inst = blocky(rng, h, w, 4, 4, np.array([0, 3, 5, 9, 200, 255]))
      inst[:10, :13], inst[10:20, :13], inst[:10, 13:26] = 3, 5, 0
      gt = blocky(rng, h, w, 5, 6, np.arange(nc))
      gt[30:34, 40:46] = nc - 1
      gt[rng.random((h, w)) < 0.1] = 255
      gt[rng.random((h, w)) < 0.03] = nc + 2
      gt[rng.random((h, w)) < 0.02] = nc
      gt[inst == 3] = 255
      five = np.flatnonzero(inst.reshape(-1) == 5)
      a, b = sorted(rng.choice(np.arange(1, nc), size=2, replace=False).tolist())
      flat = gt.reshape(-1)
      flat[five[:five.size // 2]], flat[five[five.size // 2:]] = b, a
      pred = np.where(rng.random((h, w)) < 0.7, np.minimum(gt, nc - 1), rng.integers(0, nc, size=(h, w))).astype(np.uint8)
      for value, share in ((nc, 0.04), (nc + 3, 0.03), (255, 0.03)):
        pred[rng.random((h, w)) < share] = value
      last = np.flatnonzero(gt.reshape(-1) == nc - 1)
      pred.reshape(-1)[last[:3]], pred.reshape(-1)[last[3:6]] = nc, nc - 1     # the class count over the last class: no TP
      counted = gt < nc
      assert last.size >= 6 and five.size % 2 == 0 and (gt[inst == 3] >= nc).all()
      counts5 = np.bincount(gt[inst == 5], minlength=256)
      assert counts5[a] == counts5[b] == counts5[:nc].max() and a < b
      for value in (nc, nc + 3, 255):
        assert (pred[counted] == value).any(), value
      assert ((gt >= nc) & (gt < 255)).any() and (gt == 255).any()
    elif kind == 'all_ids':
      h, w = 24, 32
      inst = rng.permutation(np.arange(h * w) % 256).reshape(h, w).astype(np.uint8)
      gt = rng.integers(0, nc, size=(h, w)).astype(np.uint8)
      gt[rng.random((h, w)) < 0.2] = 255
      pred = rng.integers(0, nc + 2, size=(h, w)).astype(np.uint8)
    elif kind == 'one_id':
      h, w = 17, 23
      inst = np.full((h, w), 7, dtype=np.uint8)
      gt = blocky(rng, h, w, 3, 3, np.arange(nc))
      pred = np.where(rng.random((h, w)) < 0.6, gt, rng.integers(0, 256, size=(h, w))).astype(np.uint8)
    elif kind == 'no_counted':
      h, w = 9, 11
      inst = blocky(rng, h, w, 2, 2, np.array([1, 2, 254]))
      gt = rng.choice(np.array([nc, 254, 255]), size=(h, w)).astype(np.uint8)
      pred = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    else:
      inst, gt, pred = (np.array([[v]], dtype=np.uint8) for v in (255, 3, 3))
    return pred, gt, inst

  store = {}
  for nc, kinds in ((21, ('blocky', 'all_ids', 'one_id', 'one_pixel', 'no_counted')),
                    (15, ('blocky', 'all_ids', 'no_counted', 'one_pixel'))):
    rng = np.random.default_rng(1500 + nc)
    env_m, env_i = {'np': np}, {'np': np}
    exec(compile(m_stats, py_m + ':25-53', 'exec'), env_m)
    exec(compile(i_stats, py_i + ':27-55', 'exec'), env_i)
    env_m.update(args=AttrDict(num_classes=nc), **{k: np.zeros(nc, dtype=np.float64) for k in ('tp_fn', 'tp_fp', 'tp')})
    env_i.update(args=AttrDict(num_classes=nc), iou=np.zeros(nc, dtype=np.float64), ninst=np.zeros(nc, dtype=np.float64))
    for fi, kind in enumerate(kinds):
      pred, gt, inst = triple(rng, nc, kind)
      env_m.update(pred=pred, gt=gt)
      env_i.update(pred=pred, gt=gt, inst=inst)
      exec(compile(m_file, py_m + ':80-88', 'exec'), env_m)
      exec(compile(i_file, py_i + ':88-113', 'exec'), env_i)
      for name in ('_tp_fn', '_tp_fp', '_tp'):
        assert (env_m[name] == env_i[name]).all()
      ninst_ = env_i['ninst_']
      ids = np.unique(inst)
      assert ninst_.sum() == min(ids.size, 255) and (ninst_ == np.round(ninst_)).all()
      if kind == 'all_ids':
        assert ids.size == 256
      if kind == 'no_counted':
        assert env_m['_tp_fn'].sum() == 0 and ninst_[0] == ids.size
      rows = np.stack([env_m['_tp_fn'], env_m['_tp_fp'], env_m['_tp'], ninst_.astype(np.int64)]).astype(np.int64)
      t = 'n%d_f%d_' % (nc, fi)
      store.update({t + 'pred': pred, t + 'gt': gt, t + 'inst': inst, t + 'rows': rows})
    exec(compile(m_final, py_m + ':90,113,116', 'exec'), env_m)
    exec(compile(i_final, py_i + ':115-116,139', 'exec'), env_i)
    assert np.isfinite(env_m['iou']).all() and 0.0 < env_m['mean_iou'] < 100.0 and 0.0 < env_i['mean_iou'] < 100.0
    store.update({'n%d_files' % nc: np.array(len(kinds)), 'n%d_iou' % nc: env_m['iou'],
                  'n%d_mean_iou' % nc: np.array(env_m['mean_iou']), 'n%d_pixel_acc' % nc: np.array(env_m['mean_pixel_acc']),
                  'n%d_inst_iou' % nc: env_i['iou'], 'n%d_inst_mean_iou' % nc: np.array(env_i['mean_iou'])})
    print('n15 score dirs, %d classes: %d files, mIoU %.4f, instance mIoU %.4f'
          % (nc, len(kinds), env_m['mean_iou'], env_i['mean_iou']))
  save(out, 'n15_score_dirs', **store)
  size = os.path.getsize(os.path.join(out, 'n15_score_dirs.npz'))
  assert size <= 100 * 1024, 'n15_score_dirs.npz is %d bytes' % size


def gen_n16(ref, out):
  """N16: the picture of a training summary.  `spml/utils/general/vis.py` is imported with empty stand-ins for
  torchvision (not installed; `make_grid` is not part of the fixture) and, where it is missing, scipy.io; its
  `embedding_to_rgb`, `convert_label_to_color` and `load_color_map`, `common.pca` / `calculate_principal_components`
  / `normalize_embedding` run as they stand on the CPU in fp32, and lines 23-29 of `write_image_to_tensorboard` (the
  nearest resize of the panels and their concatenation) are exec'd from the file.  The floats before `.byte()`
  (vis.py:95) are taken by exec'ing :74-94 of the same function next to the whole call.  Two cases: N = 2, C = 64, a
  9 x 11 embedding with 33 x 41 labels; N = 1, C = 32, 8 x 8 with 8 x 8 labels.  The embeddings are `coherent_embedding`
  with graded blob strengths; a seed is taken only if the four leading eigenvalues of the covariance of the normalised
  pixels are separated by a factor of at least 1.5 each (a degenerate pair would make the components arbitrary)."""
  import linecache
  import textwrap
  import torch.nn.functional as F
  stand_ins = {'torchvision': types.ModuleType('torchvision'), 'torchvision.utils': types.ModuleType('torchvision.utils')}
  stand_ins['torchvision'].utils = stand_ins['torchvision.utils']
  try:
    import scipy.io                                        # noqa: F401
  except ImportError:
    stand_ins.update({'scipy': types.ModuleType('scipy'), 'scipy.io': types.ModuleType('scipy.io')})
    stand_ins['scipy'].io = stand_ins['scipy.io']
  had = {name: sys.modules.get(name) for name in stand_ins}
  sys.modules.pop('spml.utils.general.vis', None)          # (n14 may have imported it with its own stand-ins)
  sys.modules.update(stand_ins)
  try:
    import spml.utils.general.vis as vis
    import spml.utils.general.common as common
  finally:
    for name, module in had.items():
      if module is None:
        del sys.modules[name]
      else:
        sys.modules[name] = module
  vis_py = os.path.join(ref, 'spml', 'utils', 'general', 'vis.py')

  def ref_lines(first, last):
    return textwrap.dedent(''.join(linecache.getline(vis_py, i) for i in range(first, last + 1)))
  floats_src, panels_src = ref_lines(74, 94), ref_lines(23, 29)
  assert floats_src.startswith('embeddings = embeddings.permute(0, 2, 3, 1)') and floats_src.rstrip().endswith('rgb *= 255')
  assert panels_src.startswith('for ind, image in enumerate(images):') and panels_src.rstrip().endswith('images = torch.cat(images, dim=3)')
  assert "mode='nearest'" in panels_src
  table = vis.load_color_map(os.path.join(ref, 'misc', 'colormapvoc.mat'))
  assert table.shape == (256, 3) and table.dtype == torch.uint8

  store = {'color_map': table.numpy()}
  cases = [(2, 64, 9, 11, 33, 41, (3.0, 2.2, 1.6, 1.2, 0.8)), (1, 32, 8, 8, 8, 8, (3.0, 2.2, 1.6, 1.2, 0.8))]
  for ci, (n, c, h, w, hl, wl, strengths) in enumerate(cases):
    for seed in range(1600 + 100 * ci, 1700 + 100 * ci):
      gen = torch.Generator().manual_seed(seed)
      emb = coherent_embedding(gen, n, c, h, w, blobs=5, noise=0.15, strengths=strengths)
      rows = common.normalize_embedding(emb.permute(0, 2, 3, 1).contiguous()).view(-1, c).double()
      rows = rows - rows.mean(0, keepdim=True)
      lam = torch.linalg.eigvalsh(rows.t() @ rows).flip(0)[:4]
      if bool((lam[:-1] >= 1.5 * lam[1:]).all()):
        break
    else:
      raise AssertionError('case %d: no seed separates the four leading eigenvalues by 1.5' % ci)
    sem = blocky_labels(gen, n, hl, wl, 4, 0, 21)
    sem[torch.rand(n, hl, wl, generator=gen) < 0.05] = 255
    ins = blocky_labels(gen, n, hl, wl, 5, 0, 12)
    # the whole function, and its lines up to `.byte()` for the floats
    rgb = vis.embedding_to_rgb(emb.clone(), 'pca')
    env = {'embeddings': emb.clone(), 'common_utils': common, 'torch': torch, 'project_type': 'pca'}
    exec(compile(floats_src, vis_py + ':74-94', 'exec'), env)
    floats = env['rgb'].clone()                            # [N, H W, 3], 0 .. 255
    assert torch.equal(floats.byte().view(n, h, w, 3).permute(0, 3, 1, 2), rgb)
    normed = common.normalize_embedding(emb.permute(0, 2, 3, 1).contiguous())
    basis = common.calculate_principal_components(normed.view(-1, c), 3)
    assert torch.equal(common.pca(normed, 3), torch.mm(normed.view(-1, c), basis).view(n, h, w, 3))
    env = {'images': [vis.convert_label_to_color(sem, table), vis.convert_label_to_color(ins, table), rgb],
           'size': (h, w), 'F': F, 'torch': torch}
    exec(compile(panels_src, vis_py + ':23-29', 'exec'), env)
    panels = env['images']
    assert panels.shape == (n, 3, h, 3 * w) and panels.dtype == torch.uint8
    t = 'c%d_' % ci
    store.update({t + 'embedding': emb, t + 'semantic': sem.to(torch.uint8), t + 'instance': ins.to(torch.uint8),
                  t + 'basis': basis, t + 'floats': floats.view(n, h, w, 3), t + 'bytes': rgb, t + 'panels': panels,
                  t + 'eigenvalues': lam, t + 'seed': np.array(seed)})
    print('n16 case %d: seed %d, leading eigenvalues %s' % (ci, seed, ['%.4f' % v for v in lam.tolist()]))
  save(out, 'n16_train_summary', **store)
  size = os.path.getsize(os.path.join(out, 'n16_train_summary.npz'))
  assert size <= 100 * 1024, 'n16_train_summary.npz is %d bytes' % size


class AttrDict(dict):
  __getattr__ = dict.__getitem__


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--ref', default='/root/reference')
  ap.add_argument('--out', default=os.path.join(
      os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
  ap.add_argument('--only', default=None, help='comma separated fixture names')
  args = ap.parse_args()
  global ONLY
  ONLY = set(args.only.split(',')) if args.only else None
  out = os.path.abspath(args.out)
  os.makedirs(out, exist_ok=True)

  sys.path.insert(0, args.ref)
  torch.set_num_threads(1)       # bit-stable fp32 sums
  if ONLY is not None and ONLY <= {'n7_pseudo_labels', 'n8_softmax_msc', 'n9_knn_msc', 'n10_prototype_msc',
                                   'n11_pseudo_knn_msc', 'n11_instance_iou', 'n12_densepose_pseudo',
                                   'n13_augment', 'n14_inference_io', 'n15_score_dirs', 'n16_train_summary'}:      # (need none of the imports and shims below)
    if 'n7_pseudo_labels' in ONLY:
      gen_n7(args.ref, out)
    if 'n8_softmax_msc' in ONLY:
      gen_n8(args.ref, out)
    if 'n9_knn_msc' in ONLY:
      gen_n9(args.ref, out)
    if 'n10_prototype_msc' in ONLY:
      gen_n10(args.ref, out)
    if 'n11_pseudo_knn_msc' in ONLY:
      gen_n11(args.ref, out)
    if 'n11_instance_iou' in ONLY:
      gen_n11_instance(args.ref, out)
    if 'n12_densepose_pseudo' in ONLY:
      gen_n12(args.ref, out)
    if 'n13_augment' in ONLY:
      gen_n13(args.ref, out)
    if 'n14_inference_io' in ONLY:
      gen_n14(args.ref, out)
    if 'n15_score_dirs' in ONLY:
      gen_n15(args.ref, out)
    if 'n16_train_summary' in ONLY:
      gen_n16(args.ref, out)
    return

  import spml.utils.general.common as g_common
  import spml.utils.segsort.common as s_common
  import spml.utils.segsort.loss as s_loss
  import spml.utils.segsort.eval as s_eval
  import spml.models.utils as m_utils
  import spml.utils.general.train as g_train
  import spml.models.predictions.segsort as p_segsort

  # --- shim 1: device.index is None on CPU (common.py:376) ------------------
  src = inspect.getsource(s_common.segment_by_kmeans)
  assert 'cur_cluster_indices.device.index' in src
  src = src.replace('cur_cluster_indices.device.index',
                    '(cur_cluster_indices.device.index or GPU_ID)')
  ns = dict(s_common.__dict__)
  ns['GPU_ID'] = 0
  exec(compile(src, '<segment_by_kmeans+cpu-shim>', 'exec'), ns)
  ref_segment_by_kmeans = ns['segment_by_kmeans']

  def segment_by_kmeans_rank(gpu_id, *a, **kw):
    ns['GPU_ID'] = gpu_id
    try:
      return ref_segment_by_kmeans(*a, **kw)
    finally:
      ns['GPU_ID'] = 0

  # --- shim 2: scatter_gather.gather asserts on CPU --------------------------
  m_utils.scatter_gather = types.SimpleNamespace(
      gather=lambda xs, dev: torch.cat(list(xs), 0))

  # ======================= A1 / A2 / A3 / A13 ================================
  g = torch.Generator().manual_seed(235)
  x = torch.randn(7, 5, 19, generator=g)
  x[0, 0] = 0.0                     # zero row -> eps branch
  x[1, 2] *= 1e-14                  # tiny norm < eps
  save(out, 'a01_normalize', x=x, y=g_common.normalize_embedding(x))

  grids = {}
  for tag, (k, hw) in {'k3_17': ((3, 3), (17, 17)), 'k6_130': ((6, 6), (130, 130)),
                       'k6_128': ((6, 6), (128, 128)), 'k12_194': ((12, 12), (194, 194)),
                       'k32_258': ((32, 32), (258, 258)), 'k6_513': ((6, 6), (513, 513)),
                       'k4x5_33x29': ((4, 5), (33, 29)), 'k12_512': ((12, 12), (512, 512)),
                       'k2_3': ((2, 2), (3, 3))}.items():
    grids['init_' + tag] = s_common.initialize_cluster_labels(k, hw, 'cpu')
    grids['argk_' + tag] = np.array(k)
  save(out, 'a03_init_grid', **grids)

  locs = {}
  for tag, hw in {'17x17': (17, 17), '33x29': (33, 29), '130x130': (130, 130)}.items():
    locs['float_' + tag] = s_common.generate_location_features(hw, 'cpu', 'float')
    locs['int_' + tag] = s_common.generate_location_features(hw, 'cpu', 'int')
  save(out, 'a02_location', **locs)

  lab = torch.randint(0, 9, (2, 11, 13), generator=g)
  save(out, 'a13_onehot_resize', lab=lab, onehot=g_common.one_hot(lab),
       onehot12=g_common.one_hot(lab, 12),
       big=blocky_labels(g, 2, 65, 65, 5, 0, 255),
       **{'resized_%d' % s: g_common.resize_labels(
           blocky_labels(torch.Generator().manual_seed(7), 2, 65, 65, 5, 0, 255), (s, s))
          for s in (17, 33, 130)})
  save(out, 'a13_resize_src',
       src=blocky_labels(torch.Generator().manual_seed(7), 2, 65, 65, 5, 0, 255))

  # ======================= A4 / A5 / A6 ======================================
  for tag, (p, d, k, it) in {'tiny': (289, 10, 9, 10), 'small': (1089, 66, 36, 10),
                             'k144': (2000, 34, 144, 6)}.items():
    g = torch.Generator().manual_seed(1000 + p)
    side = int(round(p ** 0.5))
    if side * side == p:
      emb = coherent_embedding(g, 1, d, side, side)[0].permute(1, 2, 0).reshape(p, d)
    else:
      emb = torch.randn(p, d, generator=g)
    emb = g_common.normalize_embedding(emb)
    init = torch.randint(0, k, (p,), generator=g)
    init[:k] = torch.arange(k)
    if tag == 'tiny':
      init[init == 4] = 3           # cluster 4 starts empty -> zero prototype
    protos0 = s_common.calculate_prototypes_from_labels(emb, init, k)
    near0 = s_common.find_nearest_prototypes(emb, protos0)
    labels = init
    per_iter, per_proto, per_margin = [], [], []
    for _ in range(it):
      pr = s_common.calculate_prototypes_from_labels(emb, labels, k)
      sims = torch.mm(emb, pr.t())
      labels = s_common.find_nearest_prototypes(emb, pr)
      t2 = torch.topk(sims, 2, dim=1).values
      per_iter.append(labels)
      per_proto.append(pr)
      per_margin.append(t2[:, 0] - t2[:, 1])
    final = s_common.kmeans_with_initial_labels(emb, init, k, it)
    assert torch.equal(final, labels)
    save(out, 'a06_kmeans_' + tag, emb=emb, init=init, k=np.array(k),
         iterations=np.array(it), protos0=protos0, nearest0=near0,
         labels_per_iter=torch.stack(per_iter), protos_per_iter=torch.stack(per_proto),
         margin_per_iter=torch.stack(per_margin), final=final)

  # ======================= A7 / A14 ==========================================
  sem = torch.tensor([3, 3, 5, 5, 3, 7])
  ins = torch.tensor([0, 0, 0, 1, 1, 1])
  pl, inv = s_common.prepare_prototype_labels(sem, ins, 8)
  g = torch.Generator().manual_seed(77)
  sem2 = torch.randint(0, 21, (500,), generator=g)
  ins2 = torch.randint(0, 40, (500,), generator=g)
  pl2, inv2 = s_common.prepare_prototype_labels(sem2, ins2, 21)
  sel, major = s_common.find_majority_label_index(sem2, ins2)
  save(out, 'a07_labels', sem=sem, ins=ins, off=np.array(8), plab=pl, inv=inv,
       sem2=sem2, ins2=ins2, off2=np.array(21), plab2=pl2, inv2=inv2,
       major_sel=sel, major_lab=major)

  # ======================= A8 segment_by_kmeans ==============================
  for tag, (n, c, h, w, k, div, gpu) in {
      'tiny': (2, 8, 17, 17, (3, 3), 256, 0),
      'small': (2, 32, 29, 29, (6, 6), 2048, 0),
      'rank1': (2, 16, 21, 25, (4, 3), 2048, 1)}.items():
    g = torch.Generator().manual_seed(4000 + c)
    emb = coherent_embedding(g, n, c, h, w)
    sem = blocky_labels(g, n, h, w, 3, 0, 21)
    # unlabelled (254) outside a few blobs, ignore strip (255) bottom/right
    keep = blocky_labels(g, n, h, w, 6, 0, 4) == 0
    sem = torch.where(keep, sem, torch.full_like(sem, 254))
    sem[:, -2:, :] = 255
    sem[:, :, -3:] = 255
    ins = blocky_labels(g, n, h, w, 4, 0, 200)
    labels = sem * div + ins
    ignore = int(labels.max()) + 1
    labels = labels.masked_fill(sem == 255, ignore)
    loc = (s_common.generate_location_features((h, w), 'cpu', 'float') - 0.5
           ).unsqueeze(0).expand(n, h, w, 2)
    o = segment_by_kmeans_rank(gpu, emb, labels, list(k), local_features=loc,
                               ignore_index=ignore, iterations=10)
    o2 = segment_by_kmeans_rank(gpu, emb, None, list(k), iterations=3)
    save(out, 'a08_segment_' + tag, emb=emb, labels=labels, sem=sem, ins=ins,
         k=np.array(k), ignore=np.array(ignore), gpu=np.array(gpu), loc=loc,
         div=np.array(div),
         o_emb=o[0], o_embloc=o[1], o_lab=o[2], o_clu=o[3], o_bat=o[4],
         d_emb=o2[0], d_embloc=o2[1], d_lab=o2[2], d_clu=o2[3], d_bat=o2[4])

  # ======================= A9 / A10 losses (fwd + grads) =====================
  for tag, (p, m, d, ncls, kappa) in {'tiny': (200, 23, 10, 5, 6.0),
                                      'small': (700, 150, 64, 21, 12.0),
                                      'loc': (400, 60, 66, 21, 16.0)}.items():
    g = torch.Generator().manual_seed(9000 + p)
    protos = g_common.normalize_embedding(torch.randn(m, d, generator=g))
    own = torch.randint(0, m, (p,), generator=g)
    emb = g_common.normalize_embedding(
        protos[own] + 0.7 * torch.randn(p, d, generator=g))
    p_sem = torch.randint(0, ncls, (m,), generator=g)
    sem = p_sem[own].clone()
    flip = torch.rand(p, generator=g) < 0.1
    sem[flip] = torch.randint(0, ncls, (int(flip.sum()),), generator=g)
    # make one class have a single prototype -> 'pos <= 0' fallback branch
    p_sem[0] = ncls + 3
    sem[own == 0] = ncls + 3
    emb_r = emb.clone().requires_grad_(True)
    pro_r = protos.clone().requires_grad_(True)
    nll = s_loss._calculate_log_likelihood(emb_r, sem, own, pro_r, p_sem, kappa,
                                           'segsort+')
    loss = s_loss.SegSortLoss(kappa, 'segsort+', reduction='mean')(
        emb_r, sem, own, pro_r, p_sem)
    loss.backward()
    # tag sets
    p_tags = (torch.rand(m, ncls - 1, generator=g) < 0.15).long()
    p_tags[torch.arange(m), torch.randint(0, ncls - 1, (m,), generator=g)] = 1
    p_tags[1] = 0                                  # a prototype with no tag
    tags = p_tags[own].clone()
    tflip = torch.rand(p, generator=g) < 0.1
    tags[tflip] = (torch.rand(int(tflip.sum()), ncls - 1, generator=g) < 0.1).long()
    emb_s = emb.clone().requires_grad_(True)
    pro_s = protos.clone().requires_grad_(True)
    snll = s_loss._one_hot_calculate_log_likelihood(emb_s, tags, own, pro_s, p_tags,
                                                    kappa, 'segsort+')
    sloss = s_loss.SetSegSortLoss(kappa, 'segsort+', reduction='mean')(
        emb_s, tags, own, pro_s, p_tags)
    sloss.backward()
    save(out, 'a09_loss_' + tag, emb=emb, protos=protos, own=own, sem=sem,
         p_sem=p_sem, kappa=np.array(kappa), nll=nll, loss=loss,
         d_emb=emb_r.grad, d_protos=pro_r.grad,
         tags=tags, p_tags=p_tags, set_nll=snll, set_loss=sloss,
         set_d_emb=emb_s.grad, set_d_protos=pro_s.grad)

  # ======================= A11 / A12 =========================================
  g = torch.Generator().manual_seed(1111)
  q = g_common.normalize_embedding(torch.randn(150, 32, generator=g))
  pr = g_common.normalize_embedding(torch.randn(400, 32, generator=g))
  ql = torch.randint(0, 21, (150,), generator=g)
  prl = torch.randint(0, 21, (400,), generator=g)
  acc5, top5 = s_eval.top_k_ranking(q, ql, pr, prl, 5)
  acc20, top20 = s_eval.top_k_ranking(q, ql, pr, prl, 20)
  accs, tops = s_eval.top_k_ranking(pr, prl, pr, prl, 5)
  save(out, 'a11_topk', q=q, ql=ql, pr=pr, prl=prl, acc5=acc5, top5=top5,
       acc20=acc20, top20=top20, acc_self=accs, top_self=tops,
       major20=s_eval.majority_label_from_topk(top20),
       major20_21=s_eval.majority_label_from_topk(top20, 21))

  # ======================= B1 (2 shards) + B3 ================================
  shards = []
  for gpu in (0, 1):
    g = torch.Generator().manual_seed(500 + gpu)
    n, c, h, w, k, div = 2, 16, 19, 23, (3, 3), 2048
    emb = coherent_embedding(g, n, c, h, w)
    sem = blocky_labels(g, n, h, w, 3, 0, 21)
    keep = blocky_labels(g, n, h, w, 5, 0, 3) == 0
    sem = torch.where(keep, sem, torch.full_like(sem, 254))
    sem[:, -2:, :] = 255
    ins = blocky_labels(g, n, h, w, 4, 0, 50)
    labels = (sem * div + ins)
    ignore = int(labels.max()) + 1
    labels = labels.masked_fill(sem == 255, ignore)
    o = segment_by_kmeans_rank(gpu, emb, labels, list(k), ignore_index=ignore,
                               iterations=5)
    shards.append(dict(emb=o[0], embloc=o[1], sem=o[2] // div, ins=o[2] % div,
                       clu=o[3], bat=o[4], raw_emb=emb, raw_labels=labels,
                       ignore=ignore))
  embs = [s['emb'].clone().requires_grad_(True) for s in shards]
  emls = [s['embloc'].clone().requires_grad_(True) for s in shards]
  res = m_utils.gather_clustering_and_update_prototypes(
      embs, emls, [s['clu'] for s in shards], [s['bat'] for s in shards],
      [s['sem'] for s in shards], [s['ins'] for s in shards], 'cpu')
  protos, protos_loc, p_sem, p_ins, p_bat, new_clu = res
  wgt = torch.randn(protos[0].shape, generator=g)
  wgt2 = torch.randn(protos_loc[0].shape, generator=g)
  ((protos[0] * wgt).sum() + (protos_loc[0] * wgt2).sum()).backward()
  b1 = {}
  for i, s in enumerate(shards):
    for kname in ('emb', 'embloc', 'sem', 'ins', 'clu', 'bat', 'raw_emb', 'raw_labels'):
      b1['s%d_%s' % (i, kname)] = s[kname]
    b1['s%d_ignore' % i] = np.array(s['ignore'])
    b1['s%d_new_clu' % i] = new_clu[i]
    b1['s%d_d_emb' % i] = embs[i].grad
    b1['s%d_d_embloc' % i] = emls[i].grad
  save(out, 'b01_gather', protos=protos[0], protos_loc=protos_loc[0], p_sem=p_sem[0],
       p_ins=p_ins[0], p_bat=p_bat[0], wgt=wgt, wgt2=wgt2, **b1)

  all_emb = torch.cat([s['emb'] for s in shards])
  all_bat = torch.cat([s['bat'] for s in shards])
  ms = m_utils.gather_multiset_labels_per_batch_by_nearest_neighbor(
      all_emb, protos[0].detach(), p_sem[0], all_bat, p_bat[0],
      num_classes=21, top_k=3, threshold=0.6)
  save(out, 'b03_multiset', emb=all_emb, bat=all_bat, protos=protos[0], p_sem=p_sem[0],
       p_bat=p_bat[0], out=ms, threshold=np.array(0.6))

  # ======================= F1-F3: Segsort.losses, with memory bank ===========
  cfg = AttrDict(
      train=AttrDict(sem_ann_loss_types='segsort', sem_occ_loss_types='segsort',
                     img_sim_loss_types='segsort', feat_aff_loss_types='none',
                     sem_ann_concentration=6.0, sem_occ_concentration=12.0,
                     img_sim_concentration=16.0, feat_aff_concentration=0.0,
                     sem_ann_loss_weight=1.0, sem_occ_loss_weight=0.5,
                     img_sim_loss_weight=0.1, feat_aff_loss_weight=0.0),
      dataset=AttrDict(semantic_ignore_index=255, num_classes=21),
      network=AttrDict(label_divisor=2048))
  model = p_segsort.Segsort(cfg)
  s = shards[0]
  one = m_utils.gather_clustering_and_update_prototypes(
      [s['emb']], [s['embloc']], [s['clu']], [s['bat']], [s['sem']], [s['ins']], 'cpu')
  sem_tag = torch.zeros(2, 256, dtype=torch.long)
  for b in range(2):
    present = torch.unique(s['sem'][s['bat'] == b])
    sem_tag[b, present] = 1
  emb_r = s['emb'].clone().requires_grad_(True)
  eml_r = s['embloc'].clone().requires_grad_(True)
  datas = {'cluster_index': one[5][0], 'cluster_embedding': emb_r,
           'cluster_embedding_with_loc': eml_r,
           'cluster_semantic_label': s['sem'], 'cluster_instance_label': s['ins'],
           'cluster_batch_index': s['bat']}
  # memory bank made from shard 1's prototypes (detached), batch index shifted
  s1 = shards[1]
  mem = m_utils.gather_clustering_and_update_prototypes(
      [s1['emb']], [s1['embloc']], [s1['clu']], [s1['bat']], [s1['sem']], [s1['ins']], 'cpu')
  mem_tag = torch.zeros(4, 256, dtype=torch.long)
  for b in (2, 3):
    present = torch.unique(s1['sem'][s1['bat'] == b])
    mem_tag[b, present] = 1
  targets = {'prototype': one[0][0].detach(), 'prototype_semantic_label': one[2][0],
             'prototype_batch_index': one[4][0], 'semantic_tag': sem_tag,
             'prototype_semantic_tag': sem_tag[one[4][0]],
             'memory_prototype': [mem[0][0].detach()],
             'memory_prototype_semantic_label': [mem[2][0]],
             'memory_prototype_batch_index': [mem[4][0]],
             'memory_prototype_semantic_tag': [mem_tag[mem[4][0]]]}
  l_ann, l_occ, l_img, acc = model.losses(datas, targets)
  (l_ann + l_occ + l_img).backward()
  targets_nomem = {k: v for k, v in targets.items() if not k.startswith('memory')}
  n_ann, n_occ, n_img, n_acc = model.losses(
      {k: (v.detach() if v.is_floating_point() else v) for k, v in datas.items()},
      targets_nomem)
  save(out, 'f01_segsort_losses',
       clu=one[5][0], emb=s['emb'], embloc=s['embloc'], sem=s['sem'], ins=s['ins'],
       bat=s['bat'], protos=one[0][0], p_sem=one[2][0], p_bat=one[4][0],
       sem_tag=sem_tag, mem_protos=mem[0][0], mem_p_sem=mem[2][0], mem_p_bat=mem[4][0],
       mem_tag=mem_tag[mem[4][0]],
       l_ann=l_ann, l_occ=l_occ, l_img=l_img, acc=acc,
       d_emb=emb_r.grad, d_embloc=eml_r.grad,
       n_ann=n_ann, n_occ=n_occ, n_img=n_img, n_acc=n_acc)

  # ======================= N1: kNN predictions + memory-bank files ============
  # Segsort.predictions (segsort.py:68-125): prototypes of the (gappy) cluster ids,
  # 20-NN retrieval in the memory bank in 10 groups, majority vote, scatter to pixels.
  import spml.utils.segsort.others as s_others
  gappy = one[5][0] * 3 + 1                       # ids with holes: exercises the unique()
  bank = torch.cat([mem[0][0], one[0][0]], 0).detach()
  bank_lab = torch.cat([mem[2][0], one[2][0]], 0)
  assert bank.shape[0] >= 20
  pred, topk = model.predictions(
      {'cluster_embedding': s['emb'], 'cluster_index': gappy},
      {'semantic_memory_prototype': bank, 'semantic_memory_prototype_label': bank_lab})
  # the on-disk memory bank of prototype.py:207-211 read back by others.py:11-41
  bank_dir = os.path.join(out, 'n1_memory_bank')
  os.makedirs(bank_dir, exist_ok=True)
  half = bank.shape[0] // 2
  if ONLY is None or 'n1_predictions' in ONLY or not os.path.exists(os.path.join(bank_dir, '2007_000032.npy')):
    np.save(os.path.join(bank_dir, '2007_000032.npy'),
            {'prototype': bank[:half].numpy(), 'prototype_label': bank_lab[:half].numpy()})
    np.save(os.path.join(bank_dir, '2007_000039.npy'),
            {'prototype': bank[half:].numpy(), 'prototype_label': bank_lab[half:].numpy()})
  loaded, loaded_lab = s_others.load_memory_banks(bank_dir)
  save(out, 'n1_predictions', emb=s['emb'], clu=gappy, bank=bank, bank_lab=bank_lab,
       pred=pred, topk=topk, loaded=loaded, loaded_lab=loaded_lab)

  # ======================= N4: DensePose embedding variant + predictor ========
  # resnet_pspnet_densepose.py: 5-channel local features (location + smoothed, normalised
  # colour), k-means on C+5 channels, embedding-with-local rebuilt from 0.1 * embedding;
  # segsort_softmax_densepose.py: tags propagated from the nearest labelled segment.
  import spml.models.embeddings.resnet_pspnet_densepose as e_dp
  import spml.models.predictions.segsort_softmax_densepose as p_dp
  cfg_dp = AttrDict(
      train=AttrDict(sem_ann_loss_types='segsort', sem_occ_loss_types='segsort',
                     img_sim_loss_types='segsort', feat_aff_loss_types='none',
                     sem_ann_concentration=6.0, sem_occ_concentration=12.0,
                     img_sim_concentration=16.0, feat_aff_concentration=0.0,
                     sem_ann_loss_weight=1.0, sem_occ_loss_weight=0.5,
                     img_sim_loss_weight=0.1, feat_aff_loss_weight=0.0),
      dataset=AttrDict(semantic_ignore_index=255, num_classes=15),
      network=AttrDict(label_divisor=2048, embedding_dim=16, kmeans_num_clusters=[3, 3],
                       kmeans_iterations=5, use_syncbn=False, backbone_types='panoptic_pspnet_101'))
  g = torch.Generator().manual_seed(77)
  torch.manual_seed(77)
  net = e_dp.ResnetPspnet([1, 1, 1, 1], [1, 2, 1, 1], [1, 1, 2, 4], cfg_dp).eval()
  n, c, h, w = 2, 16, 22, 18
  image = torch.nn.functional.interpolate(torch.randn(n, 3, 12, 10, generator=g), size=(88, 72),
                                          mode='bilinear', align_corners=False)
  image = image + 0.1 * torch.randn(n, 3, 88, 72, generator=g)
  dp_emb = coherent_embedding(g, n, c, h, w)
  dp_sem = blocky_labels(g, n, h, w, 3, 0, 15)
  dp_sem = torch.where(blocky_labels(g, n, h, w, 5, 0, 3) == 0, dp_sem, torch.full_like(dp_sem, 254))
  dp_sem[:, :, -3:] = 255
  dp_ins = blocky_labels(g, n, h, w, 4, 0, 40)
  with torch.no_grad():
    dp_local = net.lfn(image, size=(h, w))
  assert dp_local.shape[-1] == 5
  orig_sbk = e_dp.segsort_common.segment_by_kmeans
  e_dp.segsort_common.segment_by_kmeans = ref_segment_by_kmeans
  try:
    dp_out = net.generate_clusters(dp_emb, dp_sem, dp_ins, dp_local)
  finally:
    e_dp.segsort_common.segment_by_kmeans = orig_sbk

  pred_dp = p_dp.SegsortSoftmax(cfg_dp).eval()
  s0 = shards[0]
  dp_nc = 15
  sem15 = torch.where(s0['sem'] < 21, s0['sem'] % dp_nc, s0['sem'])     # classes of this recipe
  p_sem15 = torch.where(one[2][0] < 21, one[2][0] % dp_nc, one[2][0])
  m_sem15 = torch.where(mem[2][0] < 21, mem[2][0] % dp_nc, mem[2][0])
  emb_r = s0['emb'].clone().requires_grad_(True)
  fmap = torch.randn(2, 16, 11, 13, generator=g)
  flab = blocky_labels(g, 2, 40, 44, 3, 0, 17)
  flab[:, :4] = 255
  datas_dp = {'cluster_index': one[5][0], 'cluster_embedding': emb_r,
              'cluster_embedding_with_loc': s0['embloc'],
              'cluster_semantic_label': sem15, 'cluster_instance_label': s0['ins'],
              'cluster_batch_index': s0['bat'], 'embedding': fmap}
  targets_dp = {'prototype': one[0][0].detach(), 'prototype_with_loc': one[1][0].detach(),
                'prototype_semantic_label': p_sem15, 'prototype_batch_index': one[4][0],
                'semantic_label': flab.clone(),
                'memory_prototype': [mem[0][0].detach()],
                'memory_prototype_with_loc': [mem[1][0].detach()],
                'memory_prototype_semantic_label': [m_sem15],
                'memory_prototype_batch_index': [mem[4][0]]}
  dl_ann, dl_occ, dl_img, dl_acc = pred_dp.losses(datas_dp, targets_dp)
  (dl_ann + dl_occ + dl_img).backward()
  all_loc = torch.cat([one[1][0], mem[1][0]], 0).detach()
  all_sem = torch.cat([p_sem15, m_sem15], 0)
  all_bat = torch.cat([one[4][0], mem[4][0]], 0)
  prop_tags = m_utils.gather_multiset_labels_per_batch_by_nearest_neighbor(
      all_loc, all_loc, all_sem, all_bat, all_bat, num_classes=dp_nc, top_k=1, threshold=0.95,
      label_divisor=2048)
  save(out, 'n4_densepose',
       image=image, emb_map=dp_emb, sem_map=dp_sem, ins_map=dp_ins, local=dp_local,
       o_emb=dp_out['cluster_embedding'], o_embloc=dp_out['cluster_embedding_with_loc'],
       o_sem=dp_out['cluster_semantic_label'], o_ins=dp_out['cluster_instance_label'],
       o_clu=dp_out['cluster_index'], o_bat=dp_out['cluster_batch_index'],
       cls_w0=pred_dp.semantic_classifier[0].weight, cls_bn_w=pred_dp.semantic_classifier[1].weight,
       cls_bn_b=pred_dp.semantic_classifier[1].bias, cls_w4=pred_dp.semantic_classifier[4].weight,
       cls_b4=pred_dp.semantic_classifier[4].bias,
       clu=one[5][0], emb=s0['emb'], embloc=s0['embloc'], sem=sem15, ins=s0['ins'], bat=s0['bat'],
       fmap=fmap, flab=flab, protos=one[0][0], protos_loc=one[1][0], p_sem=p_sem15, p_bat=one[4][0],
       mem_protos=mem[0][0], mem_protos_loc=mem[1][0], mem_p_sem=m_sem15, mem_p_bat=mem[4][0],
       l_ann=dl_ann, l_occ=dl_occ, l_img=dl_img, acc=dl_acc, d_emb=emb_r.grad, prop_tags=prop_tags)

  # ======================= H1: two training steps of the reference ===========
  # pyscripts/train/train.py:154-309 on ONE device with the reference's own model classes
  # (ResnetDeeplab + SegsortSoftmax -- train.py:31 binds `segsort` to the softmax variant)
  # and lib.nn.optimizer.SGD: embeddings + k-means, prototypes, tags, memory bank, losses,
  # poly lr, SGD.step(lr), memory-bank FIFO with the batch-index shift.  Step 1 runs with
  # the memory bank filled by step 0.  Weights: tests/tools_synth.reinit_parameters (the
  # same function re-creates them in the tests), inputs: spml_amd.synth.make_batch.
  import spml.models.embeddings.resnet_deeplab as e_dl
  import spml.models.predictions.segsort_softmax as p_soft
  import lib.nn.optimizer as ref_opt
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
  from tools_synth import reinit_parameters, parameter_checksums
  from spml_amd import synth
  cfg_h1 = AttrDict(
      train=AttrDict(sem_ann_loss_types='segsort', sem_occ_loss_types='segsort',
                     img_sim_loss_types='segsort', feat_aff_loss_types='none',
                     sem_ann_concentration=6.0, sem_occ_concentration=12.0,
                     img_sim_concentration=16.0, feat_aff_concentration=0.0,
                     sem_ann_loss_weight=1.0, sem_occ_loss_weight=0.5,
                     img_sim_loss_weight=0.1, feat_aff_loss_weight=0.0,
                     base_lr=3e-3, max_iteration=30000, warmup_iteration=100, momentum=0.9,
                     weight_decay=5e-4, batch_size=2, memory_bank_size=2),
      dataset=AttrDict(semantic_ignore_index=255, num_classes=21),
      network=AttrDict(label_divisor=2048, embedding_dim=16, kmeans_num_clusters=[4, 4],
                       kmeans_iterations=5, use_syncbn=False,
                       backbone_types='panoptic_deeplab_101'))
  def run_h1(dropout):
    """dropout=True: the head's nn.Dropout(0.75) draws from torch's global CPU generator,
    re-seeded at the start of every step (the oracle test does the same); False: p = 0 on the
    reference module instance -- the variant the GPU path is compared with (its dropout
    mask comes from another generator)."""
    h_emb = reinit_parameters(e_dl.ResnetDeeplab([1, 1, 1, 1], [1, 2, 1, 1], [1, 1, 2, 4], cfg_h1), 31)
    h_pred = reinit_parameters(p_soft.SegsortSoftmax(cfg_h1), 32)
    h_emb.train(); h_pred.train()
    if not dropout:
      h_pred.semantic_classifier[3].p = 0.0
    h_opt = ref_opt.SGD(h_emb.get_params_lr() + h_pred.get_params_lr(), lr=1,
                        momentum=cfg_h1.train.momentum, weight_decay=cfg_h1.train.weight_decay)
    h_opt.zero_grad()
    orig_sbk = e_dl.segsort_common.segment_by_kmeans
    e_dl.segsort_common.segment_by_kmeans = ref_segment_by_kmeans
    h_store = {}
    memory_banks = {}
    num_gpus, h_iter0 = 1, 57          # inside the warm-up ramp of lr_poly
    try:
      for step in range(2):
        torch.manual_seed(4000 + step)
        datas, targets = synth.make_batch(2, 161, seed=900 + step)
        image_batch, label_batch = [datas], [dict(targets)]
        embeddings = [h_emb(image_batch[0], label_batch[0])]
        embeddings[0]['embedding'].retain_grad()
        seg_ids = embeddings[0]['cluster_index'].clone()     # as segment_by_kmeans returned them
        (prototypes, prototypes_with_loc, prototype_semantic_labels, prototype_instance_labels,
         prototype_batch_indices, cluster_indices) = m_utils.gather_clustering_and_update_prototypes(
             [e['cluster_embedding'] for e in embeddings],
             [e['cluster_embedding_with_loc'] for e in embeddings],
             [e['cluster_index'] for e in embeddings], [e['cluster_batch_index'] for e in embeddings],
             [e['cluster_semantic_label'] for e in embeddings],
             [e['cluster_instance_label'] for e in embeddings], 'cpu')
        label_batch[0]['prototype'] = prototypes[0]
        label_batch[0]['prototype_with_loc'] = prototypes_with_loc[0]
        label_batch[0]['prototype_semantic_label'] = prototype_semantic_labels[0]
        label_batch[0]['prototype_instance_label'] = prototype_instance_labels[0]
        label_batch[0]['prototype_batch_index'] = prototype_batch_indices[0]
        embeddings[0]['cluster_index'] = cluster_indices[0]
        semantic_tags = m_utils.gather_and_update_datas([label_batch[0]['semantic_tag']], 'cpu')
        label_batch[0]['semantic_tag'] = semantic_tags[0]
        label_batch[0]['prototype_semantic_tag'] = torch.index_select(
            semantic_tags[0], 0, label_batch[0]['prototype_batch_index'])
        for k in memory_banks.keys():
          assert label_batch[0].get(k, None) is None
          label_batch[0][k] = list(memory_banks[k])
        outputs = h_pred(embeddings[0], label_batch[0])
        losses = []
        for k in ['sem_ann_loss', 'sem_occ_loss', 'img_sim_loss', 'feat_aff_loss']:
          if outputs.get(k, None) is not None:
            outputs[k] = outputs[k].mean()
            losses.append(outputs[k])
        loss = sum(losses)
        lr = g_train.lr_poly(cfg_h1.train.base_lr, h_iter0 + step, cfg_h1.train.max_iteration,
                             cfg_h1.train.warmup_iteration)
        h_opt.zero_grad()
        loss.backward()
        h_opt.step(lr)
        with torch.no_grad():
          for k in list(label_batch[0].keys()):
            if 'prototype' in k and 'memory' not in k:
              memory_banks.setdefault('memory_' + k, []).append(label_batch[0][k].clone().detach())
              if len(memory_banks['memory_' + k]) > cfg_h1.train.memory_bank_size:
                memory_banks['memory_' + k] = memory_banks['memory_' + k][1:]
          for mem_lab in memory_banks.get('memory_prototype_batch_index', []):
            mem_lab += cfg_h1.train.batch_size * num_gpus
        names_e, sums_e = parameter_checksums(h_emb)
        names_p, sums_p = parameter_checksums(h_pred)
        t = 's%d_' % step
        h_store.update({
            t + 'image_seed': np.array(900 + step), t + 'image_head': datas['image'].reshape(-1)[:64],
            t + 'image_sums': np.array([datas['image'].double().sum().item(), datas['image'].double().abs().sum().item()]),
            t + 'semantic_label': targets['semantic_label'].to(torch.int16),
            t + 'instance_label': targets['instance_label'].to(torch.int16),
            t + 'semantic_tag': targets['semantic_tag'].to(torch.int16),
            t + 'sem_ann_loss': outputs['sem_ann_loss'], t + 'sem_occ_loss': outputs['sem_occ_loss'],
            t + 'img_sim_loss': outputs['img_sim_loss'], t + 'accuracy': outputs['accuracy'].mean(),
            t + 'loss': loss, t + 'lr': np.array(lr), t + 'n_prototypes': np.array(prototypes[0].shape[0]),
            t + 'emb_param_sums': sums_e, t + 'pred_param_sums': sums_p,
            t + 'aspp_w_head': dict(h_emb.named_parameters())['aspp.aspp_1.0.weight'].detach().reshape(-1)[:256].clone(),
            t + 'cls_w_head': dict(h_pred.named_parameters())['semantic_classifier.4.weight'].detach().reshape(-1)[:256].clone(),
        })
        if not dropout:
          # for the GPU step test's "given clustering" mode: the reference's own segment ids (the
          # chaotic k-means outcome, injected on the GPU) and d loss / d embedding map (every
          # 7th element + the two sums) -- everything downstream of the clustering is smooth
          d_emb = embeddings[0]['embedding'].grad.reshape(-1)
          h_store.update({
              t + 'cluster_index': seg_ids.to(torch.int16),
              t + 'd_embedding_strided': d_emb[::7].clone(),
              t + 'd_embedding_sums': np.array([d_emb.double().sum().item(), d_emb.double().abs().sum().item()]),
          })
    finally:
      e_dl.segsort_common.segment_by_kmeans = orig_sbk
    h_store['iter0'] = np.array(h_iter0)
    h_store['emb_param_names'] = np.array(names_e)
    h_store['pred_param_names'] = np.array(names_p)
    save(out, 'h01_step' if dropout else 'h01_step_nodrop', **h_store)

  run_h1(True)
  run_h1(False)

  # SGD alone: the reference class on a few tensors, three steps with changing lr / groups
  g = torch.Generator().manual_seed(5)
  w0 = [torch.randn(7, 5, generator=g), torch.randn(11, generator=g), torch.randn(3, 2, 2, generator=g)]
  grads = [[torch.randn(w.shape, generator=g) for w in w0] for _ in range(3)]
  ps = [torch.nn.Parameter(w.clone()) for w in w0]
  groups = [{'params': [ps[0]], 'lr': 1.0}, {'params': [ps[1]], 'lr': 2.0, 'weight_decay': 0.0},
            {'params': [ps[2]], 'lr': 10.0}]
  ref_sgd = ref_opt.SGD(groups, lr=1, momentum=0.9, weight_decay=5e-4)
  sgd_lrs = [3e-3, 1.7e-3, 2.9e-3]
  sgd_out = {}
  for i in range(3):
    for pth, gr in zip(ps, grads[i]):
      pth.grad = gr.clone()
    ref_sgd.step(sgd_lrs[i])
    for j, pth in enumerate(ps):
      sgd_out['w%d_after%d' % (j, i)] = pth.detach().clone()
  save(out, 'h01_sgd', lrs=np.array(sgd_lrs), **{'w%d' % j: w for j, w in enumerate(w0)},
       **{'g%d_%d' % (i, j): gr for i in range(3) for j, gr in enumerate(grads[i])}, **sgd_out)

  # ======================= N2 / N3: arithmetic blocks of the inference scripts ============
  # The scripts themselves cannot be imported (cv2, tensorboardX, hard-coded .cuda()), but the
  # blocks below are pure torch: their SOURCE LINES are read from the reference tree at run
  # time, dedented, stripped of the device moves and exec'd on seeded CPU inputs (nothing is
  # copied into the repository; only inputs and outputs are stored).
  import linecache
  import math
  import textwrap

  def ref_lines(path, first, last):
    txt = ''.join(linecache.getline(path, i) for i in range(first, last + 1))
    assert txt.strip(), path
    return textwrap.dedent(txt).replace('.to("cuda:0")', '').replace('.cuda()', '')

  # ---- N2: pyscripts/inference/prototype.py:134-205 (window ends, per-crop normalise +
  # overlap accumulation, division by the counts, full-image k-means, prototypes, majority
  # labels).  embedding_model: a seeded 5x5 conv as generate_embeddings, the reference's own
  # ResnetDeeplab.generate_clusters (on the CPU-shimmed segment_by_kmeans).
  import spml.models.embeddings.resnet_deeplab as e_dl2
  proto_py = os.path.join(args.ref, 'pyscripts', 'inference', 'prototype.py')
  src_n2 = ref_lines(proto_py, 134, 205)
  assert 'patch_ind_h' in src_n2 and 'find_majority_label_index' in src_n2

  class StubEmbedder:
    label_divisor = 2048
    semantic_ignore_index = 255
    kmeans_iterations = 10

    def __init__(self, conv, clusters):
      self.conv, self.kmeans_num_clusters = conv, clusters

    def generate_embeddings(self, datas, targets=None, resize_as_input=False):
      return {'embedding': self.conv(datas['image']), 'local_feature': None}

    generate_clusters = e_dl2.ResnetDeeplab.generate_clusters

  n2_store = {}
  orig_sbk2 = e_dl2.segsort_common.segment_by_kmeans
  e_dl2.segsort_common.segment_by_kmeans = ref_segment_by_kmeans
  try:
    for ci, (c, pad, valid, crop, stride, k) in enumerate([
        (16, (70, 90), (60, 83), (48, 48), (32, 32), (3, 3)),
        (8, (50, 50), (41, 50), (50, 50), (33, 33), (2, 2))]):
      gen = torch.Generator().manual_seed(1300 + ci)
      torch.manual_seed(1300 + ci)
      conv = torch.nn.Conv2d(3, c, 5, padding=2)
      base = torch.randn(1, 3, pad[0] // 8 + 2, pad[1] // 8 + 2, generator=gen)
      image = torch.nn.functional.interpolate(base, size=pad, mode='bilinear', align_corners=False)
      image = image + 0.05 * torch.randn(1, 3, pad[0], pad[1], generator=gen)
      sem = torch.randint(0, 5, (valid[0] // 10 + 1, valid[1] // 10 + 1), generator=gen)
      sem = sem.repeat_interleave(10, 0).repeat_interleave(10, 1)[:valid[0], :valid[1]].contiguous()
      fake = torch.full((1, pad[0], pad[1]), 255, dtype=torch.long)
      fake[:, :valid[0], :valid[1]] = 0                      # prototype.py:117-131
      env = {
          'config': AttrDict(test=AttrDict(stride=list(stride), crop_size=list(crop)),
                             network=AttrDict(label_divisor=2048)),
          'pad_image_h': pad[0], 'pad_image_w': pad[1], 'image_batch': {'image': image},
          'embedding_model': StubEmbedder(conv, list(k)), 'common_utils': g_common,
          'segsort_common': s_common, 'fake_label_batch': {'semantic_label': fake, 'instance_label': fake.clone()},
          'label_batch': {'semantic_label': sem.unsqueeze(0)}, 'math': math, 'np': np, 'torch': torch,
          'os': os, 'prototype_dir': '/nonexistent', 'base_name': 'x.png'}
      exec(compile(src_n2, proto_py + ':134-205', 'exec'), env)
      t = 'c%d_' % ci
      n2_store.update({
          t + 'image': image, t + 'sem': sem, t + 'conv_w': conv.weight, t + 'conv_b': conv.bias,
          t + 'cfg': np.array([c, pad[0], pad[1], valid[0], valid[1], crop[0], crop[1], stride[0],
                               stride[1], k[0], k[1]]),
          t + 'ends_h': env['patch_ind_h'], t + 'ends_w': env['patch_ind_w'],
          t + 'embedding': env['embeddings']['embedding'], t + 'counts': env['counts'],
          t + 'cluster_index': env['embeddings']['cluster_index'],
          t + 'prototypes': env['prototypes'], t + 'prototype_labels': env['prototype_labels']})
  finally:
    e_dl2.segsort_common.segment_by_kmeans = orig_sbk2
  save(out, 'n2_window', **n2_store)

  # ---- N3: pyscripts/inference/pseudo_camrw_crf.py:139-148 (per view: crop to the image,
  # un-flip, 1/8 bilinear, normalise, exp(5 cos - 5)) and :150-164 (mean over the views, CAM to
  # 1/8, 20th power, column normalisation, T <- T.T x WALK_STEPS, cam . T).
  rw_py = os.path.join(args.ref, 'pyscripts', 'inference', 'pseudo_camrw_crf.py')
  src_view = ref_lines(rw_py, 139, 148)
  src_walk = ref_lines(rw_py, 150, 164)
  assert 'exp_()' in src_view and 'WALK_STEPS' in src_walk
  walk_steps = None
  for i in range(20, 40):
    ln = linecache.getline(rw_py, i).strip()
    if ln.startswith('WALK_STEPS'):
      walk_steps = int(ln.split('=')[1])
  assert walk_steps == 6
  n3_store = {}
  for ci, (c, image_hw, pad_hw) in enumerate([(12, (56, 72), (64, 72)), (8, (32, 32), (32, 32))]):
    gen = torch.Generator().manual_seed(1400 + ci)
    image_h, image_w = image_hw
    views = []
    base = torch.randn(1, c, pad_hw[0] // 16 + 2, pad_hw[1] // 16 + 2, generator=gen)
    for flip in (False, True):
      e = torch.nn.functional.interpolate(base, size=pad_hw, mode='bilinear', align_corners=False)
      e = e + 0.2 * torch.randn(1, c, pad_hw[0], pad_hw[1], generator=gen)
      views.append((torch.flip(e, dims=[3]) if flip else e, flip))
    cam = torch.rand(21, image_h, image_w, generator=gen)
    env = {'torch': torch, 'F': torch.nn.functional, 'affs': [], 'image_h': image_h, 'image_w': image_w,
           'resize_image_h': image_h, 'resize_image_w': image_w, 'image_batch': None, 'label_batch': None,
           'WALK_STEPS': walk_steps, 'cam_full_arr': cam.clone()}
    for vi, (e, flip) in enumerate(views):
      env['embedding_model'] = lambda a, b, resize_as_input=True, _e=e: {'embedding': _e}
      env['data_info'] = {'is_flip': flip}
      exec(compile(src_view, rw_py + ':139-148', 'exec'), env)
      n3_store['c%d_view%d' % (ci, vi)] = e
      n3_store['c%d_flip%d' % (ci, vi)] = np.array(int(flip))
      n3_store['c%d_embs8_%d' % (ci, vi)] = env['embs']        # the 1/8-resolution unit embedding
    exec(compile(src_walk, rw_py + ':150-164', 'exec'), env)
    n3_store.update({'c%d_cam' % ci: cam, 'c%d_cam8' % ci: env['cam_full_arr'],
                     'c%d_trans' % ci: env['aff_mat'] / torch.sum(env['aff_mat'], dim=0, keepdim=True),
                     'c%d_cam_rw' % ci: env['cam_rw'], 'c%d_hw' % ci: np.array([image_h, image_w])})
  n3_store['walk_steps'] = np.array(walk_steps)
  save(out, 'n3_randomwalk', **n3_store)

  # ======================= N5 = N1 o N2: full-resolution kNN label inference ==============
  # pyscripts/inference/inference.py:162-227: window ends, per-crop normalise + overlap average,
  # k-means over the whole (padded) image with the padding ignored, Segsort.predictions against a
  # memory bank -> one label per un-padded pixel.  Same exec-the-lines arrangement as N2: a seeded
  # 5x5 conv as generate_embeddings, the reference's own generate_clusters and Segsort.
  inf_py = os.path.join(args.ref, 'pyscripts', 'inference', 'inference.py')
  src_n5 = ref_lines(inf_py, 162, 227)
  assert 'patch_ind_h' in src_n5 and 'with_prediction=True' in src_n5
  n5_store = {}
  e_dl2.segsort_common.segment_by_kmeans = ref_segment_by_kmeans
  try:
    for ci, (c, pad, valid, crop, stride, k, n_bank, n_cls) in enumerate([
        (16, (70, 90), (60, 83), (48, 48), (32, 32), (5, 5), 60, 5),
        (8, (50, 50), (41, 50), (50, 50), (33, 33), (6, 4), 33, 4)]):
      gen = torch.Generator().manual_seed(1500 + ci)
      torch.manual_seed(1500 + ci)
      conv = torch.nn.Conv2d(3, c, 5, padding=2)
      base = torch.randn(1, 3, pad[0] // 8 + 2, pad[1] // 8 + 2, generator=gen)
      image = torch.nn.functional.interpolate(base, size=pad, mode='bilinear', align_corners=False)
      image = image + 0.05 * torch.randn(1, 3, pad[0], pad[1], generator=gen)
      fake = torch.full((1, pad[0], pad[1]), 255, dtype=torch.long)
      fake[:, :valid[0], :valid[1]] = 0                      # inference.py:145-156
      # a memory bank that looks like the image's own segments: normalised embeddings of random pixels
      with torch.no_grad():
        full = g_common.normalize_embedding(conv(image).permute(0, 2, 3, 1).reshape(-1, c))
      pick = torch.randint(0, full.shape[0], (n_bank,), generator=gen)
      bank = g_common.normalize_embedding(full[pick] + 0.1 * torch.randn(n_bank, c, generator=gen))
      bank_lab = torch.randint(0, n_cls, (n_bank,), generator=gen)
      env = {
          'config': AttrDict(test=AttrDict(stride=list(stride), crop_size=list(crop)),
                             network=AttrDict(label_divisor=2048)),
          'pad_image_h': pad[0], 'pad_image_w': pad[1], 'image_batch': {'image': image},
          'embedding_model': StubEmbedder(conv, list(k)), 'common_utils': g_common,
          'fake_label_batch': {'semantic_label': fake, 'instance_label': fake.clone()},
          'prediction_model': model, 'semantic_memory_prototypes': bank,
          'semantic_memory_prototype_labels': bank_lab, 'math': math, 'np': np, 'torch': torch}
      exec(compile(src_n5, inf_py + ':162-227', 'exec'), env)
      t = 'c%d_' % ci
      pred = env['outputs']['semantic_prediction']
      assert pred.numel() == valid[0] * valid[1]             # inference.py:233 views it as the un-padded image
      n5_store.update({
          t + 'image': image, t + 'conv_w': conv.weight, t + 'conv_b': conv.bias,
          t + 'cfg': np.array([c, pad[0], pad[1], valid[0], valid[1], crop[0], crop[1], stride[0],
                               stride[1], k[0], k[1]]),
          t + 'bank': bank, t + 'bank_lab': bank_lab,
          t + 'cluster_index': env['embeddings']['cluster_index'].to(torch.int16),
          t + 'semantic_prediction': pred.view(valid[0], valid[1]).to(torch.uint8),
          t + 'semantic_topk': env['outputs']['semantic_score'].to(torch.uint8)[::7].clone()})
  finally:
    e_dl2.segsort_common.segment_by_kmeans = orig_sbk2
  save(out, 'n5_inference', **n5_store)

  # ======================= N6: full-resolution softmax inference + IoU counts ==============
  # pyscripts/inference/inference_softmax.py:105-148: window ends, per crop `embedding_model(crop,
  # resize_as_input=True)` and the reference's own SoftmaxClassifier in eval mode, the crops' outputs SUMMED into the
  # padded canvas (no counts), arg-max, crop to the un-padded size.  Same exec-the-lines arrangement as N2 / N5: the
  # seeded 5x5 conv as the embedding model (called as a function here), seeded head weights, non-trivial running
  # statistics.  `margin` = top-1 minus top-2 of the reference canvas per valid pixel: the tests compare labels where
  # it is at least 2e-4 * max|logit|, and fewer than 1 % of the valid pixels may fall below (asserted here).
  import spml.models.predictions.softmax_classifier as p_cls6
  sm_py = os.path.join(args.ref, 'pyscripts', 'inference', 'inference_softmax.py')
  src_n6 = ref_lines(sm_py, 105, 148)
  assert 'patch_ind_h' in src_n6 and 'torch.argmax(semantic_logits, 1)' in src_n6 and 'counts' not in src_n6

  class CallableStub(StubEmbedder):
    def __call__(self, datas, targets=None, resize_as_input=False):
      return self.generate_embeddings(datas, targets, resize_as_input=resize_as_input)

  n6_store = {}
  for ci, (c, ncls, pad, valid, crop, stride) in enumerate([
      (32, 5, (70, 90), (60, 83), (48, 48), (32, 32)),
      (64, 21, (50, 50), (41, 50), (50, 50), (33, 33))]):
    gen = torch.Generator().manual_seed(1600 + ci)
    torch.manual_seed(1600 + ci)
    conv = torch.nn.Conv2d(3, c, 5, padding=2)
    base = torch.randn(1, 3, pad[0] // 8 + 2, pad[1] // 8 + 2, generator=gen)
    image = torch.nn.functional.interpolate(base, size=pad, mode='bilinear', align_corners=False)
    image = image + 0.05 * torch.randn(1, 3, pad[0], pad[1], generator=gen)
    cfg6 = AttrDict(dataset=AttrDict(semantic_ignore_index=255, num_classes=ncls),
                    network=AttrDict(embedding_dim=c),
                    test=AttrDict(stride=list(stride), crop_size=list(crop)))
    head = p_cls6.SoftmaxClassifier(cfg6)
    with torch.no_grad():
      bn = head.semantic_classifier[1]
      bn.weight.copy_(0.5 + torch.rand(2 * c, generator=gen))
      bn.bias.copy_(0.1 * torch.randn(2 * c, generator=gen))
      bn.running_mean.copy_(0.05 * torch.randn(2 * c, generator=gen))
      bn.running_var.copy_(0.02 + 0.05 * torch.rand(2 * c, generator=gen))
      head.semantic_classifier[4].bias.copy_(0.1 * torch.randn(ncls, generator=gen))
    head.eval()
    env = {'config': cfg6, 'pad_image_h': pad[0], 'pad_image_w': pad[1], 'resize_image_h': valid[0],
           'resize_image_w': valid[1], 'image_batch': {'image': image},
           'embedding_model': CallableStub(conv, [1, 1]), 'prediction_model': head, 'math': math, 'np': np,
           'torch': torch}
    exec(compile(src_n6, sm_py + ':105-148', 'exec'), env)
    logit = env['semantic_logits']
    pred = env['semantic_pred']
    assert tuple(logit.shape) == (1, ncls, pad[0], pad[1]) and pred.shape == tuple(valid) and pred.dtype == np.uint8
    top2 = logit[0, :, :valid[0], :valid[1]].topk(2, dim=0).values
    margin = top2[0] - top2[1]
    low = (margin < 2e-4 * logit.abs().max()).float().mean().item()
    assert low < 0.01, 'case %d: %.4f of the valid pixels have a low margin -- pick another seed' % (ci, low)
    t = 'c%d_' % ci
    n6_store.update({
        t + 'image': image, t + 'conv_w': conv.weight, t + 'conv_b': conv.bias,
        t + 'cfg': np.array([c, ncls, pad[0], pad[1], valid[0], valid[1], crop[0], crop[1], stride[0], stride[1]]),
        t + 'semantic_logit': logit, t + 'semantic_pred': pred, t + 'margin': margin,
        t + 'state_names': np.array(list(head.state_dict().keys()))})
    n6_store.update({t + 'sd_' + k: v for k, v in head.state_dict().items()})
  # IoU counts: pyscripts/benchmark/benchmark_by_mIoU.py:25-53 (pure numpy; the module imports PIL at its top, so the
  # function's lines are exec'd).  Targets of 255 and a prediction >= num_classes at a valid pixel are included.
  iou_py = os.path.join(args.ref, 'pyscripts', 'benchmark', 'benchmark_by_mIoU.py')
  iou_env = {'np': np}
  exec(compile(ref_lines(iou_py, 25, 53), iou_py + ':25-53', 'exec'), iou_env)
  rs = np.random.RandomState(1650)
  iou_ncls = 7
  iou_target = rs.randint(0, iou_ncls, size=(37, 53)).astype(np.uint8)
  iou_pred = np.where(rs.rand(37, 53) < 0.6, iou_target, rs.randint(0, iou_ncls, size=(37, 53))).astype(np.uint8)
  iou_target[rs.rand(37, 53) < 0.1] = 255
  iou_target[0, 0], iou_pred[0, 0] = 3, iou_ncls + 2          # a prediction outside every bin at a valid pixel
  iou_target[0, 1], iou_pred[0, 1] = 255, iou_ncls + 2        # ... and at an ignored one
  tp_fn, tp_fp, tp = iou_env['iou_stats'](iou_pred, iou_target, num_classes=iou_ncls)
  n6_store.update({'iou_pred': iou_pred, 'iou_target': iou_target, 'iou_num_classes': np.array(iou_ncls),
                   'iou_counts': np.stack([tp_fn, tp_fp, tp]).astype(np.int64)})
  save(out, 'n6_softmax_inference', **n6_store)

  # ======================= N7: pseudo labels from the softmax head + affinity random walk ==
  if ONLY is None or 'n7_pseudo_labels' in ONLY:
    gen_n7(args.ref, out)

  # ======================= N8: multi-scale + flip softmax inference =========================
  if ONLY is None or 'n8_softmax_msc' in ONLY:
    gen_n8(args.ref, out)

  # ======================= N9: multi-scale + flip kNN inference ==============================
  if ONLY is None or 'n9_knn_msc' in ONLY:
    gen_n9(args.ref, out)
  if ONLY is None or 'n10_prototype_msc' in ONLY:
    gen_n10(args.ref, out)

  # ======================= N11: tag-recipe kNN pseudo labels, instance-weighted IoU ==========
  if ONLY is None or 'n11_pseudo_knn_msc' in ONLY:
    gen_n11(args.ref, out)
  if ONLY is None or 'n11_instance_iou' in ONLY:
    gen_n11_instance(args.ref, out)

  # ======================= N12: DensePose pseudo labels (tag propagation, walk) ==============
  if ONLY is None or 'n12_densepose_pseudo' in ONLY:
    gen_n12(args.ref, out)

  # ======================= N13: the numpy-only stages of the training augmentation ===========
  if ONLY is None or 'n13_augment' in ONLY:
    gen_n13(args.ref, out)

  # ======================= N14: sizes, order and flags of the inference programs' image chain ====
  if ONLY is None or 'n14_inference_io' in ONLY:
    gen_n14(args.ref, out)

  # ======================= N15: scoring directories (mIoU and instance-weighted IoU per file) ====
  if ONLY is None or 'n15_score_dirs' in ONLY:
    gen_n15(args.ref, out)

  # ======================= N16: the picture of a training summary (PCA embedding panels, label panels) ====
  if ONLY is None or 'n16_train_summary' in ONLY:
    gen_n16(args.ref, out)

  # ======================= H2: two steps of the stage-2 classifier training ===============
  # pyscripts/train/train_classifier.py:139-169, the loop body exec'd as it stands on ONE device:
  # the reference's ResnetDeeplab in eval mode under no_grad, its SoftmaxClassifier (dropout
  # p = 0: the GPU draws its mask from another generator) in train mode, ONE lib.nn.optimizer.SGD
  # over the groups of both models, poly lr.  DataParallel's calling convention (`model(*zip(...))`
  # -> list of per-device outputs, scatter_gather.gather) is stood in for by two lambdas.
  import spml.models.predictions.softmax_classifier as p_cls
  cls_py = os.path.join(args.ref, 'pyscripts', 'train', 'train_classifier.py')
  src_h2 = ref_lines(cls_py, 139, 169)
  assert 'prediction_model(*zip(embeddings, label_batch))' in src_h2 and 'optimizer.step(lr)' in src_h2
  cfg_h2 = AttrDict(
      train=AttrDict(base_lr=3e-3, max_iteration=4000, warmup_iteration=100, momentum=0.9,
                     weight_decay=5e-4, batch_size=2, lr_policy='poly'),
      dataset=AttrDict(semantic_ignore_index=255, num_classes=21),
      network=AttrDict(label_divisor=2048, embedding_dim=16, kmeans_num_clusters=[1, 1],
                       kmeans_iterations=0, use_syncbn=False, backbone_types='panoptic_deeplab_101'))
  c_emb = reinit_parameters(e_dl.ResnetDeeplab([1, 1, 1, 1], [1, 2, 1, 1], [1, 1, 2, 4], cfg_h2), 31)
  c_pred = reinit_parameters(p_cls.SoftmaxClassifier(cfg_h2), 33)
  c_pred.semantic_classifier[3].p = 0.0
  c_opt = ref_opt.SGD(c_emb.get_params_lr() + c_pred.get_params_lr(), lr=1,
                      momentum=cfg_h2.train.momentum, weight_decay=cfg_h2.train.weight_decay)
  c_opt.zero_grad()
  c_emb.eval()                                               # train_classifier.py:110-111
  c_pred.train()
  emb_sums_before = parameter_checksums(c_emb)[1]
  h2_store = {}
  orig_sbk3 = e_dl.segsort_common.segment_by_kmeans
  e_dl.segsort_common.segment_by_kmeans = ref_segment_by_kmeans
  try:
    for step in range(2):
      datas, targets = synth.make_batch(2, 161, seed=950 + step)
      env = {
          'torch': torch, 'config': cfg_h2, 'train_utils': g_train, 'optimizer': c_opt, 'curr_iter': 40 + step,
          'gpu_ids': ['cpu'], 'image_batch': [datas], 'label_batch': [dict(targets)],
          'embedding_model': lambda *pairs: [c_emb(*pr) for pr in pairs],
          'prediction_model': lambda *pairs: [c_pred(*pr) for pr in pairs],
          'scatter_gather': types.SimpleNamespace(
              gather=lambda outs, dev: {k: torch.stack([o[k] for o in outs]) if outs[0][k].dim() == 0
                                        else torch.cat([o[k] for o in outs], 0) for k in outs[0]})}
      exec(compile(src_h2, cls_py + ':139-169', 'exec'), env)
      names_p, sums_p = parameter_checksums(c_pred)
      t = 's%d_' % step
      h2_store.update({
          t + 'image_seed': np.array(950 + step), t + 'image_head': datas['image'].reshape(-1)[:64],
          t + 'image_sums': np.array([datas['image'].double().sum().item(), datas['image'].double().abs().sum().item()]),
          t + 'semantic_label': targets['semantic_label'].to(torch.int16),
          t + 'loss': env['loss'].detach(), t + 'accuracy': env['acc'].detach(), t + 'lr': np.array(env['lr']),
          t + 'pred_param_sums': sums_p,
          t + 'cls_w_head': dict(c_pred.named_parameters())['semantic_classifier.4.weight'].detach().reshape(-1)[:256].clone(),
          t + 'conv_w_head': dict(c_pred.named_parameters())['semantic_classifier.0.weight'].detach().reshape(-1)[:256].clone(),
          t + 'bn_running_mean': c_pred.semantic_classifier[1].running_mean.clone(),
          t + 'bn_running_var': c_pred.semantic_classifier[1].running_var.clone()})
  finally:
    e_dl.segsort_common.segment_by_kmeans = orig_sbk3
  # (the frozen network: not one parameter of it moved)
  assert torch.equal(parameter_checksums(c_emb)[1], emb_sums_before)
  h2_store['iter0'] = np.array(40)
  h2_store['pred_param_names'] = np.array(names_p)
  save(out, 'h02_classifier_step', **h2_store)

  # ======================= LR schedules ======================================
  its = np.arange(0, 30000, 37)
  save(out, 'h01_lr', its=its,
       poly=np.array([g_train.lr_poly(3e-3, int(i), 30000, 100) for i in its]),
       step=np.array([g_train.lr_step(3e-3, int(i), [20000, 25000], 100) for i in its]))

  # ======================= M1 / M2: the reference's model classes ============
  # ResnetDeeplab, ResnetPspnet and SoftmaxClassifier of the reference with the weights of
  # tests/tools_synth.reinit_parameters (the tests give this repository's classes the same ones):
  # state-dict names and shapes, LR groups, checkpoint name mapping and the outputs of seeded
  # inputs on CPU -- in fp64 (`*64`: fp32 convolutions differ by ~1e-5 between CPU models and
  # thread counts), the location features of the fp32 forward.
  import copy
  import spml.models.embeddings.resnet_pspnet as e_psp
  import spml.models.predictions.softmax_classifier as p_cls
  from spml_amd.train import voc12_scribble_config
  cfg_m = voc12_scribble_config(batch_size=1, embedding_dim=16)

  def sd_names(model):
    return np.array(['%s:%s' % (k, 'x'.join(str(s) for s in v.shape)) for k, v in model.state_dict().items()])

  gen = torch.Generator().manual_seed(41)
  m_net = reinit_parameters(e_dl.ResnetDeeplab([1, 1, 1, 1], [1, 2, 1, 1], [1, 1, 2, 4], cfg_m), 41).eval()
  m_img = torch.randn(1, 3, 65, 65, generator=gen)
  with torch.no_grad():
    m_out = m_net.generate_embeddings({'image': m_img})
    m_out64 = copy.deepcopy(m_net).double().generate_embeddings({'image': m_img.double()})
  save(out, 'm1_resnet_deeplab', state_dict=sd_names(m_net), image=m_img,
       embedding64=m_out64['embedding'], local_feature=m_out['local_feature'])

  p_net = reinit_parameters(e_psp.ResnetPspnet([1, 1, 1, 1], [1, 2, 1, 1], [1, 1, 2, 4], cfg_m), 42).eval()
  p_cls_m = reinit_parameters(p_cls.SoftmaxClassifier(cfg_m), 43).eval()
  p_img = torch.randn(1, 3, 65, 65, generator=gen)
  with torch.no_grad():
    p_out = p_net.generate_embeddings({'image': p_img}, resize_as_input=True)
    p_out64 = copy.deepcopy(p_net).double().generate_embeddings({'image': p_img.double()}, resize_as_input=True)
  names = {id(p): n for n, p in p_net.named_parameters()}
  groups = np.array(['%r|%r|%s' % (g['lr'], g.get('weight_decay'), ','.join(names[id(p)] for p in g['params']))
                     for g in p_net.get_params_lr()])
  c_emb = torch.randn(2, 16, 17, 17, generator=gen)
  c_lab = torch.randint(0, 23, (2, 33, 33), generator=gen)
  c_lab[0, :5] = 255
  c_out = copy.deepcopy(p_cls_m).double()({'embedding': c_emb.double()}, {'semantic_label': c_lab.clone()})
  save(out, 'm2_pspnet_softmax_classifier', state_dict=sd_names(p_net), image=p_img,
       embedding64=p_out64['embedding'], local_feature=p_out['local_feature'],
       lr_groups=groups, name_mapping=np.array([p_net.name_mapping('layer3.0.conv1.weight')]),
       cls_state_dict=sd_names(p_cls_m), cls_embedding=c_emb, cls_label=c_lab,
       semantic_logit64=c_out['semantic_logit'].detach(), sem_ann_loss64=c_out['sem_ann_loss'].detach(),
       accuracy64=c_out['accuracy'], semantic_prediction=c_out['semantic_prediction'],
       cls_lr_groups=np.array([[g['lr'], len(g['params'])] for g in p_cls_m.get_params_lr()], dtype=np.float64))

if __name__ == '__main__':
  main()
