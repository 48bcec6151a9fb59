"""Inputs and yardsticks of the DensePose pseudo-label tests (tests/test_densepose_pseudo.py, test_densepose_pseudo_gpu.py):
`pyscripts/inference/pseudo_denseposerw_crf.py:153-201` of twke18/SPML restated in fp64 on the CPU, taking the discrete
inputs (the nearest prototype of every pixel, the labels, the segment ids) as given, and seeded case builders for the
shape list the kernels are tested on.  Nothing here touches the code under test."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'n12_densepose_pseudo.npz')

# (half map (h2, w2), output (oh, ow), segments S, classes): a single output pixel and a single segment; one class; the
# golden's geometry (non-integer scales, taps that clamp at the border); more segments than a workgroup has threads; the
# class limit; the segment limit, which is the global table (S * ncls > 8192), most segments empty
SHAPES = [((4, 4), (1, 1), 1, 15), ((8, 8), (2, 2), 5, 1), ((21, 30), (5, 7), 37, 15), ((8, 64), (2, 16), 300, 21),
          ((17, 33), (4, 8), 64, 64), ((33, 47), (8, 11), 4096, 15)]
SEEDS = (1, 2, 3)
THRESHOLD = -1.0                   # what the program passes (:167)


def shape_id(shape):
  (h2, w2), (oh, ow), s, ncls = shape
  return '%dx%d-%dx%d-S%d-C%d' % (h2, w2, oh, ow, s, ncls)


@functools.lru_cache(maxsize=None)
def case(shape, seed=1):
  """Seeded inputs of one shape -> dict of read-only numpy arrays: `nn_index` int64 / `nn_value` fp32 `[N]`,
  `proto_label` int64 `[M]`, `cluster_index` int64 `[N]` (blocky, so that bilinear taps mix few rows).  About a tenth of
  the pixels has a similarity below the threshold, some prototypes carry the label `ncls` (the ignore value as the
  program maps it) or 254 (unlabelled): such pixels have no class.  Segment ids are drawn from a subset of `[0, S)` that
  leaves at least one id without a pixel (S = 1 has nothing to leave out); the last used id holds only class-less pixels
  where another id is left for the others."""
  (h2, w2), _, s, ncls = shape
  n = h2 * w2
  rng = np.random.RandomState(1000 * seed + 7 * s + ncls + n)
  used = np.arange(s) if s == 1 else np.sort(rng.choice(s, size=max(1, min(s - 1, n // 6)), replace=False))
  cells_y, cells_x = max(1, h2 // 3), max(1, w2 // 3)
  grid = used[rng.randint(0, len(used), size=(cells_y, cells_x))]
  iy = np.minimum(np.arange(h2) * cells_y // h2, cells_y - 1)
  ix = np.minimum(np.arange(w2) * cells_x // w2, cells_x - 1)
  clu = grid[iy][:, ix].reshape(-1).astype(np.int64)
  m = s + 2
  proto_label = rng.randint(0, ncls, size=m).astype(np.int64)
  proto_label[rng.rand(m) < 0.1] = ncls
  proto_label[rng.rand(m) < 0.1] = 254
  proto_label[0] = 0                                        # (at least one prototype with a class)
  nn_index = rng.randint(0, m, size=n).astype(np.int64)
  nn_value = rng.uniform(-0.6, 1.0, size=n).astype(np.float32)
  nn_value[rng.rand(n) < 0.1] = np.float32(-1.25)
  present = np.unique(clu)
  if len(present) > 1:
    nn_value[clu == present[-1]] = np.float32(-1.5)
  else:
    nn_index[0] = 0
    nn_value[0] = np.float32(0.5)                           # (the one segment keeps a counted pixel)
  out = {'nn_index': nn_index, 'nn_value': nn_value, 'proto_label': proto_label, 'cluster_index': clu}
  for a in out.values():
    a.setflags(write=False)
  return out


def pixel_classes(nn_index, nn_value, proto_label, threshold, ncls):
  """The class of every pixel, -1 for none (models/utils.py:207-221 with top_k = 1; a label outside `[0, ncls)` is no
  class)."""
  lab = np.asarray(proto_label)[np.asarray(nn_index)]
  none = (np.asarray(nn_value) < np.float32(threshold)) | (lab < 0) | (lab >= ncls)
  return np.where(none, -1, lab)


def segment_counts(classes, cluster_index, s, ncls):
  """counts int64 `[S, ncls]`: the pixels of every segment per class (the scatter-add of the one-hot rows, :172-173)."""
  counts = np.zeros((s, ncls), np.int64)
  ok = classes >= 0
  np.add.at(counts, (np.asarray(cluster_index)[ok], classes[ok]), 1)
  return counts


def segment_probs(counts, cluster_index):
  """:172-174 in fp64: `segment_mean` (the counts over the pixels of the segment, an empty segment divided by 1) and the
  division of every row by its sum; a row without a counted pixel is zeros (the reference has 0 / 0 there)."""
  s = counts.shape[0]
  pixels = np.bincount(np.asarray(cluster_index), minlength=s).astype(np.float64)
  mean = counts.astype(np.float64) / np.where(pixels == 0, 1.0, pixels).reshape(-1, 1)
  total = mean.sum(1, keepdims=True)
  return np.where(total > 0, mean / np.where(total > 0, total, 1.0), 0.0)


def resampled(probs, cluster_index, half_hw, out_hw):
  """:175-182 in fp64: the rows gathered per pixel, `[h2, w2, ncls]` -> `[ncls, h2, w2]`, `F.interpolate(mode='bilinear')`
  on the CPU -> `[ncls, oh, ow]`."""
  h2, w2 = half_hw
  pixel = torch.from_numpy(probs[np.asarray(cluster_index)]).view(1, h2, w2, -1).permute(0, 3, 1, 2).contiguous()
  return F.interpolate(pixel, size=tuple(out_hw), mode='bilinear')[0].numpy()


def segment_cam(nn_index, nn_value, proto_label, threshold, cluster_index, s, ncls, half_hw, out_hw):
  """-> (counts int64 `[S, ncls]`, probs fp64 `[S, ncls]`, acc fp64 `[ncls, oh, ow]`): :159-182."""
  classes = pixel_classes(nn_index, nn_value, proto_label, threshold, ncls)
  counts = segment_counts(classes, cluster_index, s, ncls)
  probs = segment_probs(counts, cluster_index)
  return counts, probs, resampled(probs, cluster_index, half_hw, out_hw)


def normalized_cam(acc, tags, background_threshold=None):
  """:183-190 in fp64: every class over its maximum, the classes the image does not carry zero, class 0 the background
  value when one is given."""
  acc = np.asarray(acc, np.float64)
  peak = acc.reshape(acc.shape[0], -1).max(1).reshape(-1, 1, 1)
  with np.errstate(invalid='ignore', divide='ignore'):
    cam = acc / peak
  cam[~np.asarray(tags, bool)] = 0.0
  if background_threshold is not None:
    cam[0] = background_threshold
  return cam


def walked(cam, trans, walk_steps=6):
  """:196-201 in fp64 on a given transition matrix (the matrix before the squarings)."""
  t = np.asarray(trans, np.float64)
  for _ in range(walk_steps):
    t = t @ t
  return (np.asarray(cam, np.float64).reshape(cam.shape[0], -1) @ t).reshape(cam.shape)


@functools.lru_cache(maxsize=None)
def yardstick(shape, seed=1):
  """(the case, counts, probs, acc) of one shape, computed once and shared by the tests; read-only."""
  half_hw, out_hw, s, ncls = shape
  c = case(shape, seed)
  out = segment_cam(c['nn_index'], c['nn_value'], c['proto_label'], THRESHOLD, c['cluster_index'], s, ncls, half_hw,
                    out_hw)
  for a in out:
    a.setflags(write=False)
  return (c,) + out


@functools.lru_cache(maxsize=None)
def golden_cases():
  """The two cases of tests/golden/n12_densepose_pseudo.npz (tools/gen_golden.py: gen_n12) -> list of dicts of arrays;
  integer arrays widened to int64, `half_hw`, `out_hw`, `ncls` and `num_segments` added."""
  z = np.load(GOLDEN)
  cases = []
  for ci in range(2):
    t = 'c%d_' % ci
    d = {k[len(t):]: z[k] for k in z.files if k.startswith(t)}
    for k, v in list(d.items()):
      if v.dtype in (np.int16, np.uint8) and k != 's_tags':
        d[k] = v.astype(np.int64)
    _, ncls, h, w = (int(v) for v in d['cfg'][:4])
    d.update(half_hw=(h // 2, w // 2), out_hw=(h // 8, w // 8), image_hw=(h, w), ncls=ncls,
             num_segments=int(d['proto_label'].shape[0]))
    cases.append(d)
  return cases
