"""Inputs and yardsticks of the random-walk + dense-CRF tests (tests/test_random_walk_crf.py, test_random_walk_crf_gpu.py):
the tail of `pyscripts/inference/pseudo_softmaxrw_crf.py:172-187` and the CAM lines of `pseudo_camrw_crf.py:108-111,
151-152` of twke18/SPML, restated on the CPU from the two existing yardsticks (tests/dense_crf_ref.py, fp64 over all
pixel pairs; tests/pseudo_label_ref.py, the up-sampling).  Nothing here touches the code under test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import dense_crf_ref
import pseudo_label_ref

# (h, w, C): a 1 x 1 map (every pixel has the same taps: all labels tied by construction, compared on Q only); two
# classes; ragged N; N a multiple of the 32-pixel tile; many tiles; both 32-class tiles; one row
SHAPES = [(8, 8, 3), (16, 24, 2), (33, 47, 5), (32, 40, 21), (64, 64, 21), (17, 129, 64), (1, 300, 4)]
MARGIN = 1e-3                      # labels are compared where the yardstick's top two marginals are further apart
SEED = 1


def walked_map(h, w, c, seed):
  """-> (image uint8 [h, w, 3], low fp32 [c, max(h//8, 1), max(w//8, 1)]): what the walk hands to the tail -- every class
  divided by its own maximum (values in [0, 1], not a distribution), the last class absent (all zero) when c > 2."""
  image = dense_crf_ref.blocky(h, w, c, seed)[0]
  low = dense_crf_ref.blocky(max(h // 8, 1), max(w // 8, 1), c, seed + 100)[1]
  low = low / low.reshape(c, -1).max(1).reshape(c, 1, 1)
  if c > 2:
    low[c - 1] = 0.0
  return image, low.astype(np.float32)


def upsampled(low, image_hw):
  """`pseudo_label_ref.upsampled` (F.interpolate, bilinear, align_corners=False, on the CPU) of a numpy map -> numpy fp32."""
  return pseudo_label_ref.upsampled(torch.from_numpy(np.array(low)), image_hw).numpy()


def label_cap(shape):
  """Largest share of pixels that may fall under MARGIN where labels are compared; None: compared on Q only."""
  if shape == (8, 8, 3):
    return None
  if shape == (17, 129, 64):
    return 0.20
  assert 1 < shape[2] <= 21
  return 0.02


def under_margin(want):
  """-> (keep: bool [h, w], the pixels outside the margin; the share left out)."""
  top = np.sort(want, axis=0)
  keep = (top[-1] - top[-2]) > MARGIN
  return keep, 1.0 - float(keep.mean())


@functools.lru_cache(maxsize=None)
def yardstick(shape, parameters, seed=SEED):
  """(image, low, up fp32 [c, h, w], fp64 Q [c, h, w]) of one case, computed once and shared by the tests; read-only."""
  h, w, c = shape
  image, low = walked_map(h, w, c, seed)
  up = upsampled(low, (h, w))
  want = dense_crf_ref.dense_crf(image, up, **dense_crf_ref.PARAMETER_SETS[parameters])
  for a in (image, low, up, want):
    a.setflags(write=False)
  return image, low, up, want


# ---------------------------------------------------------------------------
# pseudo_camrw_crf.py, the lines themselves
def reference_cam_full(cam, image_hw, alpha, num_classes=21):
  """:108-111 (numpy): `cam` {class - 1: [h, w]} -> [num_classes, h, w] with the background at class 0."""
  image_h, image_w = image_hw
  cam_full_arr = np.zeros((num_classes, image_h, image_w), np.float32)
  for k, v in cam.items():
    cam_full_arr[k + 1] = v
  cam_full_arr[0] = np.power(1 - np.max(cam_full_arr[1:], axis=0, keepdims=True), alpha)
  return cam_full_arr


def reference_cam_down(cam_full_arr):
  """:151-152 (torch, here on the CPU)."""
  cam_full_arr = torch.from_numpy(cam_full_arr)
  return F.interpolate(cam_full_arr.unsqueeze(0), scale_factor=1 / 8., mode='bilinear').squeeze(0)
