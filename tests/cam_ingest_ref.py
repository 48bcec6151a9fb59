"""Yardstick of the CAM ingest kernel (`spml_cam_ingest_f32`): the four-tap expression in fp64, the kernel cases, and the
bound the kernel is held to.

`pseudo_camrw_crf.py:108-111` stacks the planes of a CAM file into `[ncls, h, w]` with the background `(1 - max_fg) **
ALPHA` at class 0, and :151-152 reduces the array with `F.interpolate(scale_factor=1/8, mode='bilinear')`.  That call
takes the GIVEN factor for the source coordinate, `8 (d + 0.5) - 0.5 = 8 d + 3.5`: an output pixel is the mean of the four
source pixels at rows `8 y + 3, 8 y + 4` and columns `8 x + 3, 8 x + 4`.  `four_tap` states that in fp64 (Y); `reference`
runs the reference's own lines (R, tests/random_walk_crf_ref.py: numpy for :108-111, ATen on the CPU for :151-152).
tests/test_cam_lists.py pins the tap model, `max |R - Y| <= 4 * 2^-24 * max |Y|` on every case, and the kernel is held to
`max |G - Y| <= 4 * max(max |R - Y|, 2^-24 * max |Y|)`: four times the reference's own deviation, because the kernel may
add the taps in another order than ATen and take the power by multiplication."""
import numpy as np

import random_walk_crf_ref

U = 2.0 ** -24
ALPHA = 6

# (h, w, ncls, keys, shift): the planes are uniform in [0, 1) + shift; keys in the order the planes are given
CASES = [
    (8, 8, 21, [], 0.0),                      # the smallest image, a file without entries: the background is exactly 1
    (9, 15, 2, [0], -0.6),                    # every class present and negative activations: no clamp at 0
    (17, 23, 3, [0, 1], -0.6),
    (41, 16, 21, [19], 0.0),                  # the last class alone; w // 8 = 2
    (33, 40, 21, list(range(20)), 0.0),       # every class present
    (97, 129, 21, [7, 19, 2], 0.0),           # keys out of order; more than one workgroup (12 x 16 = 192 output pixels)
]
IDS = ['%dx%dx%d_k%d' % (h, w, n, len(k)) for h, w, n, k, _ in CASES]


def planes_of(case, seed=7):
  h, w, _, keys, shift = case
  rng = np.random.RandomState(seed + 31 * h + w)
  planes = (rng.rand(len(keys), h, w) + shift).astype(np.float32)
  planes.setflags(write=False)
  return planes


def four_tap(planes, keys, hw, ncls, alpha=ALPHA):
  """Y: fp64 `[ncls, h // 8, w // 8]` from fp32 planes `[K, h, w]` and their keys (class - 1)."""
  h, w = hw
  full = np.zeros((ncls, h, w), np.float64)
  for plane, key in zip(planes, keys):
    full[key + 1] = plane.astype(np.float64)
  if ncls > 1:
    full[0] = (1.0 - full[1:].max(axis=0)) ** alpha        # (the zero planes of absent classes take part, as in :111)
  else:
    full[0] = 1.0
  oh, ow = h // 8, w // 8
  rows, cols = 8 * np.arange(oh) + 3, 8 * np.arange(ow) + 3
  taps = [full[:, rows + dy][:, :, cols + dx] for dy in (0, 1) for dx in (0, 1)]
  return (taps[0] + taps[1] + taps[2] + taps[3]) / 4.0


def reference(planes, keys, hw, ncls, alpha=ALPHA):
  """R: the reference's own lines, fp32 `[ncls, h // 8, w // 8]`."""
  cam = {int(key): plane for plane, key in zip(planes, keys)}
  return random_walk_crf_ref.reference_cam_down(random_walk_crf_ref.reference_cam_full(cam, hw, alpha, ncls)).numpy()


def bound(want, reference_deviation):
  return 4.0 * max(reference_deviation, U * float(np.abs(want).max()))
