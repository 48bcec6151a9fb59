"""The shapes of tests/test_inference_io.py and tests/test_inference_io_gpu.py, chosen once: the smallest that reach
every branch of csrc/inference_io.hip.

Views -- crop 33 x 33, scales 0.5 / 1 / 1.75 with flip:
  23 x 37 -> 11 x 18 (padded in both axes), 23 x 37 (padded in height only: 37 > 33), 40 x 64 (in neither; 64 = two
             full 32-pixel tiles)
  41 x 29 -> 20 x 14 (both), 41 x 29 (width only), 71 x 50 (neither; 50 is off the tile)
so every launch has views smaller than its tile grid (whole workgroups outside their own plane), widths on and off the
32-pixel tile, more than one workgroup per axis, and scale 1 (fraction 0: the normalised byte itself).
  23 x 43 at image_size 23 -> 12 x 22: the truncation quirk of resize_with_interpolation.
Export: identity out of a padded map, up-scaling and down-scaling, label values covering 0 .. 255."""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CROP = (33, 33)
SCALES = [0.5, 1, 1.75]

# (source h, w), scales, is_flip, image_size, the view sizes the plan must give (per scale)
VIEW_CASES = [((23, 37), SCALES, True, 0, [(11, 18), (23, 37), (40, 64)]),
              ((41, 29), SCALES, True, 0, [(20, 14), (41, 29), (71, 50)]),
              ((23, 43), [1], False, 23, [(12, 22)])]

# (pred h, w), (valid h, w), (out h, w)
EXPORT_CASES = [((33, 37), (23, 37), (23, 37)),      # identity out of a padded map
                ((33, 33), (12, 22), (23, 43)),      # up: the way back of 23 x 43 at image_size 23
                ((40, 64), (40, 64), (23, 37))]      # down


def source(hw, seed=0):
  """-> (rgb uint8 [h, w, 3], semantic uint8 [h, w]) with every byte value present."""
  rng = np.random.RandomState(1400 + seed + 7 * hw[0] + hw[1])
  rgb = rng.randint(0, 256, hw + (3,)).astype(np.uint8)
  rgb.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
  semantic = rng.choice(np.array([0, 1, 5, 14, 20, 254, 255], np.uint8), hw)
  return rgb, semantic


def prediction(pred_hw, valid_hw, seed=0):
  """int64 [pred_h, pred_w] whose valid rectangle holds every value 0 .. 255."""
  rng = np.random.RandomState(1500 + seed)
  pred = rng.randint(0, 256, pred_hw).astype(np.int64)
  valid = rng.randint(0, 256, valid_hw).astype(np.int64)
  valid.reshape(-1)[:256] = rng.permutation(256)
  pred[:valid_hw[0], :valid_hw[1]] = valid
  return pred


def color_map(seed=3):
  return np.random.RandomState(seed).randint(0, 256, (256, 3)).astype(np.uint8)
