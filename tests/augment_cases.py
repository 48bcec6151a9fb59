"""The packed batches of tests/test_augment_gpu.py (and of the measurement that set its bound): sources, plans and the
fp64 restatement's outputs, computed once per seed.

Crop 29 x 37 (not square: a swapped axis shows; 37 is no multiple of the 32-pixel tile, 29 none of the 8-row one), five
sources of different sizes per launch, each with its own flags.  Every plan is written out by hand -- the ratios are the
issue's, `new = int(ratio * side)`."""
import numpy as np

import augment_ref as ref

CROP = (29, 37)
BIG_CROP = (65, 65)
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
IDENTITY = np.arange(256, dtype=np.uint8)
DENSEPOSE = IDENTITY.copy()
DENSEPOSE[:15] = [0, 1, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 14]
SEEDS = (0, 1, 2)


def weights(sigma):
  return ref.blur_weights(sigma).reshape(25).astype(np.float32)


def plan(h, w, ratio, start, flip=False, gray=False, sigma=None):
  return {'h': h, 'w': w, 'new_h': int(ratio * h), 'new_w': int(ratio * w), 'start_h': start[0], 'start_w': start[1],
          'flip': flip, 'gray': gray, 'blur': sigma is not None,
          'weights': np.zeros(25, np.float32) if sigma is None else weights(sigma)}


# name -> (crop, remap, plans)
BATCHES = {
    # A: the DensePose table.  20 x 27 at 0.5 -> 10 x 13 (padding right and below, start 0); 41 x 23 at 1.3 -> 53 x 29
    # (taller, narrower than the crop), mirrored: the remap applies; 70 x 90 at 1.5 -> 105 x 135 at the largest legal
    # start (76, 98), not mirrored: the table is present and must not apply; an interior start; 28 x 35 unscaled: the
    # padding begins at row 28 / column 35, one and two pixels inside the crop's far edges -- both in one 5 x 5 window
    'A': (CROP, DENSEPOSE, [
        plan(20, 27, 0.5, (0, 0)),
        plan(41, 23, 1.3, (11, 0), flip=True, gray=True),
        plan(70, 90, 1.5, (76, 98), sigma=5.0),
        plan(70, 90, 1.5, (13, 40), flip=True, gray=True, sigma=0.1),
        plan(28, 35, 1.0, (0, 0), flip=True, gray=True, sigma=5.0),
    ]),
    # B: identity table, other parameters on the same buffers.  58 x 74 at 0.5 is the crop itself (padded == S);
    # 20 x 27 at 2.0 -> 40 x 54 at its largest start; the blur alone with both sigmas; 1.3 with grayscale and blur
    'B': (CROP, IDENTITY, [
        plan(58, 74, 0.5, (0, 0)),
        plan(20, 27, 2.0, (11, 17), flip=True),
        plan(28, 35, 1.0, (0, 0), sigma=0.1),
        plan(28, 35, 1.0, (0, 0), flip=True, sigma=5.0),
        plan(41, 23, 1.3, (24, 0), gray=True, sigma=0.1),
    ]),
    # C, D: one image, a crop of several tiles per axis: blurred interior crop; padded on both sides
    'C': (BIG_CROP, DENSEPOSE, [plan(70, 90, 1.5, (20, 35), flip=True, sigma=5.0)]),
    'D': (BIG_CROP, IDENTITY, [plan(41, 23, 1.3, (0, 0), gray=True)]),
}

_cache = {}


def sources(plans, seed):
  """(rgb, sem, inst) per plan: random bytes; the semantic plane draws from 0..14, 254, 255 and holds each of 0, 14,
  254, 255 at least once."""
  rng = np.random.RandomState(4000 + seed)
  out = []
  for p in plans:
    h, w = p['h'], p['w']
    rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    sem = rng.choice(np.array(list(range(15)) + [254, 255], np.uint8), (h, w))
    sem.reshape(-1)[rng.choice(h * w, 4, replace=False)] = [0, 14, 254, 255]
    inst = rng.randint(0, 256, (h, w)).astype(np.uint8)
    out.append((rgb, sem, inst))
  return out


def case(name, seed):
  """-> dict(crop, remap, plans, samples, image fp64, sem, inst, tags): the restatement, computed once."""
  key = (name, seed)
  if key not in _cache:
    crop, remap, plans = BATCHES[name]
    samples = sources(plans, seed)
    image, sem, inst, tags = ref.augment_batch(samples, plans, crop, MEAN, STD, remap)
    for a in (image, sem, inst, tags):
      a.setflags(write=False)
    _cache[key] = {'crop': crop, 'remap': remap, 'plans': plans, 'samples': samples, 'image': image, 'sem': sem,
                   'inst': inst, 'tags': tags}
  return _cache[key]


def packed(c):
  """The batch as the batcher lays it out: (buffer uint8 numpy, records)."""
  from spml_amd.data import batcher
  full = [(r, s, i, p, k) for k, ((r, s, i), p) in enumerate(zip(c['samples'], c['plans']))]
  _, total = batcher.packed_layout(full)
  buf = np.zeros(total + 8, np.uint8)
  buf = buf[(-buf.ctypes.data) % 8:][:total]
  records = batcher.pack(full, buf)
  return buf, records
