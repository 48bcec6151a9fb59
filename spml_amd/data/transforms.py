"""The *plan* of the reference's augmentation (`spml/data/transforms.py`, the `_training_preprocess` of its dataset
classes): what it draws, in its order and from its distributions -- and nothing else.  The functions return the
parameter record of `spml_augment_batch_u8` (include/spml_hip.h) instead of pixels; the pixels are made on the GPU by one
launch per batch (csrc/augment.hip).

The draws come from a `numpy.random.Generator` seeded by `(seed, epoch, index)`, never from global state: a sample's
augmentation is a function of those three numbers, whichever thread decodes it and whenever."""
import numpy as np


def sample_rng(seed, epoch, index):
  return np.random.default_rng([int(seed), int(epoch), int(index)])


def plan_mirror(rng):
  """transforms.py:91."""
  return bool(rng.uniform(0, 1.0) >= 0.5)


def plan_resize(rng, h, w, scale_min, scale_max, name=''):
  """transforms.py:61,26-27: ratio ~ U(scale_min, scale_max), new = int(ratio * side)."""
  assert scale_max >= scale_min
  ratio = rng.uniform(scale_min, scale_max)
  new_h, new_w = int(ratio * h), int(ratio * w)
  if new_h < 1 or new_w < 1:
    raise ValueError('%s: %d x %d at ratio %.4f has no pixel left' % (name or 'image', h, w, ratio))
  return new_h, new_w


def plan_crop(rng, h, w, crop_size):
  """transforms.py:134-137,184-186: the start of the crop in the plane padded up to `crop_size`."""
  pad_h, pad_w = max(h, crop_size[0]), max(w, crop_size[1])
  start_h = int(np.floor(rng.uniform(0, pad_h - crop_size[0])))
  start_w = int(np.floor(rng.uniform(0, pad_w - crop_size[1])))
  return start_h, start_w


def plan_grayscale(rng):
  """list_tag_dataset.py:201."""
  return bool(rng.uniform(0, 1.0) < 0.3)


def blur_weights(sigma):
  """list_tag_dataset.py:210-212."""
  w_x, w_y = np.meshgrid(np.linspace(-2, 2, 5), np.linspace(-2, 2, 5))
  weight = np.exp(-(w_x ** 2 + w_y ** 2) / sigma ** 2)
  return weight / weight.sum()


def plan_blur(rng):
  """list_tag_dataset.py:208-212: -> (blur?, 5 x 5 weights or None)."""
  if not rng.uniform(0, 1.0) < 0.5:
    return False, None
  return True, blur_weights(rng.uniform(0.1, 5))


def plan_training(rng, h, w, size, random_mirror, random_scale, random_crop, scale_range=(0.5, 1.5),
                  random_grayscale=False, random_blur=False, name=''):
  """The record of one training sample of an `h x w` file, drawn in the order of `_training_preprocess`
  (mirror, scale, crop, grayscale, blur).  A dict with the fields of `spml_augment_params` that do not depend on where
  the bytes end up (the batcher adds the offsets)."""
  if size is None or not random_crop:
    raise ValueError('training batches need `size` and `random_crop`: images of different sizes share one batch')
  flip = plan_mirror(rng) if random_mirror else False
  new_h, new_w = plan_resize(rng, h, w, scale_range[0], scale_range[1], name) if random_scale else (h, w)
  start_h, start_w = plan_crop(rng, new_h, new_w, size)
  gray = plan_grayscale(rng) if random_grayscale else False
  blur, weights = plan_blur(rng) if random_blur else (False, None)
  return {'h': int(h), 'w': int(w), 'new_h': new_h, 'new_w': new_w, 'flip': flip, 'start_h': start_h,
          'start_w': start_w, 'gray': gray, 'blur': blur,
          'weights': np.zeros((25,), np.float32) if weights is None else weights.reshape(25).astype(np.float32)}
