"""The *plan* of the reference's augmentation (`spml/data/transforms.py`, the `_training_preprocess` of its dataset
classes): what it draws, in its order and from its distributions -- and nothing else.  The functions return the
parameter record of `spml_augment_batch_u8` (include/spml_hip.h) instead of pixels; the pixels are made on the GPU by one
launch per batch (csrc/augment.hip).  `plan_views` is the same for the inference programs: the views of one file in the
reference's order and sizes, as the records of `spml_image_views_u8` (csrc/inference_io.hip).

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


def _align16(n):
  return (int(n) + 15) // 16 * 16


def plan_views(h, w, scales, is_flip, crop_size, image_size=0, name=''):
  """The views of one `h x w` file at inference, in the reference's order and arithmetic: per scale the flipped view
  first, then the plain one (`create_image_pyramid`, spml/utils/general/others.py:29-32); `new = int(scale * side)` in
  Python doubles (transforms.py:26-27); with `image_size > 0` (the single-view programs; only with `scales == [1]`) the
  larger side goes to `image_size`: `ratio = min(S / h, S / w)`, `new = int(ratio * side)` (transforms.py:110-113; the
  truncation can leave the larger side one short of S); `pad = max(new, crop)` per axis (transforms.py:134-137).
  -> list of dicts with the fields of `spml_view_params`; `image_off` / `label_off` are byte offsets into one fp32 and
  one int64 buffer, packed in view order with 16-byte alignment (`view_buffer_bytes`: the sizes of the two)."""
  h, w = int(h), int(w)
  scales = list(scales)
  if image_size and image_size > 0:
    if scales != [1]:
      raise ValueError('plan_views: image_size goes with scales == [1] (the single-view programs), not %r' % (scales,))
    new_size = float(image_size)
    ratio = min(new_size / h, new_size / w)
    sizes = [(int(ratio * h), int(ratio * w))]
  else:
    sizes = [(int(scale * h), int(scale * w)) for scale in scales]
  views, image_off, label_off = [], 0, 0
  for (new_h, new_w), scale in zip(sizes, scales):
    if new_h < 1 or new_w < 1:
      raise ValueError('%s: %d x %d at scale %s has no pixel left' % (name or 'image', h, w, scale))
    pad_h, pad_w = max(new_h, int(crop_size[0])), max(new_w, int(crop_size[1]))
    for flip in ((True, False) if is_flip else (False,)):
      views.append({'new_h': new_h, 'new_w': new_w, 'pad_h': pad_h, 'pad_w': pad_w, 'flip': flip,
                    'image_off': image_off, 'label_off': label_off})
      image_off = _align16(image_off + 3 * pad_h * pad_w * 4)
      label_off = _align16(label_off + new_h * new_w * 8)
  return views


def view_buffer_bytes(views):
  """-> (bytes of the fp32 buffer, bytes of the int64 buffer) that hold every plane of `plan_views`' records."""
  return (max(v['image_off'] + 3 * v['pad_h'] * v['pad_w'] * 4 for v in views),
          max(v['label_off'] + v['new_h'] * v['new_w'] * 8 for v in views))
