"""fp64 numpy restatement of the reference's training augmentation (spml/data/transforms.py,
spml/data/datasets/base_dataset.py:135-155,183-186, list_tag_dataset.py:75-78,179-218, densepose_dataset.py:78-103): the
yardstick of csrc/augment.hip and of spml_amd.data.

cv2 is not installed where this suite is developed, so `cv2.resize` and `cv2.filter2D` are restated from their
formulas instead of being called; every numpy-only stage is held to the reference's own lines by
tests/golden/n13_augment.npz, the two resize modes and the blur to ATen on the CPU (tests/test_augment.py).

The stages run FORWARDS over whole arrays, in the reference's order -- the kernel composes them backwards per output
pixel, so the two share no code path.  Images are float64 HWC in [0, 1] from `uint8 / 255`."""
import numpy as np

RGB2GRAY = np.array([0.3, 0.59, 0.11], dtype=np.float32)      # list_tag_dataset.py:202: fp32 constants


def mirror(image, label):
  """transforms.py:76-78."""
  return image[:, ::-1, ...], label[:, ::-1, ...]


def axis_scale(src, dst):
  """cv2.resize with an explicit size: inv_scale = dst / src, scale = 1 / inv_scale, in double."""
  return 1.0 / (float(dst) / float(src))


def linear_taps(src, dst):
  """INTER_LINEAR along one axis: first tap, second tap, fraction (rounded to fp32) for every destination index."""
  scale = axis_scale(src, dst)
  f = (np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5
  s = np.floor(f)
  f = f - s
  s = s.astype(np.int64)
  low, high = s < 0, s >= src - 1
  s = np.where(low, 0, np.where(high, src - 1, s))
  f = np.where(low | high, 0.0, f)
  return s, np.minimum(s + 1, src - 1), f.astype(np.float32).astype(np.float64)


def nearest_taps(src, dst):
  """INTER_NEAREST along one axis."""
  scale = axis_scale(src, dst)
  return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * scale).astype(np.int64), src - 1)


def resize_linear(image, new_h, new_w):
  """cv2.resize(image, (new_w, new_h), INTER_LINEAR) of a float image [h, w, c]; no anti-aliasing."""
  image = np.asarray(image, dtype=np.float64)
  y0, y1, fy = linear_taps(image.shape[0], new_h)
  x0, x1, fx = linear_taps(image.shape[1], new_w)
  a0, a1 = (1.0 - fx)[None, :, None], fx[None, :, None]
  b0, b1 = (1.0 - fy)[:, None, None], fy[:, None, None]
  top = a0 * image[y0][:, x0] + a1 * image[y0][:, x1]
  bottom = a0 * image[y1][:, x0] + a1 * image[y1][:, x1]
  return b0 * top + b1 * bottom


def resize_nearest(label, new_h, new_w):
  """cv2.resize(label, (new_w, new_h), INTER_NEAREST)."""
  return label[nearest_taps(label.shape[0], new_h)][:, nearest_taps(label.shape[1], new_w)]


def resize_with_pad(image, size, pad_value):
  """transforms.py:134-151, pad_mode 'left_top'."""
  h, w = image.shape[:2]
  shape = list(image.shape)
  shape[0], shape[1] = max(h, size[0]), max(w, size[1])
  out = np.zeros(shape, dtype=image.dtype)
  if np.ndim(pad_value) == 0:
    out.fill(pad_value)
  else:
    for c, v in enumerate(pad_value):
      out[:, :, c].fill(v)
  out[:h, :w, ...] = image
  return out


def crop(image, start_h, start_w, size):
  """transforms.py:187-191."""
  return image[start_h:start_h + size[0], start_w:start_w + size[1], ...]


def grayscale(image):
  """list_tag_dataset.py:202-205: (r * 0.3 + g * 0.59) + b * 0.11 into three channels, in the image's own precision
  (the reference's fp32 image gives its bits; an fp64 image takes the fp32 constants exactly)."""
  k = RGB2GRAY.astype(image.dtype)
  g = (image[..., 0] * k[0] + image[..., 1] * k[1]) + image[..., 2] * k[2]
  return np.repeat(g[..., None], 3, axis=2)


def blur_weights(sigma):
  """list_tag_dataset.py:210-212."""
  w_x, w_y = np.meshgrid(np.linspace(-2, 2, 5), np.linspace(-2, 2, 5))
  weight = np.exp(-(w_x ** 2 + w_y ** 2) / sigma ** 2)
  return weight / weight.sum()


def filter2d(image, weight):
  """cv2.filter2D(image, -1, weight): correlation, anchor at the centre, BORDER_REFLECT_101."""
  k = weight.shape[0] // 2
  padded = np.pad(image, ((k, k), (k, k), (0, 0)), mode='reflect')
  out = np.zeros_like(image, dtype=np.float64)
  h, w = image.shape[:2]
  for i in range(weight.shape[0]):
    for j in range(weight.shape[1]):
      out += float(weight[i, j]) * padded[i:i + h, j:j + w]
  return out


def tags(semantic_label):
  """list_tag_dataset.py:75-78."""
  out = np.zeros((256,), dtype=np.int64)
  out[np.unique(semantic_label)] = 1
  return out


def augment_one(rgb, sem, inst, rec, size, mean, std, remap):
  """One image through the whole chain.  rgb uint8 [h, w, 3]; sem, inst uint8 [h, w]; `rec`: the plan (a mapping with
  new_h, new_w, flip, start_h, start_w, gray, blur, weights).  -> image float64 [3, S_h, S_w], sem, inst int64."""
  image = rgb.astype(np.float64) / 255.0
  label = np.stack([sem, inst], axis=2)
  if int(rec['flip']):
    image, label = mirror(image, label)
    label = label.copy()
    label[..., 0] = np.asarray(remap)[label[..., 0]]
  new_h, new_w = int(rec['new_h']), int(rec['new_w'])
  image, label = resize_linear(image, new_h, new_w), resize_nearest(label, new_h, new_w)
  mean = np.asarray(mean, dtype=np.float64)
  image = crop(resize_with_pad(image, size, mean), int(rec['start_h']), int(rec['start_w']), size)
  label = crop(resize_with_pad(label, size, 255), int(rec['start_h']), int(rec['start_w']), size)
  if int(rec['gray']):
    image = grayscale(image)
  if int(rec['blur']):
    image = filter2d(image, np.asarray(rec['weights'], dtype=np.float64).reshape(5, 5))
  image = (image - mean) / np.asarray(std, dtype=np.float64)
  return image.transpose(2, 0, 1), label[..., 0].astype(np.int64), label[..., 1].astype(np.int64)


def augment_batch(samples, records, size, mean, std, remap):
  """`samples`: (rgb, sem, inst) per image.  -> image [B, 3, S_h, S_w] float64, two int64 maps, tags [B, 256]."""
  outs = [augment_one(r, s, i, rec, size, mean, std, remap) for (r, s, i), rec in zip(samples, records)]
  return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]),
          np.stack([tags(s) for _, s, _ in samples]))
