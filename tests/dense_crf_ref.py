"""fp64 oracle of the dense CRF (`spml/models/crf.py:23-41` of twke18/SPML restated from the model; pydensecrf is not
needed): brute force over all N x N pixel pairs.  The pattern of tests/pseudo_label_ref.py: plain numpy, no GPU."""
import numpy as np

DEFAULTS = dict(iter_max=10, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
ALTERNATIVE = dict(iter_max=3, pos_w=5, pos_xy_std=3, bi_w=10, bi_xy_std=20, bi_rgb_std=13)


def _softmax(x, dtype):
  x = x - x.max(axis=0, keepdims=True)
  e = np.exp(x)
  return (e / e.sum(axis=0, keepdims=True)).astype(dtype)


def kernels(image, pos_xy_std, bi_xy_std, bi_rgb_std, dtype=np.float64):
  """-> (K1, K2) [N, N] of an image uint8 [h, w, 3]; pixel i = y * w + x, p = (x, y)."""
  h, w = image.shape[:2]
  yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
  xs, ys = xx.reshape(-1).astype(dtype), yy.reshape(-1).astype(dtype)
  rgb = image.reshape(-1, 3).astype(dtype)
  d_pos = (xs[:, None] - xs[None, :]) ** 2 + (ys[:, None] - ys[None, :]) ** 2
  # |a - b|^2 = |a|^2 + |b|^2 - 2 a.b: integers below 2^24, exact in either dtype (and far cheaper than N x N x 3)
  sq = (rgb * rgb).sum(1)
  d_rgb = sq[:, None] + sq[None, :] - dtype(2) * (rgb @ rgb.T)
  two = dtype(2)
  # (in place: the N x N temporaries are what this function costs)
  k1 = d_pos / (-two * dtype(pos_xy_std) ** 2)
  np.exp(k1, out=k1)
  d_pos /= -two * dtype(bi_xy_std) ** 2
  d_rgb /= -two * dtype(bi_rgb_std) ** 2
  d_pos += d_rgb
  np.exp(d_pos, out=d_pos)
  return k1, d_pos


def dense_crf(image, probmap, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std, dtype=np.float64):
  """image uint8 [h, w, 3], probmap [C, h, w] (not necessarily normalised) -> Q [C, h, w] in `dtype`.  dtype=np.float32
  is the same mathematics in fp32, the yardstick for rounding."""
  c, h, w = probmap.shape
  n = h * w
  unary = -np.log(np.clip(probmap.astype(dtype), dtype(1e-5), dtype(1))).reshape(c, n)
  k1, k2 = kernels(image, pos_xy_std, bi_xy_std, bi_rgb_std, dtype)
  n1 = (dtype(1) / np.sqrt(k1.sum(1) + dtype(1e-20))).astype(dtype)
  n2 = (dtype(1) / np.sqrt(k2.sum(1) + dtype(1e-20))).astype(dtype)
  q = _softmax(-unary, dtype)
  for _ in range(int(iter_max)):
    m1 = n1[None, :] * ((q * n1[None, :]) @ k1)                # (K = K^T: sum_j K[i,j] n[j] Q[c,j])
    m2 = n2[None, :] * ((q * n2[None, :]) @ k2)
    q = _softmax(-unary + dtype(pos_w) * m1 + dtype(bi_w) * m2, dtype)
  return q.reshape(c, h, w).astype(dtype)


# ---------------------------------------------------------------------------
# the generators of the GPU test list (tests/test_dense_crf_gpu.py)
def blocky(h, w, c, seed):
  """3 x 3 constant-colour regions +- 12 noise; logits favour one class per region."""
  rng = np.random.RandomState(seed)
  ry = np.minimum(np.arange(h) * 3 // max(h, 1), 2)
  rx = np.minimum(np.arange(w) * 3 // max(w, 1), 2)
  region = ry[:, None] * 3 + rx[None, :]
  colours = rng.randint(30, 226, size=(9, 3))
  image = colours[region] + rng.randint(-12, 13, size=(h, w, 3))
  image = np.clip(image, 0, 255).astype(np.uint8)
  favoured = rng.randint(0, c, size=9)[region]
  logits = rng.randn(c, h, w) * 1.0
  logits[favoured, np.arange(h)[:, None], np.arange(w)[None, :]] += 2.0
  return image, _softmax(logits, np.float32)


def flat(h, w, c, seed):
  rng = np.random.RandomState(seed)
  image = np.empty((h, w, 3), np.uint8)
  image[...] = rng.randint(0, 256, size=3)
  return image, _softmax(rng.randn(c, h, w), np.float32)


def noise(h, w, c, seed):
  rng = np.random.RandomState(seed)
  image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
  return image, _softmax(rng.randn(c, h, w) * 2.0, np.float32)


GENERATORS = {'blocky': blocky, 'flat': flat, 'noise': noise}

# (h, w, C) of the GPU test list: one pixel; N below one 32-pixel tile; N an exact multiple of the tile; ragged N; many
# tiles; both 32-class columns with long rows; one row; one class (Q must be all ones)
SHAPES = [(1, 1, 3), (7, 5, 2), (32, 40, 21), (33, 47, 5), (64, 64, 21), (17, 129, 64), (1, 300, 4), (9, 9, 1)]
PARAMETER_SETS = {'defaults': DEFAULTS, 'alternative': ALTERNATIVE}
