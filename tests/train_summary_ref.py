"""The yardstick of the training-summary picture (csrc/train_summary.hip, spml_amd/summary.py): the reference's chain
-- `vis.embedding_to_rgb` (vis.py:62-101), `common.pca` / `calculate_principal_components` (common.py:29-73),
`normalize_embedding` (:101-120), `convert_label_to_color` (vis.py:41-48), `write_image_to_tensorboard` (:23-31) with
`torchvision.utils.make_grid(nrow=1)` -- restated in fp64 numpy.  Nothing here imports the package under test.

Differences from the reference, as the library documents them: the principal components come from `eigh` of the
C x C covariance under a sign rule (the reference takes `torch.svd`'s, whose signs are arbitrary); labels are masked
with 255 before the table look-up; a constant channel stretches to 0."""
import numpy as np

EPS = 1e-12


def normalized_rows(emb):
  """`[N, C, H, W]` -> fp64 `[N, H, W, C]`, every pixel divided by max(||x||, 1e-12)."""
  rows = np.transpose(np.asarray(emb, dtype=np.float64), (0, 2, 3, 1))
  norm = np.sqrt((rows * rows).sum(-1, keepdims=True))
  return rows / np.where(norm >= EPS, norm, EPS)


def moments(emb):
  """(mean `[C]`, cov `[C, C]`) of the normalised pixels; cov is divided by max(P - 1, 1)."""
  rows = normalized_rows(emb).reshape(-1, np.asarray(emb).shape[1])
  mean = rows.mean(0)
  centred = rows - mean
  return mean, centred.T @ centred / max(rows.shape[0] - 1, 1)


def fix_signs(basis):
  """The entry of largest magnitude of every column positive; of equal magnitudes the one of lowest index counts."""
  basis = np.array(basis, dtype=np.float64)
  for k in range(basis.shape[1]):
    mags = np.abs(basis[:, k])
    lead = min(i for i in range(mags.size) if mags[i] == mags.max())
    if basis[lead, k] < 0:
      basis[:, k] *= -1.0
  return basis


def eigenvalues(cov):
  """All eigenvalues of `cov`, descending."""
  return np.linalg.eigvalsh(np.asarray(cov, dtype=np.float64))[::-1].copy()


def components(cov, k=3):
  """(V `[C, k]`, eigenvalues `[k]`): eigenvectors of the k largest eigenvalues, descending, sign rule applied."""
  values, vectors = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
  order = np.argsort(values)[::-1][:k]
  return fix_signs(vectors[:, order]), values[order]


def project(emb, basis):
  """proj fp64 `[N, H, W, k]` = normalised row . basis (NOT centred: common.py:68)."""
  return normalized_rows(emb) @ np.asarray(basis, dtype=np.float64)


def extrema(proj):
  """`[N, k, 2]`: (min, max) per image and channel."""
  n, k = proj.shape[0], proj.shape[-1]
  flat = proj.reshape(n, -1, k)
  return np.stack([flat.min(1), flat.max(1)], axis=-1)


def stretch(proj, minmax):
  """(t, bytes): t = 255 (v - min) / (max - min) as a float `[N, H, W, k]` (0 for a constant channel), bytes = trunc(t)."""
  proj = np.asarray(proj, dtype=np.float64)
  low = np.asarray(minmax, dtype=np.float64)[:, None, None, :, 0]
  span = np.asarray(minmax, dtype=np.float64)[:, None, None, :, 1] - low
  t = np.where(span > 0, (proj - low) / np.where(span > 0, span, 1.0), 0.0) * 255.0
  return t, np.floor(t).astype(np.uint8)


def nearest_index(out_size, in_size):
  """`F.interpolate(mode='nearest')`: min(floor(dst * (fp32) in / out), in - 1), the product in fp32."""
  scale = np.float32(in_size) / np.float32(out_size)
  src = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
  return np.minimum(src, in_size - 1)


def label_panel(label, color_map, h, w):
  """int `[N, Hl, Wl]` -> uint8 `[N, h, w, 3]`: nearest resize, `color_map[label & 255]`."""
  label = np.asarray(label).astype(np.int64)
  rows, cols = nearest_index(h, label.shape[1]), nearest_index(w, label.shape[2])
  return np.asarray(color_map, dtype=np.uint8)[label[:, rows][:, :, cols] & 255]


def make_grid(images, padding=2):
  """`torchvision.utils.make_grid(images, nrow=1)` for uint8 `[N, 3, H, W]`: one image comes back as it is; otherwise
  every cell is (H + padding) x (W + padding), the grid `[3, N cellH + padding, cellW + padding]` of zeros, image i at
  row i cellH + padding, column padding."""
  images = np.asarray(images)
  n = images.shape[0]
  if n == 1:
    return images[0].copy()
  cell_h, cell_w = images.shape[2] + padding, images.shape[3] + padding
  grid = np.zeros((images.shape[1], cell_h * n + padding, cell_w + padding), dtype=images.dtype)
  for i in range(n):
    grid[:, i * cell_h + padding:i * cell_h + padding + cell_h - padding, padding:padding + cell_w - padding] = images[i]
  return grid


def picture(semantic, instance, emb_bytes, color_map):
  """uint8 `[3, Htot, Wtot]` from the label maps and the embedding's bytes `[N, h, w, 3]`."""
  h, w = emb_bytes.shape[1:3]
  rows = np.concatenate([label_panel(semantic, color_map, h, w), label_panel(instance, color_map, h, w),
                         np.asarray(emb_bytes, dtype=np.uint8)], axis=2)             # [N, h, 3 w, 3]
  return make_grid(np.transpose(rows, (0, 3, 1, 2)))


def chain(emb, semantic=None, instance=None, color_map=None, basis=None):
  """Everything at once.  `basis`: use these components (any dtype) instead of the covariance's."""
  mean, cov = moments(emb)
  own_basis, values = components(cov)
  basis = own_basis if basis is None else np.asarray(basis, dtype=np.float64)
  proj = project(emb, basis)
  minmax = extrema(proj)
  t, bytes_ = stretch(proj, minmax)
  out = dict(mean=mean, cov=cov, basis=basis, values=values, proj=proj, minmax=minmax, t=t, bytes=bytes_)
  if semantic is not None:
    out['picture'] = picture(semantic, instance, bytes_, color_map)
  return out


def near_integer(t, delta):
  """Mask of the values of `t` within `delta` of an integer (where a deviation of `delta` can change the byte)."""
  return np.abs(t - np.round(t)) <= delta
