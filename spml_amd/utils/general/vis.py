"""Colour maps of the label images (`spml/utils/general/vis.py:51-59`) and the picture of a training summary (:23-48,
:62-101)."""
import os

import numpy as np


def load_color_map(color_map_path):
  """The table of a `.mat` file -> uint8 `[N, 3]` numpy array: the entry named after the file (its base name with the
  characters of '.mat' stripped from both ends, as the reference takes it), times 255, truncated to uint8."""
  import scipy.io
  color_map = scipy.io.loadmat(color_map_path)
  color_map = color_map[os.path.basename(color_map_path).strip('.mat')]
  return (color_map * 255).astype(np.uint8)


def voc_color_map():
  """The 256-entry PASCAL VOC table (bit-interleave of the class index: bit k of the index goes to bit 7 - k / 3 of
  channel k % 3), uint8 `[256, 3]`; what the programs colour with when `dataset.color_map_path` is empty.  Entry for
  entry the table of the reference's `misc/colormapvoc.mat` (tests/golden/n14_inference_io.npz)."""
  table = np.zeros((256, 3), dtype=np.uint8)
  for index in range(256):
    c = index
    for shift in range(7, -1, -1):
      for channel in range(3):
        table[index, channel] |= ((c >> channel) & 1) << shift
      c >>= 3
  return table


# ---------------------------------------------------------------------------
# The picture of a training summary (`spml/utils/general/vis.py:23-31,41-48,62-101`; csrc/train_summary.hip)
GRID_PADDING = 2                       # torchvision.utils.make_grid's default


def summary_grid_padding(n):
  """make_grid returns a single image as it is: no border for `n == 1`."""
  return 0 if n == 1 else GRID_PADDING


def summary_grid_shape(n, h, w):
  """(Htot, Wtot) of the summary picture of `n` images with an `h x w` embedding: the three `h x w` panels of an image
  side by side, the images stacked as `torchvision.utils.make_grid(nrow=1, padding=2)` stacks them -- every cell is
  the image plus the padding above and to its left, the grid one more padding below and to the right:
  `(n (h + 2) + 2, (3 w + 2) + 2)`, image `i` at row `2 + i (h + 2)`, column 2; `(h, 3 w)` for `n == 1`."""
  pad = summary_grid_padding(n)
  return n * (h + pad) + pad, 3 * w + 2 * pad


def summary_grid_origin(n, i, h):
  """(row, column) of the top-left pixel of image `i` in the picture of `n` images with an embedding `h` rows high."""
  pad = summary_grid_padding(n)
  return pad + i * (h + pad), pad


def fix_component_signs(basis):
  """The sign rule of the principal components (`torch.svd` leaves it to chance): the entry of largest magnitude of
  every column of `basis` (numpy `[C, k]`) is made positive; on a tie the lowest index wins.  Returns a new array."""
  basis = np.array(basis, dtype=np.float64, copy=True)
  for k in range(basis.shape[1]):
    lead = int(np.argmax(np.abs(basis[:, k])))           # (the first of equal maxima)
    if basis[lead, k] < 0:
      basis[:, k] = -basis[:, k]
  return basis


def leading_components(cov, num_components=3):
  """(V `[C, k]`, eigenvalues `[k]`), numpy fp64: the eigenvectors of the `k` largest eigenvalues of the symmetric
  `cov` (numpy or CPU tensor) in descending order, under the sign rule.  `torch.linalg.eigh` in fp64 on the host."""
  import torch
  cov = torch.as_tensor(np.asarray(cov, dtype=np.float64))
  values, vectors = torch.linalg.eigh(cov)
  order = list(range(cov.shape[0] - 1, cov.shape[0] - 1 - num_components, -1))
  return fix_component_signs(vectors[:, order].numpy()), values[order].numpy().copy()


def _normalized_rows(embeddings):
  """common.normalize_embedding of the `[N, C, H, W]` embedding as `[N, H, W, C]`, framework ops."""
  import torch
  rows = embeddings.detach().permute(0, 2, 3, 1).float()
  norm = rows.norm(dim=-1, keepdim=True)
  return rows / torch.where(norm >= 1e-12, norm, torch.full_like(norm, 1e-12))


def _hip_route(embeddings):
  from spml_amd import _ffi
  pixel_stride, channel_stride = _ffi.embedding_strides(embeddings)          # (raises for a CPU tensor)
  return _ffi.pca_path_name(embeddings.shape[1], pixel_stride, channel_stride) != 'unsupported'


def principal_components(embeddings, num_components=3):
  """(V fp32 `[C, k]` on the device, mean fp64 `[C]` on the device, eigenvalues fp64 `[k]` on the host) of the
  L2-normalised pixels of `embeddings` fp32 `[N, C, H, W]` on the GPU: the columns of V are what
  `common.calculate_principal_components` takes from `torch.svd` of the centred `P x C` matrix, up to their sign
  (`fix_component_signs`) -- the leading eigenvectors of the `C x C` covariance.  Moments on the device
  (`ops.pca_moments`; framework ops in fp64 where `ops.pca_path_name` says 'unsupported'), one 8 C^2-byte copy to the
  host, `torch.linalg.eigh` there."""
  import torch
  from spml_amd import ops
  embeddings = embeddings.detach()
  if embeddings.dtype != torch.float32:
    embeddings = embeddings.float()
  if _hip_route(embeddings):
    mean, cov = ops.pca_moments(embeddings)
  else:
    rows = _normalized_rows(embeddings).reshape(-1, embeddings.shape[1]).double()
    mean = rows.mean(0)
    rows = rows - mean
    cov = rows.t() @ rows / max(rows.shape[0] - 1, 1)
  basis, values = leading_components(cov.cpu(), num_components)
  return torch.from_numpy(basis).float().contiguous().to(embeddings.device), mean, torch.from_numpy(values)


def embedding_to_rgb(embeddings, project_type='pca'):
  """`[N, C, H, W]` embedding on the GPU -> uint8 `[N, 3, H, W]` on the GPU (`vis.py:62-101`): L2-normalise, project
  on the three leading principal components (un-centred, `common.py:68`), stretch every image's channels to 0..255,
  truncate.  Three library calls for C in {32, 64} (moments, projection + extrema, bytes), the same mathematics as
  framework ops on the device otherwise.  A channel may come out inverted against the reference's picture (the sign
  rule); a constant channel gives 0 where the reference divides 0 by 0.  `project_type='random'`: the reference's
  branch cannot run (`tf.long`, vis.py:84) and is not built."""
  import torch
  from spml_amd import ops
  if project_type == 'random':
    raise ValueError("embedding_to_rgb: project_type='random' is not built (the reference's branch cannot run)")
  if project_type != 'pca':
    raise NotImplementedError()
  embeddings = embeddings.detach()
  if embeddings.dtype != torch.float32:
    embeddings = embeddings.float()
  hip = _hip_route(embeddings)
  basis = principal_components(embeddings, 3)[0]
  if hip:
    proj, minmax = ops.pca_project_minmax(embeddings, basis)
    return ops.summary_panels(None, None, proj, minmax, None)
  n = embeddings.shape[0]
  proj = _normalized_rows(embeddings) @ basis                                  # [N, H, W, 3]
  flat = proj.view(n, -1, 3)
  low, high = flat.min(1, keepdim=True)[0], flat.max(1, keepdim=True)[0]
  span = high - low
  stretched = ((flat - low) / torch.where(span > 0, span, torch.ones_like(span))) * 255
  stretched = torch.where(span > 0, stretched, torch.zeros_like(stretched))
  return stretched.to(torch.uint8).view(proj.shape).permute(0, 3, 1, 2).contiguous()


def convert_label_to_color(label, color_map):
  """int64 `[n, h, w]` labels -> uint8 `[n, 3, h, w]` (`vis.py:41-48`): `color_map[label & 255]`.  The reference's
  `index_select` raises outside 0..255; the mask is the documented difference."""
  import torch
  table = torch.as_tensor(np.asarray(color_map) if not torch.is_tensor(color_map) else color_map).to(label.device)
  return table[(label & 255).long()].permute(0, 3, 1, 2)
