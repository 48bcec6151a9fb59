"""Training summaries: what `pyscripts/train/train.py:222-258` of the reference hands to tensorboardX every
`config.train.tensorboard_step` iterations, as files.

  <directory>/image-{iter:07d}.png   per image of the batch, side by side: semantic labels in colour, instance labels
                                     in colour, the embedding projected to RGB by PCA; the images stacked as
                                     `torchvision.utils.make_grid(nrow=1)` stacks them (`vis.summary_grid_shape`)
  <directory>/scalars.jsonl          one line per summary: iter, the loss terms that are present, accuracy, loss, lr,
                                     step_ms, images_per_s

The picture is made on the device by three library calls (`ops.pca_moments`, `ops.pca_project_minmax`,
`ops.summary_panels`; csrc/train_summary.hip) around a 64 x 64 eigenproblem on the host; only its bytes and the
covariance leave the device.  A writer thread encodes the PNG.  tensorboard event files are not written."""
import json
import os
import queue
import threading
import time

import numpy as np

from spml_amd.utils.general import vis
from spml_amd.utils.general.vis import summary_grid_shape      # noqa: F401  (the picture's geometry, for callers)

SCALAR_KEYS = ('sem_ann_loss', 'sem_occ_loss', 'img_sim_loss', 'feat_aff_loss', 'accuracy', 'loss', 'lr')


def _number(value):
  return None if value is None else float(value)


class TrainingSummary:
  """`directory`: where the files go (created by the first `write`); `color_map`: uint8 `[<= 256, 3]`, numpy;
  `batch_images`: the global batch, for images_per_s."""

  def __init__(self, directory, color_map, batch_images):
    self.directory = directory
    table = np.zeros((256, 3), dtype=np.uint8)
    color_map = np.asarray(color_map, dtype=np.uint8)[:256]
    table[:color_map.shape[0]] = color_map
    self.color_map = table
    self.batch_images = int(batch_images)
    self._table_dev = None
    self._last = None                    # (wall clock, iteration) of the previous line
    self._queue = None
    self._thread = None
    self._failure = None

  @staticmethod
  def due(curr_iter, step):
    """The reference's rule (train.py:223) with `step == 0` meaning never."""
    return step > 0 and curr_iter % step == 0

  # ------------------------------------------------------------------
  def picture(self, semantic_label, instance_label, embedding):
    """uint8 `[3, Htot, Wtot]` on the embedding's device: the three launches."""
    import torch
    from spml_amd import ops
    embedding = embedding.detach()
    if not (embedding.is_contiguous() or embedding.is_contiguous(memory_format=torch.channels_last)):
      embedding = embedding.contiguous()
    if self._table_dev is None or self._table_dev.device != embedding.device:
      self._table_dev = torch.from_numpy(self.color_map).to(embedding.device)
    basis = vis.principal_components(embedding, 3)[0]
    proj, minmax = ops.pca_project_minmax(embedding, basis)
    return ops.summary_panels(semantic_label.contiguous(), instance_label.contiguous(), proj, minmax, self._table_dev)

  def _writer(self):
    from PIL import Image
    while True:
      item = self._queue.get()
      if item is None:
        return
      path, host, event = item
      try:
        if event is not None:
          event.synchronize()
        Image.fromarray(host.permute(1, 2, 0).contiguous().numpy()).save(path)      # uint8 [H, W, 3]: mode RGB
      except Exception as e:             # (reported by close(): a full disk must not kill the training silently)
        self._failure = e

  def _start(self):
    os.makedirs(self.directory, exist_ok=True)
    if self._thread is None:
      self._queue = queue.Queue()
      self._thread = threading.Thread(target=self._writer, name='summary-writer', daemon=True)
      self._thread.start()

  def write(self, curr_iter, semantic_label, instance_label, embedding, scalars):
    """The picture of this batch to `image-{iter:07d}.png` (through pinned memory and the writer thread) and one line to
    `scalars.jsonl`.  `scalars`: a dict with any of SCALAR_KEYS (tensors or numbers)."""
    import torch
    now = time.perf_counter()
    self._start()
    picture = self.picture(semantic_label, instance_label, embedding)
    event = None
    if picture.is_cuda:
      host = torch.empty(picture.shape, dtype=torch.uint8, pin_memory=True)
      host.copy_(picture, non_blocking=True)
      event = torch.cuda.Event()
      event.record()
    else:
      host = picture
    self._queue.put((os.path.join(self.directory, 'image-{:07d}.png'.format(curr_iter)), host, event))
    line = {'iter': int(curr_iter)}
    for key in SCALAR_KEYS:
      if scalars.get(key, None) is not None:
        line[key] = _number(scalars[key])
    steps = curr_iter - self._last[1] if self._last is not None else 0
    if steps > 0:
      seconds = now - self._last[0]
      line['step_ms'] = 1e3 * seconds / steps
      line['images_per_s'] = self.batch_images * steps / seconds if seconds > 0 else None
    else:
      line['step_ms'] = None
      line['images_per_s'] = None
    self._last = (now, curr_iter)
    with open(os.path.join(self.directory, 'scalars.jsonl'), 'a') as f:
      f.write(json.dumps(line) + '\n')
    return picture

  def close(self):
    """Drains the writer thread; raises what it failed with."""
    if self._thread is not None:
      self._queue.put(None)
      self._thread.join()
      self._thread = None
    if self._failure is not None:
      failure, self._failure = self._failure, None
      raise failure
