"""From a file-list dataset to training batches on the GPU.

The host decodes files and draws parameters (a thread pool); a batch of raw uint8 arrays and their parameter records
is packed into ONE pinned staging buffer, goes up in ONE `non_blocking` copy, and two launches of csrc/augment.hip turn
it into the `(datas, targets)` dicts of `spml_amd.synth.make_batch`.  In the place of the reference's
`torch.utils.data.DataLoader(shuffle, num_workers, collate_fn)` (pyscripts/train/train.py:74-80)."""
import collections
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from spml_amd import _ffi, ops

MAX_THREADS = 16          # decode threads: what one command may use, whatever the machine has
_ALIGN = 16


def _align(n):
  return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def epoch_permutation(seed, epoch, n, shuffle=True):
  """The order of epoch `epoch`: a function of `(seed, epoch)` alone."""
  if not shuffle:
    return np.arange(n)
  return np.random.default_rng([int(seed), int(epoch)]).permutation(n)


def rank_positions(seed, n, batch_size, iteration, rank=0, world=1, shuffle=True):
  """`(epoch, index)` of the `batch_size` samples rank `rank` of `world` takes in `iteration`.  The epochs'
  permutations follow each other as one endless sequence; the ranks take its positions `rank::world`, `batch_size` per
  iteration -- so every batch is full: the sequence wraps into the next epoch where the reference's loader
  (`drop_last=False`) ends an epoch on a short batch."""
  out, perms = [], {}
  for i in range(batch_size):
    pos = (iteration * batch_size + i) * world + rank
    epoch, at = divmod(pos, n)
    if epoch not in perms:
      perms[epoch] = epoch_permutation(seed, epoch, n, shuffle)
    out.append((epoch, int(perms[epoch][at])))
  return out


def packed_layout(samples):
  """Byte layout of a batch in the staging buffer: the records first, then per image RGB, semantic and instance plane.
  -> (offsets per image, total bytes)."""
  at = _align(len(samples) * _ffi.AUGMENT_PARAMS.itemsize)
  offsets = []
  for image, _, _, _, _ in samples:
    px = image.shape[0] * image.shape[1]
    offsets.append((at, at + 3 * px, at + 4 * px))
    at = _align(at + 5 * px)
  return offsets, at


def pack(samples, buffer):
  """Writes the batch into `buffer` (uint8 numpy, 8-byte aligned, at least `packed_layout(samples)[1]` bytes).
  -> the records, a view of the buffer's head."""
  offsets, total = packed_layout(samples)
  assert buffer.dtype == np.uint8 and buffer.size >= total and buffer.ctypes.data % 8 == 0
  records = buffer[:len(samples) * _ffi.AUGMENT_PARAMS.itemsize].view(_ffi.AUGMENT_PARAMS)
  for k, ((image, sem, inst, plan, _), (o_img, o_sem, o_inst)) in enumerate(zip(samples, offsets)):
    if sem is None or inst is None:
      raise ValueError('training needs the semantic and the instance label of every image (a three-column list)')
    h, w = image.shape[:2]
    if image.shape != (h, w, 3) or sem.shape != (h, w) or inst.shape != (h, w) or (h, w) != (plan['h'], plan['w']):
      raise ValueError('image %r, labels %r / %r and plan %r do not agree' % (image.shape, sem.shape, inst.shape,
                                                                             (plan['h'], plan['w'])))
    buffer[o_img:o_img + 3 * h * w] = image.reshape(-1)
    buffer[o_sem:o_sem + h * w] = sem.reshape(-1)
    buffer[o_inst:o_inst + h * w] = inst.reshape(-1)
    records['image_off'][k], records['sem_off'][k], records['inst_off'][k] = o_img, o_sem, o_inst
    for name in ('h', 'w', 'new_h', 'new_w', 'start_h', 'start_w', 'flip', 'gray', 'blur'):
      records[name][k] = int(plan[name])
    records['reserved0'][k], records['reserved1'][k] = 0, 0.0
    records['weights'][k] = plan['weights']
  return records


def resolve_data_list(args, config):
  """What a training program reads: `(data_dir, data_list)` from `--data_dir` / `--data_list`, falling back to
  `config.dataset.data_dir` / `train_data_list`; None for `synthetic` or when none is given.  A list that does not exist
  ends the program, naming it."""
  import os
  data_list = args.data_list if args.data_list is not None else (config.dataset.train_data_list or None)
  if data_list in (None, 'synthetic'):
    return None
  if not os.path.isfile(data_list):
    raise SystemExit('data list not found: %s' % data_list)
  data_dir = args.data_dir if args.data_dir is not None else config.dataset.data_dir
  return data_dir or '', data_list


def training_batcher(dataset_class, source, config, device, rank=0, world=1, first_iteration=0, **dataset_args):
  """The batcher over the dataset a reference training program builds (pyscripts/train/train.py:63-80) from
  `source = resolve_data_list(...)`, or None where the program feeds synthetic batches."""
  if source is None:
    return None
  dataset = dataset_class(data_dir=source[0], data_list=source[1], img_mean=config.network.pixel_means,
                          img_std=config.network.pixel_stds, size=config.train.crop_size,
                          random_crop=config.train.random_crop, random_scale=config.train.random_scale,
                          random_mirror=config.train.random_mirror, training=True, **dataset_args)
  return DeviceBatcher(dataset, config.train.batch_size, device, rank=rank, world=world,
                       num_threads=config.num_threads, first_iteration=first_iteration,
                       shuffle=getattr(config.train, 'shuffle', True))


class DeviceBatcher:
  """Iterates `(datas, targets)` from `dataset` (a class of spml_amd.data.datasets in training mode).

  The batch of `iteration` is a function of `(dataset.seed, iteration, rank)`: which samples, in which epoch, with which
  draws -- a resumed run (`first_iteration`) continues the sequence, as `synthetic_batches` of the training program
  does.  `num_threads` decode threads (at most 16) read `prefetch` batches ahead; no worker processes: a forked child of
  a process that holds the GPU is not safe."""

  def __init__(self, dataset, batch_size, device, rank=0, world=1, num_threads=4, first_iteration=0, shuffle=True,
               prefetch=2):
    if len(dataset) < 1:
      raise ValueError('the data list is empty')
    self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
    self.rank, self.world, self.shuffle = int(rank), int(world), bool(shuffle)
    self.iteration, self.prefetch = int(first_iteration), max(1, int(prefetch))
    self.size = (int(dataset.size[0]), int(dataset.size[1]))
    self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(num_threads), MAX_THREADS)))
    self.mean = torch.tensor([float(v) for v in dataset.img_mean], dtype=torch.float32, device=self.device)
    self.std = torch.tensor([float(v) for v in dataset.img_std], dtype=torch.float32, device=self.device)
    self.remap = torch.from_numpy(np.ascontiguousarray(dataset.label_remap, dtype=np.uint8)).to(self.device)
    self._staging = [None, None]          # pinned buffers, used in turn; [tensor, event of its last copy]
    self._turn = 0
    self._queue = collections.deque()

  def positions(self, iteration):
    return rank_positions(self.dataset.seed, len(self.dataset), self.batch_size, iteration, self.rank, self.world,
                          self.shuffle)

  def _submit(self, iteration):
    return [self.pool.submit(self.dataset.get, index, epoch) for epoch, index in self.positions(iteration)]

  def _stage(self, nbytes):
    slot = self._staging[self._turn]
    if slot is not None:
      slot[1].synchronize()               # the copy that last read this buffer has finished
    if slot is None or slot[0].numel() < nbytes:
      slot = [torch.empty((nbytes + nbytes // 4,), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
      self._staging[self._turn] = slot
    self._turn ^= 1
    return slot

  def launch(self, samples):
    """Decoded samples -> the batch: pack, one copy, the two launches."""
    _, total = packed_layout(samples)
    with torch.cuda.device(self.device):
      stage, event = self._stage(total)
      records = pack(samples, stage.numpy())
      packed = torch.empty((total,), dtype=torch.uint8, device=self.device)
      packed.copy_(stage[:total], non_blocking=True)
      event.record()
      params_dev = packed[:records.size * _ffi.AUGMENT_PARAMS.itemsize]
      image, sem, inst = ops.augment_batch(packed, records, self.mean, self.std, self.remap, self.size,
                                           params_dev=params_dev)
      targets = {'semantic_label': sem, 'instance_label': inst}
      if self.dataset.with_tags:
        targets['semantic_tag'] = ops.augment_tags(packed, records, params_dev=params_dev)
    return {'image': image}, targets

  def batch(self, iteration):
    """The batch of one iteration, decoded now."""
    return self.launch([f.result() for f in self._submit(iteration)])

  def __iter__(self):
    return self

  def __next__(self):
    while len(self._queue) < self.prefetch:
      self._queue.append(self._submit(self.iteration + len(self._queue)))
    futures = self._queue.popleft()
    self.iteration += 1
    return self.launch([f.result() for f in futures])

  def close(self):
    for futures in self._queue:
      for f in futures:
        f.cancel()
    self._queue.clear()
    self.pool.shutdown(wait=True)
