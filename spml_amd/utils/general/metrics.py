"""Segmentation metrics of `pyscripts/benchmark/benchmark_by_mIoU.py`: per-class (TP+FN, TP+FP, TP) counts on the
device (csrc/softmax_head.hip, integer atomics) and the mIoU / pixel-accuracy lines on the host; and of
`pyscripts/benchmark/benchmark_by_instance.py`: the instance-weighted IoU the tag recipe scores its pseudo labels by.
The functions above `DirectoryScorer` take one image's int64 maps on the device; `DirectoryScorer` and
`score_directories` take directories of label files, a batch of files per call (csrc/score_batch.hip)."""
import io
import os

import numpy as np
import torch

from spml_amd import _ffi


def iou_stats(pred, target, num_classes, counts=None):
  """benchmark_by_mIoU.py:25-53 for device label maps of equal size: int64 `[3, num_classes]` = (TP+FN, TP+FP, TP)
  over the pixels with `0 <= target < num_classes`.  Given `counts` (the result of an earlier call) the image is
  added into it, the way the reference's loop sums over the images (:86-88)."""
  pred = pred.reshape(-1).to(torch.int64).contiguous()
  target = target.reshape(-1).to(torch.int64).contiguous()
  return _ffi.iou_counts(pred, target, num_classes, counts)


def mean_iou(counts):
  """benchmark_by_mIoU.py:90,113,116 in float64 on the host: `counts` `[3, num_classes]` (tensor or array) ->
  {'iou': per-class IoU in per cent, 'mean_iou': their mean, 'pixel_acc': TP / (TP+FP) as the reference prints it}."""
  c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
  tp_fn, tp_fp, tp = (c[i].astype(np.float64) for i in range(3))
  iou = tp / (tp_fn + tp_fp - tp + 1e-12) * 100.0
  return {'iou': iou, 'mean_iou': float(iou.sum() / iou.shape[0]), 'pixel_acc': float(tp.sum() / (tp_fp.sum() + 1e-12))}


NUM_INSTANCE_IDS = 256                 # instance maps are 8-bit (benchmark_by_instance.py:84-86)


def instance_class_counts(inst, gt, num_classes):
  """benchmark_by_instance.py:97-108 for device maps of equal size: int64 `[num_classes]`, the number of instance ids
  whose most frequent ground-truth class is c.  The instance id (0 .. 255) is the segment of
  `spml_segment_majority_i64`; the reference's quirks are kept: id 0 is an instance like any other; a pixel whose
  ground truth is outside `[0, num_classes)` is counted for no class (the histogram's range, :104-106), so an id that
  has no other pixel counts for class 0 (the arg-max of an all-zero histogram); ties go to the lowest class; an id that
  does not occur counts nowhere; and when all 256 ids occur the largest is dropped (`if i < 255`, :100).  No host read."""
  inst = inst.reshape(-1).to(torch.int64).contiguous()
  gt = gt.reshape(-1).to(torch.int64).contiguous()
  major = _ffi.segment_majority(inst, gt, NUM_INSTANCE_IDS, int(num_classes))
  occurs = torch.bincount(inst.clamp(0, NUM_INSTANCE_IDS - 1), minlength=NUM_INSTANCE_IDS) > 0
  occurs[NUM_INSTANCE_IDS - 1] &= ~occurs.all()
  return torch.zeros((int(num_classes),), dtype=torch.int64, device=inst.device).scatter_add_(0, major, occurs.long())


class InstanceIoU:
  """The accumulator of benchmark_by_instance.py:66-67, 88-116, 139: per image the IoU of that image's own counts
  (`iou_stats` with `counts=None`) weighted per class by the image's instance counts, in float64 on the host.  One
  device -> host copy of `[4, num_classes]` int64 per image."""

  def __init__(self, num_classes):
    self.num_classes = int(num_classes)
    self.iou = np.zeros(self.num_classes, dtype=np.float64)
    self.ninst = np.zeros(self.num_classes, dtype=np.float64)

  def update(self, pred, gt, inst):
    stats = iou_stats(pred, gt, self.num_classes)
    ninst = instance_class_counts(inst, gt, self.num_classes)
    c = torch.cat([stats, ninst.view(1, -1)], 0).cpu().numpy().astype(np.float64)
    tp_fn, tp_fp, tp, ninst_ = c[0], c[1], c[2], c[3]
    self.iou += tp / (tp_fn + tp_fp - tp + 1e-12) * ninst_                       # :111-112
    self.ninst += ninst_                                                         # :113
    return ninst_

  def result(self):
    """{'iou': per-class instance-weighted IoU in per cent, 'mean_iou': their mean (:115-116, :139), 'ninst'}."""
    iou = self.iou / (self.ninst + 1e-12) * 100.0
    return {'iou': iou, 'mean_iou': float(iou.sum() / self.num_classes), 'ninst': self.ninst.copy()}


# ---------------------------------------------------------------------------
# Scoring whole directories of label files: the loops of benchmark_by_mIoU.py:66-88 and benchmark_by_instance.py:68-113
# with the per-file arithmetic of a batch of files in one `_ffi.score_batch` call (csrc/score_batch.hip).

class ScoreInputError(ValueError):
  """A directory, a file or a pair of files the scorer cannot use; the message names the path."""


def mapped_name(predname, pred_dir, other_dir, string_replace=','):
  """benchmark_by_mIoU.py:69-72: the ground-truth (or instance) file of a prediction -- `str.replace` of the directory
  prefix on the WHOLE path (every occurrence, as there), then the `a,b` replacement of --string_replace."""
  name = predname.replace(pred_dir, other_dir)
  if string_replace != '':
    parts = string_replace.split(',')
    if len(parts) != 2:
      raise ScoreInputError("--string_replace takes 'a,b' (got '%s')" % string_replace)
    name = name.replace(parts[0], parts[1])
  return name


def directory_triples(pred_dir, gt_dir, inst_dir=None, string_replace=','):
  """[(prediction, ground truth, instance mask or None)] in `os.walk` order of `pred_dir` (:66-72).  Raises
  ScoreInputError for a directory that is none, an empty prediction directory and a prediction whose partner is missing."""
  for what, d in (('--pred_dir', pred_dir), ('--gt_dir', gt_dir)) + ((('--inst_dir', inst_dir),) if inst_dir is not None else ()):
    if not os.path.isdir(d):
      raise ScoreInputError("%s '%s' is not a directory" % (what, d))
  triples = []
  for dirpath, _, filenames in os.walk(pred_dir):
    for filename in filenames:
      predname = os.path.join(dirpath, filename)
      gtname = mapped_name(predname, pred_dir, gt_dir, string_replace)
      if not os.path.isfile(gtname):
        raise ScoreInputError("prediction '%s' has no ground truth '%s'" % (predname, gtname))
      instname = None
      if inst_dir is not None:
        instname = mapped_name(predname, pred_dir, inst_dir, string_replace)
        if not os.path.isfile(instname):
          raise ScoreInputError("prediction '%s' has no instance mask '%s'" % (predname, instname))
      triples.append((predname, gtname, instname))
  if not triples:
    raise ScoreInputError("prediction directory '%s' holds no file" % pred_dir)
  return triples


def check_sizes(triples, threads=16):
  """The files of one triple must have one size (the reference dies inside numpy's boolean indexing there): read from
  the files' headers, nothing is decoded.  Raises ScoreInputError naming the first offending pair in the list's order."""
  from concurrent.futures import ThreadPoolExecutor
  from PIL import Image

  def size_of(source):
    with Image.open(io.BytesIO(source) if isinstance(source, (bytes, bytearray)) else source) as im:
      return im.size[1], im.size[0]

  def one(triple):
    sizes = [size_of(s) for s in triple if s is not None]
    for what, source, size in zip(('ground truth', 'instance mask'), triple[1:], sizes[1:]):
      if size != sizes[0]:
        return "prediction '%s' is %d x %d but its %s '%s' is %d x %d" % (
            (_name_of(triple[0]),) + sizes[0] + (what, _name_of(source)) + size)
    return None

  with ThreadPoolExecutor(max_workers=max(1, int(threads))) as pool:
    for message in pool.map(one, triples):
      if message is not None:
        raise ScoreInputError(message)


def decode_label(source, mode):
  """uint8 `[h, w]` of a label file as the reference reads it (:74-79; benchmark_by_instance.py:84-86): PIL's conversion
  to `mode` -- 'L' for predictions and ground truth, 'P' for instance masks.  `source`: a path, or the file's bytes."""
  from PIL import Image
  with Image.open(io.BytesIO(source) if isinstance(source, (bytes, bytearray)) else source) as im:
    return np.asarray(im.convert(mode=mode), dtype=np.uint8)


def _name_of(source):
  return '<%d bytes>' % len(source) if isinstance(source, (bytes, bytearray)) else str(source)


def _pad16(n):
  return (n + _ffi.SCORE_PLANE_ALIGN - 1) // _ffi.SCORE_PLANE_ALIGN * _ffi.SCORE_PLANE_ALIGN


class DirectoryScorer:
  """Scores (prediction, ground truth[, instance mask]) files on the GPU.  The host only decodes, ahead on a thread
  pool; the raw planes of up to `batch_files` files (and at most `batch_bytes` of planes, one file at least) are staged
  with their records in ONE pinned buffer: one upload, one `_ffi.score_batch` call and one download of `[B, 4, ncls]`
  int64 per batch.  The float64 accumulation on the host is the two reference programs':
    benchmark_by_mIoU.py:86-90,113,116      counts summed over the files, tp / (tp_fn + tp_fp - tp + 1e-12) * 100,
                                            tp.sum() / (tp_fp.sum() + 1e-12)
    benchmark_by_instance.py:111-116,139    every file's own IoU times its instance counts, / (ninst + 1e-12) * 100."""

  def __init__(self, num_classes, batch_files=64, batch_bytes=64 << 20, decode_threads=16, device=None):
    if not torch.cuda.is_available():
      raise _ffi.SpmlHipError('scoring directories needs an MI355X (the HIP path has no CPU fallback)')
    self.num_classes = int(num_classes)
    self.batch_files = max(1, min(int(batch_files), _ffi.MAX_SCORE_FILES))
    self.batch_bytes = int(batch_bytes)
    self.decode_threads = max(1, int(decode_threads))
    self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    self._staging = None
    self.reset()

  def reset(self):
    n = self.num_classes
    self.tp_fn, self.tp_fp, self.tp = (np.zeros(n, dtype=np.float64) for _ in range(3))
    self.inst_iou, self.ninst = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    self.files = self.batches = self.upload_bytes = self.download_bytes = 0
    self.score_path = None
    self.with_instances = False

  @staticmethod
  def _decode(triple):
    pred_src, gt_src, inst_src = triple
    pred, gt = decode_label(pred_src, 'L'), decode_label(gt_src, 'L')
    if pred.shape != gt.shape:
      raise ScoreInputError("prediction '%s' is %d x %d but its ground truth '%s' is %d x %d"
                            % (_name_of(pred_src), pred.shape[0], pred.shape[1], _name_of(gt_src), gt.shape[0], gt.shape[1]))
    inst = None
    if inst_src is not None:
      inst = decode_label(inst_src, 'P')
      if inst.shape != gt.shape:
        raise ScoreInputError("prediction '%s' is %d x %d but its instance mask '%s' is %d x %d"
                              % (_name_of(pred_src), pred.shape[0], pred.shape[1], _name_of(inst_src), inst.shape[0], inst.shape[1]))
    if pred.size < 1:
      raise ScoreInputError("prediction '%s' holds no pixel" % _name_of(pred_src))
    return pred, gt, inst

  @staticmethod
  def _planes_bytes(decoded):
    return _pad16(decoded[0].size) * (2 if decoded[2] is None else 3)

  def score_batch(self, batch):
    """One batch of decoded (pred, gt, inst or None) uint8 arrays: staged, uploaded, scored, accumulated.  Returns the
    batch's `[B, 4, ncls]` int64 array."""
    planes = sum(self._planes_bytes(d) for d in batch)
    rec_bytes = len(batch) * _ffi.SCORE_PARAMS.itemsize
    if self._staging is None or self._staging.numel() < planes + rec_bytes:
      need = planes + rec_bytes                              # (a quarter of slack: batches of like files differ little)
      self._staging = torch.empty((need + need // 4,), dtype=torch.uint8).pin_memory()
    stage = self._staging.numpy()
    records = np.zeros(len(batch), dtype=_ffi.SCORE_PARAMS)
    at = 0
    for b, (pred, gt, inst) in enumerate(batch):
      n = pred.size
      records[b]['n'], records[b]['inst_off'] = n, -1
      for name, plane in (('pred_off', pred), ('gt_off', gt), ('inst_off', inst)):
        if plane is None:
          continue
        stage[at:at + n] = plane.reshape(-1)
        records[b][name] = at
        at += _pad16(n)
    assert at == planes
    stage[planes:planes + rec_bytes] = records.view(np.uint8).reshape(-1)
    if self.score_path is None:
      self.score_path = _ffi.score_batch_path_name(records, planes, self.num_classes)
    with torch.cuda.device(self.device):
      dev = self._staging[:planes + rec_bytes].to(self.device, non_blocking=True)
      stats = _ffi.score_batch(dev[:planes], records, self.num_classes, params_dev=dev[planes:])
      table = stats.cpu().numpy()                            # (blocks: the staging buffer is free again after it)
    self.batches += 1
    self.upload_bytes += planes + rec_bytes
    self.download_bytes += table.nbytes
    for (pred, gt, inst), one in zip(batch, table):
      tp_fn, tp_fp, tp, ninst_ = (one[i].astype(np.float64) for i in range(4))
      self.tp_fn += tp_fn
      self.tp_fp += tp_fp
      self.tp += tp
      if inst is not None:
        self.with_instances = True
        self.inst_iou += tp / (tp_fn + tp_fp - tp + 1e-12) * ninst_
        self.ninst += ninst_
    self.files += len(batch)
    return table

  def score(self, triples):
    """Adds every (prediction, ground truth, instance mask or None) of `triples` -- paths or the files' bytes -- in
    their order; decoding runs up to two batches ahead of the GPU."""
    from concurrent.futures import ThreadPoolExecutor
    triples = list(triples)
    ahead = 2 * self.batch_files
    with ThreadPoolExecutor(max_workers=self.decode_threads) as pool:
      pending = [pool.submit(self._decode, t) for t in triples[:ahead]]
      submitted, batch, batch_planes = len(pending), [], 0
      try:
        for i in range(len(triples)):
          decoded = pending[i].result()
          pending[i] = None
          if submitted < len(triples):
            pending.append(pool.submit(self._decode, triples[submitted]))
            submitted += 1
          size = self._planes_bytes(decoded)
          if batch and (len(batch) == self.batch_files or batch_planes + size > self.batch_bytes):
            self.score_batch(batch)
            batch, batch_planes = [], 0
          batch.append(decoded)
          batch_planes += size
        if batch:
          self.score_batch(batch)
      finally:
        for f in pending:
          if f is not None:
            f.cancel()
    return self

  def result(self):
    """{'iou': per-class IoU in per cent, 'mean_iou', 'pixel_acc' (the mIoU program's numbers); 'inst_iou',
    'inst_mean_iou', 'ninst' (the instance program's; zero without instance masks); 'files', 'batches', 'score_path',
    'upload_bytes', 'download_bytes'}."""
    out = mean_iou(np.stack([self.tp_fn, self.tp_fp, self.tp]))
    inst_iou = self.inst_iou / (self.ninst + 1e-12)
    inst_iou *= 100
    out.update(inst_iou=inst_iou, inst_mean_iou=float(inst_iou.sum() / self.num_classes), ninst=self.ninst.copy(),
               files=self.files, batches=self.batches, score_path=self.score_path, upload_bytes=self.upload_bytes,
               download_bytes=self.download_bytes)
    return out


def score_directories(pred_dir, gt_dir, num_classes, inst_dir=None, string_replace=',', **scorer_args):
  """The whole of either benchmark program but its printing: walks `pred_dir`, maps the names, scores every file."""
  triples = directory_triples(pred_dir, gt_dir, inst_dir, string_replace)
  check_sizes(triples, scorer_args.get('decode_threads', 16))
  return DirectoryScorer(num_classes, **scorer_args).score(triples).result()
