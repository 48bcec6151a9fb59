"""Segmentation metrics of `pyscripts/benchmark/benchmark_by_mIoU.py`: per-class (TP+FN, TP+FP, TP) counts on the
device (csrc/softmax_head.hip, integer atomics) and the mIoU / pixel-accuracy lines on the host; and of
`pyscripts/benchmark/benchmark_by_instance.py`: the instance-weighted IoU the tag recipe scores its pseudo labels by."""
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
