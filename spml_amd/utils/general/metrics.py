"""Segmentation metrics of `pyscripts/benchmark/benchmark_by_mIoU.py`: per-class (TP+FN, TP+FP, TP) counts on the
device (csrc/softmax_head.hip, integer atomics) and the mIoU / pixel-accuracy lines on the host."""
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
