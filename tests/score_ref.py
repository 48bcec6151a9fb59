"""A numpy restatement, written here, of what `spml_score_batch_u8` computes per file (include/spml_hip.h) and of the
float64 accumulation of the two benchmark programs: the table formulation -- a `[ncls, ncls + 2]` table of (ground truth,
prediction bin) and a `[256, ncls + 1]` table of (instance id, ground truth or "outside").  tests/test_score_dirs.py
checks it against the reference's recorded results (tests/golden/n15_score_dirs.npz); the GPU tests check the kernel
against it on shapes the fixture does not hold."""
import numpy as np

NUM_IDS = 256


def file_stats(pred, gt, inst, ncls):
  """int64 `[4, ncls]`: TP+FN, TP+FP, TP and the instances per class of one file; `inst` None: row 3 is zero."""
  ncls = int(ncls)
  p = np.asarray(pred, dtype=np.uint8).reshape(-1).astype(np.int64)
  g = np.asarray(gt, dtype=np.uint8).reshape(-1).astype(np.int64)
  assert p.size == g.size
  counted = g < ncls
  q = np.minimum(p, ncls + 1)                                             # columns: the classes, "== ncls", "no bin"
  pair = np.bincount(g[counted] * (ncls + 2) + q[counted], minlength=ncls * (ncls + 2)).reshape(ncls, ncls + 2)
  out = np.zeros((4, ncls), dtype=np.int64)
  out[0] = pair.sum(1)
  out[1] = pair[:, :ncls].sum(0)
  out[1, ncls - 1] += pair[:, ncls].sum()                                 # the last bin is closed on the right ...
  out[2] = np.diagonal(pair[:, :ncls])                                    # ... but `pred == target` is not
  if inst is not None:
    s = np.asarray(inst, dtype=np.uint8).reshape(-1).astype(np.int64)
    assert s.size == g.size
    table = np.bincount(s * (ncls + 1) + np.where(counted, g, ncls), minlength=NUM_IDS * (ncls + 1))
    table = table.reshape(NUM_IDS, ncls + 1)
    occurs = table.sum(1) > 0
    if occurs.all():
      occurs[NUM_IDS - 1] = False                                         # `if i < 255` over the sorted unique ids
    major = table[:, :ncls].argmax(1)                                     # first maximum; 0 for an all-zero row
    out[3] = np.bincount(major[occurs], minlength=ncls)
  return out


def batch_stats(files, ncls):
  """int64 `[B, 4, ncls]` of a list of (pred, gt, inst or None)."""
  return np.stack([file_stats(p, g, s, ncls) for p, g, s in files])


def miou_result(stats):
  """benchmark_by_mIoU.py's float64 tail on `[B, 4, ncls]`: (iou in per cent, mean, pixel accuracy)."""
  ncls = stats.shape[2]
  tp_fn, tp_fp, tp = (np.zeros(ncls, dtype=np.float64) for _ in range(3))
  for one in stats:
    tp_fn += one[0]
    tp_fp += one[1]
    tp += one[2]
  iou = tp / (tp_fn + tp_fp - tp + 1e-12) * 100.0
  return iou, iou.sum() / ncls, tp.sum() / (tp_fp.sum() + 1e-12)


def instance_result(stats):
  """benchmark_by_instance.py's float64 tail on `[B, 4, ncls]`: (iou in per cent, mean, instances per class)."""
  ncls = stats.shape[2]
  iou, ninst = np.zeros(ncls, dtype=np.float64), np.zeros(ncls, dtype=np.float64)
  for one in stats:
    tp_fn, tp_fp, tp, n_ = (one[i].astype(np.float64) for i in range(4))
    iou += tp / (tp_fn + tp_fp - tp + 1e-12) * n_
    ninst += n_
  iou /= ninst + 1e-12
  iou *= 100
  return iou, iou.sum() / ncls, ninst


def pack(files, garbage=None):
  """(packed uint8 array, records) of a list of (pred, gt, inst or None): every plane at the next multiple of 16, the
  padding zero or, with `garbage` (a numpy Generator), random bytes.  The record type is `_ffi.SCORE_PARAMS`."""
  dtype = np.dtype([('pred_off', '<i8'), ('gt_off', '<i8'), ('inst_off', '<i8'), ('n', '<i8')])
  total = sum(((np.asarray(p).size + 15) // 16 * 16) * (2 if s is None else 3) for p, g, s in files)
  packed = np.zeros(total, dtype=np.uint8) if garbage is None else garbage.integers(0, 256, size=total, dtype=np.uint8)
  records = np.zeros(len(files), dtype=dtype)
  at = 0
  for b, (p, g, s) in enumerate(files):
    n = np.asarray(p).size
    records[b]['n'] = n
    records[b]['inst_off'] = -1
    for name, plane in (('pred_off', p), ('gt_off', g), ('inst_off', s)):
      if plane is None:
        continue
      packed[at:at + n] = np.asarray(plane, dtype=np.uint8).reshape(-1)
      records[b][name] = at
      at += (n + 15) // 16 * 16
  return packed, records
