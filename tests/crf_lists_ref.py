"""numpy restatements for the dense CRF on image lists (csrc/inference_io.hip: crf_guide, label_export_scored).

  round_trip   pyscripts/inference/inference_softmax_crf_msc.py:159-164 of the reference, line for line: the uint8 image
               its CRF takes is rebuilt from the network's normalised float32 input
                   image = image.astype(np.float32); image *= stds; image += means; image = image * 255; astype(np.uint8)
               `stds` / `means` are float64 arrays (np.reshape of the config's Python lists), so numpy runs the two
               in-place steps in float64 and rounds each result to float32; `* 255` stays in float32.
  iou_counts   pyscripts/benchmark/benchmark_by_mIoU.py:25-53 under the rule of `spml_iou_counts_i64`: only pixels with
               truth < ncls count, a prediction >= ncls falls into no bin.

The views themselves are tests/inference_io_ref.py's."""
import numpy as np

import inference_io_ref as ref


def round_trip(image, mean, std):
  """image float [h, w, 3], normalised -> (uint8 [h, w, 3], the float32 value before the truncation as float64)."""
  image = np.array(image).astype(np.float32)
  image *= np.reshape(np.asarray(std, np.float64), (1, 1, 3))
  image += np.reshape(np.asarray(mean, np.float64), (1, 1, 3))
  image = image * 255
  assert image.dtype == np.float32
  return image.astype(np.int32).astype(np.uint8), image.astype(np.float64)


def byte_table(mean, std):
  """-> uint8 [256, 3]: the guide of byte b in channel c at the source's own size."""
  bytes_ = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)        # [256, 1, 3]
  return round_trip(ref.normalise_f32(bytes_, mean, std), mean, std)[0][:, 0, :]


def guide_same_size(rgb, mean, std):
  return round_trip(ref.normalise_f32(rgb, mean, std), mean, std)[0]


def guide_resized(rgb, new_hw, mean, std):
  """The fp64 view of tests/inference_io_ref.py, un-flipped and un-padded, through the round trip."""
  view = {'new_h': new_hw[0], 'new_w': new_hw[1], 'pad_h': new_hw[0], 'pad_w': new_hw[1], 'flip': 0}
  image, _ = ref.one_view(rgb, None, view, mean, std)
  return round_trip(image.transpose(1, 2, 0), mean, std)


def iou_counts(pred, truth, ncls):
  """uint8 maps of one size -> int64 [3, ncls]: TP+FN, TP+FP, TP."""
  pred, truth = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(truth).reshape(-1).astype(np.int64)
  counted = truth < ncls
  pred, truth = pred[counted], truth[counted]
  return np.stack([np.bincount(truth, minlength=ncls)[:ncls], np.bincount(pred[pred < ncls], minlength=ncls)[:ncls],
                   np.bincount(truth[pred == truth], minlength=ncls)[:ncls]]).astype(np.int64)
