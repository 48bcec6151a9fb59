"""fp64 numpy restatement of the image chain of the reference's inference programs: the yardstick of
csrc/inference_io.hip and of `spml_amd.inference.device_views` / `export_label_map`.

  views   base_dataset.py (uint8 / 255, mean, std) -> transforms.resize (cv2.INTER_LINEAR on the normalised image,
          INTER_NEAREST on the label; `create_image_pyramid`) -> mirror of the RESIZED arrays -> resize_with_pad(..., 0)
  export  inference_softmax.py:142-160: crop to the valid rectangle -> cv2.resize(INTER_NEAREST) -> colour table

cv2 is not installed where this suite is developed: the two resize modes are those of tests/augment_ref.py (held to
ATen on the CPU by tests/test_inference_io.py at the sizes used here); the sizes, the order and the flags are held to the
reference's own functions by tests/golden/n14_inference_io.npz.  The stages run FORWARDS over whole arrays -- the
kernels compose them backwards per output pixel, so the two share no code path."""
import numpy as np

import augment_ref


def normalise(rgb, mean, std):
  """uint8 [h, w, 3] -> float64 [h, w, 3]."""
  return (rgb.astype(np.float64) / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)


def normalise_f32(rgb, mean, std):
  """The same in fp32 operations, as the kernel's taps: what a view at the source's own size holds exactly."""
  return (rgb.astype(np.float32) / np.float32(255.0) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


def one_view(rgb, semantic, view, mean, std):
  """`view`: a mapping with new_h, new_w, pad_h, pad_w, flip.  -> (image float64 [3, pad_h, pad_w], label int64
  [new_h, new_w] or None)."""
  new_h, new_w = int(view['new_h']), int(view['new_w'])
  image = augment_ref.resize_linear(normalise(rgb, mean, std), new_h, new_w)
  label = None if semantic is None else augment_ref.resize_nearest(semantic, new_h, new_w)
  if int(view['flip']):
    image = image[:, ::-1, :]
    label = None if label is None else label[:, ::-1]
  image = augment_ref.resize_with_pad(image, (int(view['pad_h']), int(view['pad_w'])), 0)
  assert image.shape[:2] == (int(view['pad_h']), int(view['pad_w']))
  return image.transpose(2, 0, 1), None if label is None else np.ascontiguousarray(label).astype(np.int64)


def views(rgb, semantic, plan, mean, std):
  return [one_view(rgb, semantic, view, mean, std) for view in plan]


def export(prediction, valid_hw, out_hw, color_map):
  """prediction int [pred_h, pred_w] -> (gray uint8 [out_h, out_w], rgb uint8 [out_h, out_w, 3])."""
  valid = np.asarray(prediction)[:valid_hw[0], :valid_hw[1]].astype(np.uint8)
  gray = augment_ref.resize_nearest(valid, out_hw[0], out_hw[1])
  return gray, np.asarray(color_map)[gray]
