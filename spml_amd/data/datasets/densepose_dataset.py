"""DensePose datasets (`spml/data/datasets/densepose_dataset.py`)."""
import numpy as np

from spml_amd.data.datasets.base_dataset import ListDataset


class DenseposeDataset(ListDataset):
  """`ListDataset` whose mirrored part labels swap left and right (densepose_dataset.py:73-76,92)."""

  def __init__(self,
               data_dir,
               data_list,
               img_mean=(0, 0, 0),
               img_std=(1, 1, 1),
               size=None,
               random_crop=False,
               random_scale=False,
               random_mirror=False,
               training=False,
               seed=235):
    super(DenseposeDataset, self).__init__(
        data_dir, data_list, img_mean, img_std, size, random_crop, random_scale, random_mirror, training, seed)
    self.part_label_remap = np.arange(256, dtype=np.uint8)
    self.part_label_remap[:15] = [0, 1, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 14]
    self.label_remap = self.part_label_remap


class DenseposeClassifierDataset(DenseposeDataset):
  """For the softmax classifier: a wider scale range (densepose_dataset.py:174), random grayscale and random blur."""
  scale_range = (0.5, 2.0)

  def __init__(self,
               data_dir,
               data_list,
               img_mean=(0, 0, 0),
               img_std=(1, 1, 1),
               size=None,
               random_crop=False,
               random_scale=False,
               random_mirror=False,
               random_grayscale=False,
               random_blur=False,
               training=False,
               seed=235):
    super(DenseposeClassifierDataset, self).__init__(
        data_dir, data_list, img_mean, img_std, size, random_crop, random_scale, random_mirror, training, seed)
    self.random_grayscale = random_grayscale
    self.random_blur = random_blur
