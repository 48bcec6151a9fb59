"""Datasets with image-level tags (`spml/data/datasets/list_tag_dataset.py`)."""
from spml_amd.data.datasets.base_dataset import ListDataset


class ListTagDataset(ListDataset):
  """`ListDataset` whose batches also carry `semantic_tag`, the multi-hot of the values in the un-augmented semantic
  label (list_tag_dataset.py:75-78; made on the GPU by `spml_augment_tags_u8`)."""
  with_tags = True


class ListTagClassifierDataset(ListTagDataset):
  """For the softmax classifier: a wider scale range (list_tag_dataset.py:194), random grayscale and random blur."""
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
    super(ListTagClassifierDataset, self).__init__(
        data_dir, data_list, img_mean, img_std, size, random_crop, random_scale, random_mirror, training, seed)
    self.random_grayscale = random_grayscale
    self.random_blur = random_blur
