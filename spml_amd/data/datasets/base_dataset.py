"""Base class of the file-list datasets (`spml/data/datasets/base_dataset.py`).

The reference's class decodes a file, augments it with numpy / cv2 on the host and returns the finished fp32 image.
Here the host only decodes and draws: `__getitem__` returns the raw uint8 arrays, the plan of the augmentation
(spml_amd/data/transforms.py) and the index; `spml_amd.data.DeviceBatcher` packs a batch of them and one launch of
csrc/augment.hip makes the pixels."""
import os

import numpy as np
import PIL.Image as Image

import spml_amd.data.transforms as transforms


class ListDataset:
  """Takes a file of paired lists of images, semantic labels and instance labels."""

  scale_range = (0.5, 1.5)       # base_dataset.py:147
  with_tags = False              # base_dataset.py:187-188: no `semantic_tag` among the labels

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
    """The reference's arguments (base_dataset.py:20-58) and `seed`, the first of the three numbers
    `(seed, epoch, index)` a sample's augmentation is drawn from."""
    self.image_paths, self.semantic_label_paths, self.instance_label_paths = (
        self._read_image_and_label_paths(data_dir, data_list))
    self.training = training
    self.img_mean = img_mean
    self.img_std = img_std
    self.size = size
    self.random_crop = random_crop
    self.random_scale = random_scale
    self.random_mirror = random_mirror
    self.random_grayscale = False
    self.random_blur = False
    self.seed = seed
    self.label_remap = np.arange(256, dtype=np.uint8)      # what a mirrored semantic label becomes: itself

  def eval(self):
    self.training = False

  def train(self):
    self.training = True

  def _read_image_and_label_paths(self, data_dir, data_list):
    """base_dataset.py:70-100: 'image semantic_label instance_label' per line, or the image alone."""
    images, semantic_labels, instance_labels = [], [], []
    with open(data_list, 'r') as list_file:
      for line in list_file:
        line = line.strip('\n')
        parts = line.split(' ')
        if len(parts) == 3:
          img, semantic_lab, instance_lab = parts
        else:
          img, semantic_lab, instance_lab = line, None, None
        images.append(os.path.join(data_dir, img))
        if semantic_lab is not None:
          semantic_labels.append(os.path.join(data_dir, semantic_lab))
        if instance_lab is not None:
          instance_labels.append(os.path.join(data_dir, instance_lab))
    return images, semantic_labels, instance_labels

  def _read_image(self, image_path):
    """RGB uint8 [h, w, 3] (base_dataset.py:105; the division by 255 is the kernel's)."""
    return np.array(Image.open(image_path).convert(mode='RGB'))

  def _read_label(self, label_path):
    """uint8 [h, w] (base_dataset.py:112)."""
    return np.array(Image.open(label_path).convert(mode='L'))

  def _get_datas_by_index(self, idx):
    image = self._read_image(self.image_paths[idx])
    semantic_label = self._read_label(self.semantic_label_paths[idx]) if self.semantic_label_paths else None
    instance_label = self._read_label(self.instance_label_paths[idx]) if self.instance_label_paths else None
    return image, semantic_label, instance_label

  def read(self, idx):
    """-> (rgb uint8 [h, w, 3], semantic_label, instance_label uint8 [h, w] or None): the decoded files of entry `idx`,
    in either mode.  What the inference programs take (`spml_amd.inference_cli.ImageSource`): their views are made on
    the GPU from these bytes (csrc/inference_io.hip)."""
    return self._get_datas_by_index(idx)

  def plan(self, idx, h, w, epoch=0):
    """The parameter record of sample `idx` in `epoch` for an `h x w` file."""
    return transforms.plan_training(
        transforms.sample_rng(self.seed, epoch, idx), h, w, self.size, self.random_mirror, self.random_scale,
        self.random_crop, self.scale_range, self.random_grayscale, self.random_blur, name=self.image_paths[idx])

  def get(self, idx, epoch=0):
    """-> (image uint8 [h, w, 3], semantic_label, instance_label uint8 [h, w] or None, plan, idx)."""
    if not self.training:
      raise NotImplementedError('only the training mode is built: the inference programs read their own files')
    image, semantic_label, instance_label = self._get_datas_by_index(idx)
    return image, semantic_label, instance_label, self.plan(idx, image.shape[0], image.shape[1], epoch), idx

  def __len__(self):
    return len(self.image_paths)

  def __getitem__(self, idx):
    return self.get(idx, 0)
