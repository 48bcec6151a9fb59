"""Colour maps of the label images (`spml/utils/general/vis.py:51-59`)."""
import os

import numpy as np


def load_color_map(color_map_path):
  """The table of a `.mat` file -> uint8 `[N, 3]` numpy array: the entry named after the file (its base name with the
  characters of '.mat' stripped from both ends, as the reference takes it), times 255, truncated to uint8."""
  import scipy.io
  color_map = scipy.io.loadmat(color_map_path)
  color_map = color_map[os.path.basename(color_map_path).strip('.mat')]
  return (color_map * 255).astype(np.uint8)


def voc_color_map():
  """The 256-entry PASCAL VOC table (bit-interleave of the class index: bit k of the index goes to bit 7 - k / 3 of
  channel k % 3), uint8 `[256, 3]`; what the programs colour with when `dataset.color_map_path` is empty.  Entry for
  entry the table of the reference's `misc/colormapvoc.mat` (tests/golden/n14_inference_io.npz)."""
  table = np.zeros((256, 3), dtype=np.uint8)
  for index in range(256):
    c = index
    for shift in range(7, -1, -1):
      for channel in range(3):
        table[index, channel] |= ((c >> channel) & 1) << shift
      c >>= 3
  return table
