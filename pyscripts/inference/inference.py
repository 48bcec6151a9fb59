#!/usr/bin/env python3
"""Single-view inference for semantic segmentation by nearest-neighbour retrieval, with the reference's command line and
config surface (`pyscripts/inference/inference.py:35-255` of twke18/SPML):

  python3 pyscripts/inference/inference.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory and the prototype memory bank from
`--semantic_memory_dir` (the ignore class dropped: :99-111).  Every image is zero-padded to the crop size and goes through
`spml_amd.inference.predict_full_resolution` (:136-237: sliding-window embedding, k-means over the whole image with the
padding ignored, top-20 retrieval per segment, majority vote, scatter to the pixels).  `--data_dir D --data_list L`
reads the reference's file list (`ListDataset`): the view of every file is made on the GPU from its decoded bytes
(`spml_amd.inference.device_views`: normalised, resized to `test.image_size`, padded, :124-142), the label map goes back
to the file's own size (:238-241) as `semantic_gray/<name>.png` and `semantic_color/<name>.png`
(`spml_amd.inference.export_label_map`), and `--semantic_memory_dir` is required.  `--data_list synthetic` feeds seeded
synthetic images of `test.image_size` (made at the network's size) and writes `semantic_gray/<name>.npy` (uint8); without
`--semantic_memory_dir` it builds the bank itself, as `inference_msc.py` does.  One JSON line
reports images/s, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`).
`--crf` (off by default) adds the denseCRF tail of `inference_crf.py`, on either kind of `--data_list`: the per-segment votes and the guide image at the un-padded `test.image_size` view through `spml_amd.inference.predict_knn_full_resolution_crf`, the label map going back to the file's size afterwards; the labels written and scored are the refined ones and the JSON line gains `crf_path`, `crf_share`, `mIoU_before_crf` and `changed_by_crf` (see `run_knn` of spml_amd/inference_cli.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd.inference_cli import run_knn
  run_knn('Inference for semantic segmentation.', [1], False, argv, single_view=True)          # :124-142


if __name__ == '__main__':
  main()
