#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by nearest-neighbour retrieval, with the reference's command
line and config surface (`pyscripts/inference/inference_msc.py:35-255` of twke18/SPML), the form the recipes report
their kNN numbers through:

  python3 pyscripts/inference/inference_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:83-89) and the prototype memory bank from
`--semantic_memory_dir` (`segsort_others.load_memory_banks`, the ignore class dropped: :92-111).  Every image becomes
ten views (scales 0.5, 0.75, 1, 1.25, 1.5, each flipped and plain,
zero-padded to the crop size: :123-137) and goes through `spml_amd.inference.predict_knn_multiscale` (per view the
sliding-window embedding, k-means over the un-padded view, top-20 retrieval per segment and one HIP launch pair for
votes, resize, un-flip and sum; then the mean over the views and one arg-max).  `--data_dir D --data_list L`
reads the reference's file list (`ListDataset`): all ten views of a file are made on the GPU from its decoded bytes by
one launch (`spml_amd.inference.device_views`), the label map is written as `semantic_gray/<name>.png` and
`semantic_color/<name>.png` (`spml_amd.inference.export_label_map`), and `--semantic_memory_dir` is required.
`--data_list synthetic` feeds seeded synthetic images of `test.image_size` through `spml_amd.inference.flip_scale_views`
and writes `semantic_gray/<name>.npy` (uint8).  Without `--semantic_memory_dir` the synthetic mode builds the bank
itself: the prototypes of the synthetic images (`full_resolution_prototypes`, what `prototype.py` does) are written with
`save_image_memory` to `<save_dir>/semantic_prototype` and read back from those files.  One JSON line reports images/s, mIoU and pixel accuracy
(`pyscripts/benchmark/benchmark_by_mIoU.py`), the number of views and the path taken by the per-view tail.
`--crf` (off by default) adds the denseCRF tail of `inference_crf_msc.py`, on either kind of `--data_list`: the view mean of the vote maps and the guide image at the file's own size through `spml_amd.inference.dense_crf_refine`; the labels written and scored are the refined ones and the JSON line gains `crf_path`, `crf_share`, `mIoU_before_crf` and `changed_by_crf` (see `run_knn` of spml_amd/inference_cli.py).
`--pseudo_tags` (off by default) makes the run the kNN pseudo-label step of the image-tag recipe, `pseudo_inference_msc.py`
(with `--crf`: `pseudo_inference_crf_msc.py`) on either kind of `--data_list`:

  python3 pyscripts/inference/inference_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_dir D \\
      --data_list L --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048 --pseudo_tags [--crf]

eight views (PSEUDO_SCALES, flipped and plain), the image tags from the classes of the file's label map -- the list needs
its label columns -- and `spml_amd.inference.pseudo_labels_knn_multiscale` (votes normalised per tagged class by their
maximum over the image, floored at PSEUDO_FLOOR); with `--crf` that normalised map is what the CRF refines.  The JSON line
gains `normalize_path`.  The instance-weighted IoU of a list is left to `pyscripts/benchmark/benchmark_by_instance.py` on
the written directory (the list source does not upload the instance plane); on synthetic images `instance_mIoU` is
reported as `pseudo_inference_msc.py` reports it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :125
PSEUDO_SCALES, PSEUDO_FLOOR = [0.5, 1, 1.5, 2], 0.15                     # pseudo_inference_crf_msc.py:135, :260


def main(argv=None):
  from spml_amd.inference_cli import run_knn
  run_knn('Inference for semantic segmentation.', SCALES, True, argv,                         # :123-137
          pseudo_tags=(PSEUDO_SCALES, PSEUDO_FLOOR))


if __name__ == '__main__':
  main()
