#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by the softmax classifier, with the reference's command line
and config surface (`pyscripts/inference/inference_softmax_msc.py:29-167` of twke18/SPML), the form every stage-2 recipe
reports its number through:

  python3 pyscripts/inference/inference_softmax_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:70-76): `embedding_model` through the reference's
name mapping (`resume=True`), `prediction_model` non-strictly -- a stage-1 `SegsortSoftmax` snapshot carries the same
`semantic_classifier.*` names next to entries this model does not have.  Every image becomes ten views (scales 0.5, 0.75, 1, 1.25, 1.5, each flipped and plain, zero-padded to the crop
size: :90-103) and goes through `spml_amd.inference.predict_softmax_multiscale` (sliding windows and the HIP classifier
head per view, one HIP kernel per view for counts, crop, resize, softmax, un-flip and sum, one arg-max).  
`--data_dir D --data_list L` reads the reference's file list (`ListDataset`): all ten views of a file are made on the GPU
from its decoded bytes by one launch (`spml_amd.inference.device_views`) and the label map is written as
`semantic_gray/<name>.png` and `semantic_color/<name>.png` (`spml_amd.inference.export_label_map`), the folders
`benchmark_by_mIoU.py` scores.  `--data_list synthetic` feeds seeded synthetic images of `test.image_size` through
`spml_amd.inference.flip_scale_views` and writes `semantic_gray/<name>.npy` (uint8).  One JSON line reports images/s, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`), the number of
views and the paths taken by the classifier head and by the per-view tail.
`--crf` (off by default) adds the denseCRF tail of `inference_softmax_crf_msc.py`, on either kind of `--data_list`: the mean of the views' class probabilities and the guide image at the file's own size through `spml_amd.inference.dense_crf_refine`; the labels written and scored are the refined ones and the JSON line gains `crf_path`, `crf_share`, `mIoU_before_crf` and `changed_by_crf` (see `run_softmax` of spml_amd/inference_cli.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :92


def main(argv=None):
  from spml_amd.inference_cli import run_softmax
  run_softmax('Inference for semantic segmentation.', SCALES, True, argv)                      # :90-103


if __name__ == '__main__':
  main()
