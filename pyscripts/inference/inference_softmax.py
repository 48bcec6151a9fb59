#!/usr/bin/env python3
"""Inference for semantic segmentation by the softmax classifier, with the reference's command line and config
surface (`pyscripts/inference/inference_softmax.py:26-166` of twke18/SPML):

  python3 pyscripts/inference/inference_softmax.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:70-76): `embedding_model` through the reference's
name mapping (`resume=True`), `prediction_model` non-strictly -- a stage-1 `SegsortSoftmax` snapshot carries the same
`semantic_classifier.*` names next to entries this model does not have.  Every image goes through
`spml_amd.inference.predict_softmax_full_resolution` (sliding windows, HIP classifier head, summed logits, arg-max).
`--data_dir D --data_list L` reads the reference's file list (`ListDataset`): the view of every file is made on the GPU
from its decoded bytes (`spml_amd.inference.device_views`: normalised, resized to `test.image_size`, padded to the crop
size, :89-103) and the label map goes back to the file's own size (:148-152) as `semantic_gray/<name>.png` and
`semantic_color/<name>.png` (`spml_amd.inference.export_label_map`), the folders `benchmark_by_mIoU.py` scores.
`--data_list synthetic` feeds seeded synthetic images of `test.image_size` and writes `semantic_gray/<name>.npy` (uint8).
One JSON line reports images/s and, where labels exist, mIoU and pixel accuracy
(`pyscripts/benchmark/benchmark_by_mIoU.py`).
`--crf` (off by default) adds the denseCRF tail of `inference_softmax_crf.py`, on either kind of `--data_list`: the soft-max of the summed logits and the guide image at the un-padded `test.image_size` view through `spml_amd.inference.dense_crf_refine`; the labels written and scored are the refined ones and the JSON line gains `crf_path`, `crf_share`, `mIoU_before_crf` and `changed_by_crf` (see `run_softmax` of spml_amd/inference_cli.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

def main(argv=None):
  from spml_amd.inference_cli import run_softmax
  run_softmax('Inference for semantic segmentation.', [1], False, argv, single_view=True)      # :89-103


if __name__ == '__main__':
  main()
